"""Worker of tests/test_nce_distributed_cpu.py: the sharded per-sample InfoNCE (distributed.GlobalBatchNceFn) over gloo,
with an fp64 ops object that implements the row-block protocol of the HIP ops (nce_forward / nce_merge / nce_backward,
the same part layout) from the definition in tests/nce_reference.py.  What it checks is the exchange: the gathers, the
rank-ordered merge of the parts, the reduce-scatter of dY and the all-reduce of the parameter gradients."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mutual-information-multimodal_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

NEG_INF = float("-inf")


def bilinear_scores(x, y, w):
    return (x @ w) @ y.t()


def separable_scores(x, y, wg, wh):
    return (x @ wg) @ (y @ wh).t()


SCORERS = {"bilinear": bilinear_scores, "separable": separable_scores}


def id_pattern(name: str, b: int, b_local: int) -> torch.Tensor:
    sid = torch.arange(b, dtype=torch.int64) * 7 + 3
    if name == "dup_in_rank":        # equal ids inside one rank's rows
        sid[1] = sid[0]
        sid[b_local + 2] = sid[b_local + 1]
    elif name == "dup_across":       # equal ids on two ranks
        sid[b - 1] = sid[0]
        sid[b_local] = sid[b_local - 1]
    elif name == "majority":         # every row but the last shares one id: a rank whose rows are all in the group has
        sid[:-1] = 11                # no candidate for the group's columns (an empty partial)
    elif name == "all_equal":        # no negatives anywhere: every term, the loss and every gradient are 0
        sid[:] = 5
    elif name != "unique":
        raise ValueError(name)
    return sid


PATTERNS = ("unique", "dup_in_rank", "dup_across", "majority", "all_equal")


def problem(critic: str, b: int, d: int, k: int, salt: int):
    gen = torch.Generator().manual_seed(1000 + salt)
    x = torch.randn(b, d, generator=gen, dtype=torch.float64)
    y = torch.randn(b, d + 1, generator=gen, dtype=torch.float64)
    if critic == "bilinear":
        params = [0.3 * torch.randn(d, d + 1, generator=gen, dtype=torch.float64)]
    else:
        params = [0.4 * torch.randn(d, k, generator=gen, dtype=torch.float64),
                  0.4 * torch.randn(d + 1, k, generator=gen, dtype=torch.float64)]
    return x, y, params


class OracleNceOps:
    """fp64 stand-in for HipBilinearOps / HipSeparableOps in the row-block NCE protocol."""

    def __init__(self, critic: str):
        self.scorer = SCORERS[critic]

    def nce_forward(self, x, y_all, params, sid_rows, sid_all, row_offset, mode, precision, need_grad=True):
        with torch.enable_grad():  # called from inside an autograd.Function.forward, where grad mode is off
            leaves = [t.detach().clone().requires_grad_(True) for t in (x, y_all, *params)]
            s = self.scorer(*leaves)
        sd = s.detach()
        br, b = sd.shape
        gi = torch.arange(br) + row_offset
        pos = gi[:, None] == torch.arange(b)[None, :]
        cand = pos | (sid_rows[:, None] != sid_all[None, :])
        masked = torch.where(cand, sd, torch.full_like(sd, NEG_INF))
        r = torch.logsumexp(masked, dim=1)
        diag = sd[torch.arange(br), gi]
        m = masked.max(dim=0).values
        m_safe = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        ssum = torch.where(cand, torch.exp(masked - m_safe[None, :]), torch.zeros_like(sd)).sum(dim=0)
        part = torch.cat([torch.stack([m, ssum], dim=1).reshape(-1), r - diag, diag])
        return part, r, (leaves, s, cand, pos, r, mode, b)

    @staticmethod
    def nce_merge(parts, b_rows, mode):
        g = parts.shape[0]
        b = g * b_rows
        m, s = parts[:, 0:2 * b:2], parts[:, 1:2 * b:2]
        mm = m.max(dim=0).values
        scaled = torch.where(torch.isinf(m), torch.zeros_like(s), s * torch.exp(m - mm[None, :]))
        c = mm + torch.log(scaled.sum(dim=0))
        row_terms = parts[:, 2 * b:2 * b + b_rows].reshape(-1)
        diag = parts[:, 2 * b + b_rows:].reshape(-1)
        loss = row_terms.mean()
        if mode == 1:
            loss = 0.5 * loss + 0.5 * (c - diag).mean()
        return loss.reshape(1), c

    @staticmethod
    def nce_backward(saved, lse_cols, grad_out):
        leaves, s, cand, pos, r, mode, b = saved
        sd = s.detach()
        wr, wc = (1.0 / b, 0.0) if mode == 0 else (0.5 / b, 0.5 / b)
        c = cand.to(sd.dtype)
        g = wr * (c * torch.exp(sd - r[:, None]) - pos.to(sd.dtype))
        if mode == 1:
            g = g + wc * (c * torch.exp(sd - lse_cols[None, :]) - pos.to(sd.dtype))
        g = g * grad_out.to(sd.dtype)
        grads = torch.autograd.grad(s, leaves, g)
        return grads[0], grads[1], list(grads[2:])


def run(rank, world, port, b_local, d, k, critic, estimator, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mutual_info_img_txt.distributed import global_batch_mi_bound
    b = world * b_local
    sl = slice(rank * b_local, (rank + 1) * b_local)
    x, y, params = problem(critic, b, d, k, salt=b + d)
    out = {}
    for pattern in PATTERNS:
        sid = id_pattern(pattern, b, b_local)
        xl = x[sl].clone().requires_grad_(True)
        yl = y[sl].clone().requires_grad_(True)
        pl = [p.clone().requires_grad_(True) for p in params]
        loss, (lse_rows, lse_cols) = global_batch_mi_bound(xl, yl, sid[sl].contiguous(), pl, estimator, "f32",
                                                           critic=critic, group=dist.group.WORLD,
                                                           ops=OracleNceOps(critic), return_stats=True)
        assert tuple(loss.shape) == () and tuple(lse_rows.shape) == (b_local,) and tuple(lse_cols.shape) == (b,)
        loss.backward()
        with torch.no_grad():  # forward only: the same loss, nothing to differentiate
            again = global_batch_mi_bound(x[sl].clone(), y[sl].clone(), sid[sl].contiguous(), params, estimator, "f32",
                                          critic=critic, group=dist.group.WORLD, ops=OracleNceOps(critic))
        out[pattern] = {"loss": loss.detach().reshape(1), "lse_rows": lse_rows, "lse_cols": lse_cols, "dx": xl.grad,
                        "dy": yl.grad, "dparams": [p.grad for p in pl], "loss_no_grad": again.reshape(1),
                        "no_grad_requires_grad": bool(again.requires_grad)}
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()
