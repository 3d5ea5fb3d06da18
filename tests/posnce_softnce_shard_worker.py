"""Worker of tests/test_posnce_softnce_distributed_cpu.py: the sharded study-positive and soft-target InfoNCE
(distributed.GlobalBatchPosNceFn / distributed_label_targets.GlobalBatchSoftNceFn) over gloo, with an fp64 ops object that implements the row-block
protocol of the HIP ops (posnce_* / softnce_* forward, merge, backward; the same part layouts) from the definitions in
tests/posnce_reference.py and tests/softnce_reference.py.  What it checks is the exchange: the gathers of Y and the ids /
masks, the rank-ordered merge of the parts, the reduce-scatter of dY and the all-reduce of the parameter gradients."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mutual-information-multimodal_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import softnce_reference as sref  # noqa: E402
from nce_shard_worker import SCORERS, id_pattern, problem  # noqa: E402,F401

ID_PATTERNS = ("unique", "dup_in_rank", "dup_across", "majority", "all_equal")
# (mask pattern, tau, mix): mix = 0 in one case of seven; two values of tau
LABEL_CASES = (("random", 0.5, 0.5), ("random", 0.1, 1.0), ("zero", 0.5, 1.0), ("equal", 0.5, 1.0),
               ("one_bit_per_study", 0.1, 1.0), ("bit63", 0.5, 0.5), ("random", 0.5, 0.0))


def label_pattern(name: str, b: int, b_local: int) -> torch.Tensor:
    """int64 [b] finding-set masks."""
    if name == "random":       # six findings, ~half set: every rank holds reports that overlap with other ranks'
        gen = torch.Generator().manual_seed(77 + b)
        bits = torch.randint(0, 2, (b, 6), generator=gen)
        return (bits << torch.arange(6)).sum(dim=1).to(torch.int64)
    if name == "zero":
        return torch.zeros(b, dtype=torch.int64)
    if name == "equal":
        return torch.full((b,), 0b1011, dtype=torch.int64)
    if name == "one_bit_per_study":  # the studies of the "dup_across" ids: equal masks on two ranks
        sid = id_pattern("dup_across", b, b_local).tolist()
        order = {v: n for n, v in enumerate(dict.fromkeys(sid))}
        return torch.tensor([1 << order[v] for v in sid], dtype=torch.int64)
    if name == "bit63":        # bit 63 is ignored: sample 0 and the last sample carry it on top of their findings
        lab = label_pattern("random", b, b_local).tolist()
        lab[0] -= 1 << 63
        lab[-1] -= 1 << 63
        return torch.tensor(lab, dtype=torch.int64)
    raise ValueError(name)


def _column_partials(sd):
    """(m, s) of every column over the rows of ``sd`` and the part's interleaved form."""
    m = sd.max(dim=0).values
    ssum = torch.exp(sd - m[None, :]).sum(dim=0)
    return torch.stack([m, ssum], dim=1).reshape(-1)


def _merge_columns(parts, b):
    m, s = parts[:, 0:2 * b:2], parts[:, 1:2 * b:2]
    mm = m.max(dim=0).values
    return mm + torch.log((s * torch.exp(m - mm[None, :])).sum(dim=0))


class OraclePosSoftOps:
    """fp64 stand-in for HipBilinearOps / HipSeparableOps in the row-block protocols of the two losses."""

    def __init__(self, critic: str):
        self.scorer = SCORERS[critic]

    def _scores(self, x, y_all, params):
        with torch.enable_grad():  # called from inside an autograd.Function.forward, where grad mode is off
            leaves = [t.detach().clone().requires_grad_(True) for t in (x, y_all, *params)]
            s = self.scorer(*leaves)
        return leaves, s

    # ------------------------------------------------------------------------------------------ study positives
    def posnce_forward(self, x, y_all, params, sid_rows, sid_all, row_offset, mode, precision, need_grad=True):
        leaves, s = self._scores(x, y_all, params)
        sd = s.detach()
        br, b = sd.shape
        assert torch.equal(sid_rows, sid_all[row_offset:row_offset + br])
        pos = (sid_rows[:, None] == sid_all[None, :]).to(sd.dtype)
        n = pos.sum(dim=1)
        r = torch.logsumexp(sd, dim=1)
        row_terms = r - (pos * sd).sum(dim=1) / n
        part = torch.cat([_column_partials(sd), (pos * sd).sum(dim=0), row_terms, n])
        assert part.numel() == 3 * b + 2 * br
        return part, r, n.to(torch.int32), (leaves, s, pos, n, r, mode, b)

    @staticmethod
    def posnce_merge(parts, b_rows, mode):
        b = parts.shape[0] * b_rows
        c = _merge_columns(parts, b)
        col_pos = parts[:, 2 * b:3 * b].sum(dim=0)
        row_terms = parts[:, 3 * b:3 * b + b_rows].reshape(-1)
        n = parts[:, 3 * b + b_rows:].reshape(-1)
        loss = row_terms.mean()
        if mode == 1:
            loss = 0.5 * loss + 0.5 * (c - col_pos / n).mean()
        return loss.reshape(1), c

    @staticmethod
    def posnce_backward(saved, lse_cols, grad_out):
        leaves, s, pos, n, r, mode, b = saved
        sd = s.detach()
        wr, wc = (1.0 / b, 0.0) if mode == 0 else (0.5 / b, 0.5 / b)
        g = wr * torch.exp(sd - r[:, None]) - (wr + wc) * pos / n[:, None]
        if mode == 1:
            g = g + wc * torch.exp(sd - lse_cols[None, :])
        grads = torch.autograd.grad(s, leaves, g * grad_out.to(sd.dtype))
        return grads[0], grads[1], list(grads[2:])

    # ------------------------------------------------------------------------------------------ soft targets
    def softnce_forward(self, x, y_all, params, lab_rows, lab_all, row_offset, mode, precision, tau, mix, need_grad=True):
        leaves, s = self._scores(x, y_all, params)
        sd = s.detach()
        br, b = sd.shape
        assert torch.equal(lab_rows, lab_all[row_offset:row_offset + br])
        k = sref.kernel(lab_all, tau)            # every rank: the kernel and the norms of ALL samples
        z = k.sum(dim=1)
        rows = slice(row_offset, row_offset + br)
        delta = torch.eye(b, dtype=sd.dtype)[rows]
        qr = (1.0 - mix) * delta + mix * k[rows] / z[rows][:, None]
        qc = (1.0 - mix) * delta + mix * k[rows] / z[None, :]
        r = torch.logsumexp(sd, dim=1)
        part = torch.cat([_column_partials(sd), (qc * sd).sum(dim=0), r - (qr * sd).sum(dim=1)])
        assert part.numel() == 3 * b + br
        return part, r, z[rows].clone(), (leaves, s, qr, qc, r, mode, b)

    @staticmethod
    def softnce_merge(parts, b_rows, mode):
        b = parts.shape[0] * b_rows
        c = _merge_columns(parts, b)
        loss = parts[:, 3 * b:].reshape(-1).mean()
        if mode == 1:
            loss = 0.5 * loss + 0.5 * (c - parts[:, 2 * b:3 * b].sum(dim=0)).mean()
        return loss.reshape(1), c

    @staticmethod
    def softnce_backward(saved, lse_cols, grad_out):
        leaves, s, qr, qc, r, mode, b = saved
        sd = s.detach()
        wr, wc = (1.0 / b, 0.0) if mode == 0 else (0.5 / b, 0.5 / b)
        g = wr * (torch.exp(sd - r[:, None]) - qr)
        if mode == 1:
            g = g + wc * (torch.exp(sd - lse_cols[None, :]) - qc)
        grads = torch.autograd.grad(s, leaves, g * grad_out.to(sd.dtype))
        return grads[0], grads[1], list(grads[2:])


def _one(fn, extra_stat, b_local, b, x, y, params, sl, codes, critic, symmetric, **kw):
    xl = x[sl].clone().requires_grad_(True)
    yl = y[sl].clone().requires_grad_(True)
    pl = [p.clone().requires_grad_(True) for p in params]
    common = dict(symmetric=symmetric, precision="f32", critic=critic, group=dist.group.WORLD, **kw)
    loss, stats = fn(xl, yl, codes[sl].contiguous(), pl, ops=OraclePosSoftOps(critic), return_stats=True, **common)
    assert tuple(loss.shape) == () and tuple(stats["lse_rows"].shape) == (b_local,)
    assert tuple(stats["lse_cols"].shape) == (b,) and tuple(stats[extra_stat].shape) == (b_local,)
    loss.backward()
    with torch.no_grad():  # forward only: the same loss, nothing to differentiate
        again = fn(x[sl].clone(), y[sl].clone(), codes[sl].contiguous(), params, ops=OraclePosSoftOps(critic), **common)
    return {"loss": loss.detach().reshape(1), "lse_rows": stats["lse_rows"], "lse_cols": stats["lse_cols"],
            extra_stat: stats[extra_stat], "dx": xl.grad, "dy": yl.grad, "dparams": [p.grad for p in pl],
            "loss_no_grad": again.reshape(1), "no_grad_requires_grad": bool(again.requires_grad)}


def run(rank, world, port, b_local, d, k, critic, estimator, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mutual_info_img_txt.distributed import global_batch_study_positive_infonce
    from mutual_info_img_txt.distributed_label_targets import global_batch_soft_target_infonce
    b = world * b_local
    sl = slice(rank * b_local, (rank + 1) * b_local)
    x, y, params = problem(critic, b, d, k, salt=b + d)
    symmetric = estimator == "infonce_symmetric"
    out = {}
    for pattern in ID_PATTERNS:
        out[f"pos/{pattern}"] = _one(global_batch_study_positive_infonce, "n_pos", b_local, b, x, y, params, sl,
                                   id_pattern(pattern, b, b_local), critic, symmetric)
    for pattern, tau, mix in LABEL_CASES:
        out[f"soft/{pattern}/{tau}/{mix}"] = _one(global_batch_soft_target_infonce, "target_norm", b_local, b, x, y, params,
                                              sl, label_pattern(pattern, b, b_local), critic, symmetric, tau=tau, mix=mix)
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()
