"""fp64 restatement of the per-sample InfoNCE against a memory bank (the definition the HIP kernels
implement), with torch autograd on the CPU.

Batch x [B], y [B], ids sid [B]; bank bank_x [M], bank_y [M], ids bank_sid [M] (constants: they do not require grad).
S[i, j] = critic(img_i, txt_j) under the current critic; index B + m is bank entry m on either side.
  C_i = {i} u {j < B : sid_j != sid_i} u {B + m : bank_sid_m != sid_i}      r_i = log sum_{j in C_i} exp S[i, j]
  R_j = {j} u {i < B : sid_i != sid_j} u {B + m : bank_sid_m != sid_j}      c_j = log sum_{i in R_j} exp S[i, j]
  infonce_rowwise:   L = mean_i (r_i - S[i, i])                  (reads bank_y only)
  infonce_symmetric: L = 1/2 mean_i (r_i - S[i, i]) + 1/2 mean_j (c_j - S[j, j])
``rounded=True`` evaluates it at the rounding points of the kernels' bf16 mode: x, y, the parameters and the bank to bf16;
T = x W and U = bank_x W (separable: the projections) to bf16 on the way into the score product; in the backward G = dL/dS
and dT (dU, the projections' gradients) to bf16 where the kernels feed them to the next product.
Not a test module (no test_ prefix): imported by tests/test_banknce_*.py."""
import torch

from oracle import mi_oracle as orc

MODES = ("infonce_rowwise", "infonce_symmetric")


def id_codes(ids) -> torch.Tensor:
    """int64 codes, equal code <=> equal id (any hashable ids, or a tensor)."""
    if torch.is_tensor(ids):
        return ids.detach().cpu().long().reshape(-1)
    table = {}
    return torch.tensor([table.setdefault(str(v), len(table)) for v in ids], dtype=torch.int64)


def _codes_pair(sid, bank_sid):
    if torch.is_tensor(sid) and torch.is_tensor(bank_sid):
        return id_codes(sid), id_codes(bank_sid)
    both = id_codes([str(v) for v in _as_list(sid)] + [str(v) for v in _as_list(bank_sid)])
    n = len(_as_list(sid))
    return both[:n], both[n:]


def _as_list(ids):
    return ids.tolist() if torch.is_tensor(ids) else list(ids)


def loss_from_scores(s_top, s_left, sid, bank_sid, estimator: str) -> dict:
    """s_top [B, B + M] (batch images x batch and bank reports), s_left [M, B] (bank images x batch reports) or None in
    the row-wise mode -> loss, lse_rows, lse_cols (None row-wise)."""
    b = s_top.shape[0]
    ids, bids = _codes_pair(sid, bank_sid)
    all_ids = torch.cat([ids, bids])
    neg_inf = torch.full((), float("-inf"), dtype=s_top.dtype)
    cand = all_ids[None, :] != ids[:, None]                       # [B, B + M]
    cand[torch.arange(b), torch.arange(b)] = True
    r = torch.logsumexp(torch.where(cand, s_top, neg_inf), dim=1)
    d = torch.diagonal(s_top[:, :b])
    row = (r - d).mean()
    if estimator == "infonce_rowwise":
        return {"loss": row, "lse_rows": r, "lse_cols": None}
    if estimator != "infonce_symmetric":
        raise ValueError(estimator)
    col_block = torch.cat([s_top[:, :b], s_left], dim=0)         # [B + M, B]
    c = torch.logsumexp(torch.where(cand.t(), col_block, neg_inf), dim=0)
    return {"loss": 0.5 * row + 0.5 * (c - d).mean(), "lse_rows": r, "lse_cols": c}


class _RoundBoth(torch.autograd.Function):
    """bf16 rounding of a value on the way forward and of its gradient on the way back."""

    @staticmethod
    def forward(ctx, t):
        return orc.round_bf16(t)

    @staticmethod
    def backward(ctx, g):
        return orc.round_bf16(g)


class _GradRound(torch.autograd.Function):
    """The value passes; its gradient (G = dL/dS) is rounded to bf16."""

    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        return orc.round_bf16(g)


def _round_leaf(t):
    """bf16 rounding of an operand; the gradient passes unrounded (the kernels write it from fp32 accumulators)."""
    return t + (orc.round_bf16(t.detach()) - t.detach())


def case(x, y, params, sid, bank_x, bank_y, bank_sid, estimator: str, kind: str = "bilinear", rounded: bool = False,
         grad_out: float = 1.0) -> dict:
    """loss, lse_rows, lse_cols, smax and the gradients [dx, dy, dparams...] of grad_out * loss.  ``kind``: "bilinear"
    (params [w], or [] for S = x y^T) or "separable" (params [wg, wh]).  bank_x may be None in the row-wise mode."""
    sym = estimator == "infonce_symmetric"
    x = x.detach().double().clone().requires_grad_(True)
    y = y.detach().double().clone().requires_grad_(True)
    params = [p.detach().double().clone().requires_grad_(True) for p in params]
    bx = bank_x.detach().double() if (bank_x is not None and sym) else None
    by = bank_y.detach().double()
    leaf = _round_leaf if rounded else (lambda t: t)
    both = _RoundBoth.apply if rounded else (lambda t: t)
    xr, yr, pr = leaf(x), leaf(y), [leaf(p) for p in params]
    bxr, byr = (None if bx is None else leaf(bx)), leaf(by)
    if kind == "separable":
        wg, wh = pr
        t, yy = both(xr @ wg), both(yr @ wh)
        u = None if bxr is None else both(bxr @ wg)
        yb = both(byr @ wh)
    elif pr:
        t, yy, yb = both(xr @ pr[0]), yr, byr
        u = None if bxr is None else both(bxr @ pr[0])
    else:
        t, yy, yb, u = xr, yr, byr, bxr
    s_top = t @ torch.cat([yy, yb]).t()
    s_left = u @ yy.t() if sym else None
    if rounded:  # the scores themselves stay fp32 in the kernels: only G = dL/dS is rounded
        s_top = _GradRound.apply(s_top)
        s_left = None if s_left is None else _GradRound.apply(s_left)
    o = loss_from_scores(s_top, s_left, sid, bank_sid, estimator)
    grads = torch.autograd.grad(o["loss"] * grad_out, [x, y, *params], allow_unused=True)
    smax = float(s_top.detach().abs().max())
    if s_left is not None and s_left.numel():
        smax = max(smax, float(s_left.detach().abs().max()))
    return {"loss": o["loss"].detach(), "lse_rows": o["lse_rows"].detach(),
            "lse_cols": None if o["lse_cols"] is None else o["lse_cols"].detach(),
            "grads": [torch.zeros_like(v) if g is None else g for g, v in zip(grads, [x, y, *params])], "smax": smax}


def brute_force(s_top, s_left, sid, bank_sid, estimator: str) -> dict:
    """The definition as a double loop over Python floats (tests of the restatement itself)."""
    import math
    b, n = s_top.shape
    sid, bank_sid = [str(v) for v in _as_list(sid)], [str(v) for v in _as_list(bank_sid)]
    all_ids = sid + bank_sid
    r, c = [], []
    for i in range(b):
        tot = sum(math.exp(float(s_top[i, j])) for j in range(n) if j == i or all_ids[j] != sid[i])
        r.append(math.log(tot))
    row = sum(r[i] - float(s_top[i, i]) for i in range(b)) / b
    if estimator == "infonce_rowwise":
        return {"loss": row, "lse_rows": r, "lse_cols": None}
    for j in range(b):
        tot = sum(math.exp(float(s_top[i, j])) for i in range(b) if i == j or sid[i] != sid[j])
        tot += sum(math.exp(float(s_left[m, j])) for m in range(n - b) if bank_sid[m] != sid[j])
        c.append(math.log(tot))
    col = sum(c[j] - float(s_top[j, j]) for j in range(b)) / b
    return {"loss": 0.5 * row + 0.5 * col, "lse_rows": r, "lse_cols": c}
