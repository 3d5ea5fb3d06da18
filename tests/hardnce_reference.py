"""fp64 restatement of the hard-negative InfoNCE (the definition the HIP kernels implement).

Scores S[i, j] = critic(img_i, txt_j); N_i = {j : sid_j != sid_i}; H_i = the first min(k, |N_i|) elements of N_i in the
total order "score descending, then index ascending" (-0.0 counts as +0.0); H'_j likewise over the rows of column j.
  r_i = log(exp S[i, i] + sum_{j in H_i} exp S[i, j]),   c_j = log(exp S[j, j] + sum_{i in H'_j} exp S[i, j])
  infonce_rowwise:   L = mean_i (r_i - S[i, i])
  infonce_symmetric: L = 1/2 mean_i (r_i - S[i, i]) + 1/2 mean_j (c_j - S[j, j])
The selection is a constant of the gradient:
  dL/dS[i, j] = w_r (1[j in H_i u {i}] exp(S[i, j] - r_i) - delta_ij) + w_c (1[i in H'_j u {j}] exp(S[i, j] - c_j) - delta_ij)
with (w_r, w_c) = (1/B, 0) row-wise and (1/2B, 1/2B) symmetric.  A training loss, not an MI bound.
Lists are int64 [B, k] with -1 tails.  Every function takes the lists to evaluate with (the kernel's own, in the GPU
tests: selection is top-k's business), or selects them itself.
Not a test module (no test_ prefix): imported by tests/test_hardnce_*.py."""
import torch

from oracle import mi_oracle as orc

MODES = ("infonce_rowwise", "infonce_symmetric")


def select(s: torch.Tensor, study_id, k: int):
    """(idx_rows, idx_cols): H_i and H'_j of the scores ``s`` as int64 [B, k], -1 tails."""
    s = s.double()
    neg = orc.negative_mask(study_id)

    def side(sc, ng):
        masked = torch.where(ng, sc, torch.full_like(sc, float("-inf")))
        # a stable descending sort keeps equal scores (-0.0 == +0.0 among them) in ascending index order
        order = torch.sort(masked, dim=1, descending=True, stable=True).indices[:, :k]
        idx = torch.where(torch.gather(ng, 1, order), order, torch.full_like(order, -1))
        if idx.shape[1] < k:
            idx = torch.cat([idx, torch.full((idx.shape[0], k - idx.shape[1]), -1, dtype=idx.dtype)], dim=1)
        return idx

    return side(s, neg), side(s.t(), neg.t())


def support(idx: torch.Tensor) -> torch.Tensor:
    """[B, B] bool: element (q, c) is true where c is listed for query q, or c == q."""
    b = idx.shape[0]
    m = torch.eye(b, dtype=torch.bool)
    q = torch.arange(b)[:, None].expand_as(idx)
    ok = idx >= 0
    m[q[ok], idx[ok].long()] = True
    return m


def lse_side(s: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """r [B]: log-sum-exp of each row of ``s`` over its listed columns and its diagonal."""
    masked = torch.where(support(idx), s, torch.full_like(s, float("-inf")))
    return torch.logsumexp(masked, dim=1)


def loss(s, idx_rows, idx_cols, estimator: str) -> torch.Tensor:
    d = torch.diagonal(s)
    row = (lse_side(s, idx_rows) - d).mean()
    if estimator == "infonce_rowwise":
        return row
    if estimator == "infonce_symmetric":
        return 0.5 * row + 0.5 * (lse_side(s.t(), idx_cols) - d).mean()
    raise ValueError(estimator)


def grad_scores(s, idx_rows, idx_cols, estimator: str) -> torch.Tensor:
    b = s.shape[0]
    eye = torch.eye(b, dtype=s.dtype)
    mr = support(idx_rows)
    g_row = (mr.to(s.dtype) * torch.exp(s - lse_side(s, idx_rows)[:, None]) - eye) / b
    if estimator == "infonce_rowwise":
        return g_row
    mc = support(idx_cols).t()
    g_col = (mc.to(s.dtype) * torch.exp(s - lse_side(s.t(), idx_cols)[None, :]) - eye) / b
    return 0.5 * g_row + 0.5 * g_col


def matrix_case(s: torch.Tensor, study_id, k: int, estimator: str, lists=None) -> dict:
    """loss, lse_rows, lse_cols, grad [B, B] and the lists used (``lists`` = (idx_rows, idx_cols) or None: selected here).
    In the row-wise mode idx_cols is not read."""
    s = s.double()
    ir, ic = select(s, study_id, k) if lists is None else (lists[0].cpu().long(), None if lists[1] is None else lists[1].cpu().long())
    if ic is None:
        ic = torch.full_like(ir, -1)
    return {"loss": loss(s, ir, ic, estimator), "lse_rows": lse_side(s, ir), "lse_cols": lse_side(s.t(), ic),
            "grad": grad_scores(s, ir, ic, estimator), "idx_rows": ir, "idx_cols": ic}


def bilinear_case(x, y, w, study_id, k: int, estimator: str, lists=None, rounded=False) -> dict:
    """The bilinear step S = (x W) y^T (w None: x y^T) in fp64 with closed-form gradients: G = dL/dS, dT = G y, dY = G^T T,
    dX = dT W^T, dW = x^T dT.  ``rounded``: at the rounding points of the 16-bit chain (x, y, w, T, G and dT to bf16), as
    nce_reference.bilinear_step_rounded."""
    rb = orc.round_bf16 if rounded else (lambda t: t)
    x, y = rb(x.double()), rb(y.double())
    wd = None if w is None else rb(w.double())
    t = x if wd is None else rb(x @ wd)
    s = t @ y.t()
    o = matrix_case(s, study_id, k, estimator, lists)
    g = rb(o["grad"])
    dt = rb(g @ y)
    o.update({"dy": g.t() @ t, "smax": float(s.abs().max()), "scores": s})
    if wd is None:
        o["dx"] = g @ y
    else:
        o.update({"dx": dt @ wd.t(), "dw": x.t() @ dt})
    return o
