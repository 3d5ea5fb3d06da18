"""fp64 restatement of the study-positive InfoNCE (the definition the HIP kernels implement).

Scores S[i, j] = critic(img_i, txt_j); P_i = {j : sid_j == sid_i} (contains i), n_i = |P_i|.  Nothing is masked:
  r_i = log sum_j exp S[i, j],   c_j = log sum_i exp S[i, j]
  t_i = r_i - (1/n_i) sum_{p in P_i} S[i, p],   t'_j = c_j - (1/n_j) sum_{p in P_j} S[p, j]
  infonce_rowwise:   L = mean_i t_i
  infonce_symmetric: L = 1/2 mean_i t_i + 1/2 mean_j t'_j
  dL/dS[i, j] = w_r exp(S[i, j] - r_i) + w_c exp(S[i, j] - c_j) - (w_r + w_c) 1[sid_i == sid_j] / n_i
with (w_r, w_c) = (1/B, 0) row-wise and (1/2B, 1/2B) symmetric.  A training loss, not an MI bound.
Gradients come from torch autograd through the fp64 loss; ``grad_scores_closed`` is the formula above, for the CPU tests
to hold the two against each other.
Not a test module (no test_ prefix): imported by tests/test_posnce_*.py."""
import torch

from oracle import mi_oracle as orc

MODES = ("infonce_rowwise", "infonce_symmetric")


def positives(study_id) -> torch.Tensor:
    """[B, B] bool: sid_i == sid_j."""
    ids = [int(v) if torch.is_tensor(v) else v for v in study_id]
    codes = {}
    c = torch.tensor([codes.setdefault(v, len(codes)) for v in ids])
    return c[:, None] == c[None, :]


def lse_rows_cols(s: torch.Tensor):
    return torch.logsumexp(s, dim=1), torch.logsumexp(s, dim=0)


def loss(s: torch.Tensor, study_id, estimator: str) -> torch.Tensor:
    p = positives(study_id).to(s.dtype)
    n = p.sum(dim=1)
    r, c = lse_rows_cols(s)
    row = (r - (p * s).sum(dim=1) / n).mean()
    if estimator == "infonce_rowwise":
        return row
    if estimator == "infonce_symmetric":
        return 0.5 * row + 0.5 * (c - (p * s).sum(dim=0) / n).mean()
    raise ValueError(estimator)


def grad_scores(s: torch.Tensor, study_id, estimator: str) -> torch.Tensor:
    """dL/dS by autograd through ``loss``."""
    sl = s.detach().clone().requires_grad_(True)
    loss(sl, study_id, estimator).backward()
    return sl.grad


def grad_scores_closed(s: torch.Tensor, study_id, estimator: str) -> torch.Tensor:
    b = s.shape[0]
    p = positives(study_id).to(s.dtype)
    n = p.sum(dim=1)
    r, c = lse_rows_cols(s)
    wr, wc = (1.0 / b, 0.0) if estimator == "infonce_rowwise" else (0.5 / b, 0.5 / b)
    return wr * torch.exp(s - r[:, None]) + wc * torch.exp(s - c[None, :]) - (wr + wc) * p / n[:, None]


def matrix_case(s: torch.Tensor, study_id, estimator: str) -> dict:
    s = s.detach().double()
    r, c = lse_rows_cols(s)
    return {"loss": loss(s, study_id, estimator), "lse_rows": r, "lse_cols": c,
            "n_pos": positives(study_id).sum(dim=1).to(torch.int32), "grad": grad_scores(s, study_id, estimator)}


def bilinear_case(x, y, w, study_id, estimator: str, rounded=False) -> dict:
    """The bilinear step S = (x W) y^T (w None: x y^T): G = dL/dS by autograd, then dT = G y, dY = G^T T, dX = dT W^T,
    dW = x^T dT.  ``rounded``: at the rounding points of the 16-bit chain -- x, y, W, T, G and dT to bf16."""
    rb = orc.round_bf16 if rounded else (lambda t: t)
    x, y = rb(x.double()), rb(y.double())
    wd = None if w is None else rb(w.double())
    t = x if wd is None else rb(x @ wd)
    s = t @ y.t()
    o = matrix_case(s, study_id, estimator)
    g = rb(o["grad"])
    o.update({"dy": g.t() @ t, "smax": float(s.abs().max()), "scores": s})
    if wd is None:
        o["dx"] = g @ y
    else:
        dt = rb(g @ y)
        o.update({"dx": dt @ wd.t(), "dw": x.t() @ dt})
    return o


def separable_case(x, y, wg, wh, study_id, estimator: str, rounded=False) -> dict:
    """The separable step: the w None form on the projections A = x Wg, C = y Wh, then the back-projection (as
    test_nce_gpu._separable_oracle)."""
    rb = orc.round_bf16 if rounded else (lambda t: t)
    x, y, wg, wh = x.double(), y.double(), wg.double(), wh.double()
    a, c = rb(rb(x) @ rb(wg)), rb(rb(y) @ rb(wh))
    s = a @ c.t()
    o = matrix_case(s, study_id, estimator)
    g = rb(o["grad"])
    da, dc = rb(g @ c), rb(g.t() @ a)
    o.update({"dx": da @ rb(wg).t(), "dwg": rb(x).t() @ da, "dy": dc @ rb(wh).t(), "dwh": rb(y).t() @ dc,
              "smax": float(s.abs().max()), "scores": s})
    return o


def step(scores_fn, leaves, study_id, estimator: str) -> dict:
    """fp64 autograd through a score function: loss, lse_rows, lse_cols and the gradients of ``leaves``."""
    leaves = [t.detach().double().clone().requires_grad_(True) for t in leaves]
    s = scores_fn(*leaves)
    l = loss(s, study_id, estimator)
    l.backward()
    r, c = lse_rows_cols(s.detach())
    return {"loss": l.detach(), "lse_rows": r, "lse_cols": c, "grads": [t.grad for t in leaves]}
