"""fp64 restatement of the per-sample InfoNCE (the definition the HIP kernels implement).

Scores S[i, j] = critic(img_i, txt_j); a pair i != j with equal study ids is dropped (main_utils.py:105).
  C_i = {i} u {j : sid_j != sid_i},  r_i = log sum_{j in C_i} exp S[i, j]
  R_j = {j} u {i : sid_i != sid_j},  c_j = log sum_{i in R_j} exp S[i, j]
  infonce_rowwise:   L = mean_i (r_i - S[i, i])
  infonce_symmetric: L = 1/2 mean_i (r_i - S[i, i]) + 1/2 mean_j (c_j - S[j, j])
Not a test module (no test_ prefix): imported by tests/test_nce_*.py."""
import torch

from oracle import mi_oracle as orc

MODES = ("infonce_rowwise", "infonce_symmetric")


def candidates(study_id) -> torch.Tensor:
    """[B, B] bool: j in C_i (equivalently i in R_j)."""
    neg = orc.negative_mask(study_id)
    return neg | torch.eye(neg.shape[0], dtype=torch.bool)


def lse_rows_cols(s: torch.Tensor, study_id):
    m = candidates(study_id)
    masked = torch.where(m, s, torch.full_like(s, float("-inf")))
    return torch.logsumexp(masked, dim=1), torch.logsumexp(masked, dim=0)


def nce_loss(s: torch.Tensor, study_id, estimator: str) -> torch.Tensor:
    r, c = lse_rows_cols(s, study_id)
    d = torch.diagonal(s)
    row = (r - d).mean()
    if estimator == "infonce_rowwise":
        return row
    if estimator == "infonce_symmetric":
        return 0.5 * row + 0.5 * (c - d).mean()
    raise ValueError(estimator)


def nce_grad_scores(s: torch.Tensor, study_id, estimator: str) -> torch.Tensor:
    """Closed form of dL/dS: (1/B)(1[j in C_i] exp(S - r_i) - delta_ij) for the row term, likewise with c_j."""
    b = s.shape[0]
    m = candidates(study_id).to(s.dtype)
    r, c = lse_rows_cols(s, study_id)
    eye = torch.eye(b, dtype=s.dtype)
    g_row = (m * torch.exp(s - r[:, None]) - eye) / b
    if estimator == "infonce_rowwise":
        return g_row
    g_col = (m * torch.exp(s - c[None, :]) - eye) / b
    return 0.5 * g_row + 0.5 * g_col


def matrix_case(s: torch.Tensor, study_id, estimator: str) -> dict:
    s = s.double()
    r, c = lse_rows_cols(s, study_id)
    return {"loss": nce_loss(s, study_id, estimator), "lse_rows": r, "lse_cols": c,
            "grad": nce_grad_scores(s, study_id, estimator)}


def step(scores_fn, leaves, study_id, estimator: str) -> dict:
    """fp64 autograd through a score function: loss, lse_rows, lse_cols and the gradients of ``leaves``."""
    leaves = [t.detach().double().clone().requires_grad_(True) for t in leaves]
    s = scores_fn(*leaves)
    loss = nce_loss(s, study_id, estimator)
    loss.backward()
    r, c = lse_rows_cols(s.detach(), study_id)
    return {"loss": loss.detach(), "lse_rows": r, "lse_cols": c, "grads": [t.grad for t in leaves]}


def bilinear_step_rounded(x, y, w, study_id, estimator: str) -> dict:
    """The bilinear step at the rounding points of the 16-bit GEMM chain: x, y, w and T = x W rounded to bf16; G = dL/dS
    rounded to bf16 before dT = G y and dY = G^T T; dT rounded to bf16 before dX = dT W^T and dW = x^T dT."""
    rb = orc.round_bf16
    xb, yb, wb = rb(x.double()), rb(y.double()), rb(w.double())
    tb = rb(xb @ wb)
    s = tb @ yb.t()
    r, c = lse_rows_cols(s, study_id)
    g = rb(nce_grad_scores(s, study_id, estimator))
    dt = rb(g @ yb)
    return {"loss": nce_loss(s, study_id, estimator), "lse_rows": r, "lse_cols": c, "dx": dt @ wb.t(),
            "dy": g.t() @ tb, "dw": xb.t() @ dt}
