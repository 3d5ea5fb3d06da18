"""fp64 restatement of the soft-target InfoNCE from finding-label bit masks (the definition the
HIP kernels implement).

Scores S[i, j] = critic(img_i, txt_j); lab_i an int whose low 63 bits are a multi-hot set of findings; tau > 0, mix in
[0, 1].  Nothing is masked:
  n_i   = popcount(lab_i)
  a_ij  = popcount(lab_i & lab_j) / sqrt(n_i n_j)   (0 where n_i n_j = 0);  a_ii := 1 always
  k_ij  = exp((a_ij - 1) / tau),   z_i = sum_j k_ij
  qr_ij = (1 - mix) delta_ij + mix k_ij / z_i,   qc_ij = (1 - mix) delta_ij + mix k_ij / z_j
  r_i = log sum_j exp S[i, j],   c_j = log sum_i exp S[i, j]
  t_i = r_i - sum_j qr_ij S[i, j],   t'_j = c_j - sum_i qc_ij S[i, j]
  infonce_rowwise:   L = mean_i t_i
  infonce_symmetric: L = 1/2 mean_i t_i + 1/2 mean_j t'_j
  dL/dS[i, j] = w_r (exp(S[i, j] - r_i) - qr_ij) + w_c (exp(S[i, j] - c_j) - qc_ij)
with (w_r, w_c) = (1/B, 0) row-wise and (1/2B, 1/2B) symmetric.  A training loss, not an MI bound.
Gradients come from torch autograd through the fp64 loss; ``grad_scores_closed`` is the formula above, for the CPU tests
to hold the two against each other.
Not a test module (no test_ prefix): imported by tests/test_softnce_*.py."""

import torch

from oracle import mi_oracle as orc

MODES = ("infonce_rowwise", "infonce_symmetric")
LOW63 = (1 << 63) - 1


def _ints(masks):
    return [int(v) & LOW63 for v in (masks.tolist() if torch.is_tensor(masks) else masks)]


def kernel(masks, tau: float) -> torch.Tensor:
    """[B, B] fp64: k_ij (symmetric, unit diagonal)."""
    m = torch.tensor(_ints(masks), dtype=torch.int64)
    bits = ((m[:, None] >> torch.arange(63)) & 1).double()          # [B, 63] multi-hot
    n = bits.sum(dim=1)
    common = bits @ bits.t()                                         # popcount(lab_i & lab_j), exact in fp64
    nn = n[:, None] * n[None, :]
    a = torch.where(nn > 0, common / torch.sqrt(nn.clamp_min(1.0)), torch.zeros_like(nn))
    a.fill_diagonal_(1.0)
    return torch.exp((a - 1.0) / tau)


_TARGETS = {}


def targets(masks, tau: float, mix: float):
    """(qr, qc, z): both [B, B] fp64 target matrices and the norms z [B] (kept per argument set; treat as read-only)."""
    key = (tuple(_ints(masks)), float(tau), float(mix))
    if key not in _TARGETS:
        if len(_TARGETS) > 64:
            _TARGETS.clear()
        k = kernel(masks, tau)
        z = k.sum(dim=1)
        eye = torch.eye(k.shape[0], dtype=torch.float64)
        _TARGETS[key] = ((1.0 - mix) * eye + mix * k / z[:, None], (1.0 - mix) * eye + mix * k / z[None, :], z)
    return _TARGETS[key]


def mean_target_entropy(masks, tau: float, mix: float) -> float:
    """mean_i H(qr_i): the floor of the row term's mean (cross-entropy >= entropy), and by symmetry of the column's."""
    qr, _, _ = targets(masks, tau, mix)
    return float(-(torch.where(qr > 0, qr * torch.log(qr.clamp_min(1e-300)), torch.zeros_like(qr))).sum(dim=1).mean())


def lse_rows_cols(s: torch.Tensor):
    return torch.logsumexp(s, dim=1), torch.logsumexp(s, dim=0)


def loss(s: torch.Tensor, masks, estimator: str, tau: float, mix: float) -> torch.Tensor:
    qr, qc, _ = targets(masks, tau, mix)
    r, c = lse_rows_cols(s)
    row = (r - (qr.to(s.dtype) * s).sum(dim=1)).mean()
    if estimator == "infonce_rowwise":
        return row
    if estimator == "infonce_symmetric":
        return 0.5 * row + 0.5 * (c - (qc.to(s.dtype) * s).sum(dim=0)).mean()
    raise ValueError(estimator)


def grad_scores(s: torch.Tensor, masks, estimator: str, tau: float, mix: float) -> torch.Tensor:
    """dL/dS by autograd through ``loss``."""
    sl = s.detach().clone().requires_grad_(True)
    loss(sl, masks, estimator, tau, mix).backward()
    return sl.grad


def grad_scores_closed(s: torch.Tensor, masks, estimator: str, tau: float, mix: float) -> torch.Tensor:
    b = s.shape[0]
    qr, qc, _ = targets(masks, tau, mix)
    r, c = lse_rows_cols(s)
    wr, wc = (1.0 / b, 0.0) if estimator == "infonce_rowwise" else (0.5 / b, 0.5 / b)
    return wr * (torch.exp(s - r[:, None]) - qr) + wc * (torch.exp(s - c[None, :]) - qc)


def matrix_case(s: torch.Tensor, masks, estimator: str, tau: float, mix: float) -> dict:
    s = s.detach().double()
    r, c = lse_rows_cols(s)
    return {"loss": loss(s, masks, estimator, tau, mix), "lse_rows": r, "lse_cols": c,
            "target_norm": targets(masks, tau, mix)[2], "grad": grad_scores(s, masks, estimator, tau, mix)}


def bilinear_case(x, y, w, masks, estimator: str, tau: float, mix: float, rounded=False) -> dict:
    """The bilinear step S = (x W) y^T (w None: x y^T): G = dL/dS by autograd, then dT = G y, dY = G^T T, dX = dT W^T,
    dW = x^T dT.  ``rounded``: at the rounding points of the 16-bit chain -- x, y, W, T, G and dT to bf16."""
    rb = orc.round_bf16 if rounded else (lambda t: t)
    x, y = rb(x.double()), rb(y.double())
    wd = None if w is None else rb(w.double())
    t = x if wd is None else rb(x @ wd)
    s = t @ y.t()
    o = matrix_case(s, masks, estimator, tau, mix)
    g = rb(o["grad"])
    o.update({"dy": g.t() @ t, "smax": float(s.abs().max()), "scores": s})
    if wd is None:
        o["dx"] = g @ y
    else:
        dt = rb(g @ y)
        o.update({"dx": dt @ wd.t(), "dw": x.t() @ dt})
    return o


def separable_case(x, y, wg, wh, masks, estimator: str, tau: float, mix: float, rounded=False) -> dict:
    """The separable step: the w None form on the projections A = x Wg, C = y Wh, then the back-projection (as
    posnce_reference.separable_case)."""
    rb = orc.round_bf16 if rounded else (lambda t: t)
    x, y, wg, wh = x.double(), y.double(), wg.double(), wh.double()
    a, c = rb(rb(x) @ rb(wg)), rb(rb(y) @ rb(wh))
    s = a @ c.t()
    o = matrix_case(s, masks, estimator, tau, mix)
    g = rb(o["grad"])
    da, dc = rb(g @ c), rb(g.t() @ a)
    o.update({"dx": da @ rb(wg).t(), "dwg": rb(x).t() @ da, "dy": dc @ rb(wh).t(), "dwh": rb(y).t() @ dc,
              "smax": float(s.abs().max()), "scores": s})
    return o


def step(scores_fn, leaves, masks, estimator: str, tau: float, mix: float) -> dict:
    """fp64 autograd through a score function: loss, lse_rows, lse_cols and the gradients of ``leaves``."""
    leaves = [t.detach().double().clone().requires_grad_(True) for t in leaves]
    s = scores_fn(*leaves)
    l = loss(s, masks, estimator, tau, mix)
    l.backward()
    r, c = lse_rows_cols(s.detach())
    return {"loss": l.detach(), "lse_rows": r, "lse_cols": c, "grads": [t.grad for t in leaves]}
