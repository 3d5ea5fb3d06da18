"""fp64 restatement of the MI estimates, written from the definitions alone: plain torch on the
host, dense masks, torch.logsumexp.  Every value is an ESTIMATE (higher means more MI, in nats), not a loss.

    S[i, j] = critic(img_i, txt_j) over b pairs; positives (i, i), n_pos = b; negatives i != j with sid_i != sid_j, n_neg of
    them; equal-id off-diagonal pairs dropped.  sp(x) = log(1 + e^x).
    dv        mean_pos s - (LSE_neg s - log n_neg)
    nwj       mean_pos s - exp(LSE_neg s - log n_neg - 1)
    jsd       -(mean_pos sp(-s) + mean_neg sp(s))
    nce_i2t   (1/b) sum_i (S_ii - r_i + log |C_i|),  r_i = LSE_{j in C_i} S_ij,  C_i = {i} u {j : sid_j != sid_i}
    nce_t2i   (1/b) sum_j (S_jj - c_j + log |R_j|),  c_j = LSE_{i in R_j} S_ij,  R_j = {j} u {i : sid_i != sid_j}
    pos_mean, neg_mean, log_n_neg
    smile[k]  mean_pos s - (log sum_neg exp(clip(s, -tau_k, tau_k)) - log n_neg)
Without negatives dv, nwj, jsd, neg_mean and smile are NaN, log_n_neg is -inf and nce_* is exactly 0."""
import math

import torch

def softplus(x):
    """log(1 + e^x) without torch's linear shortcut above 20."""
    return torch.logaddexp(torch.zeros_like(x), x)


NAMES = ("dv", "nwj", "jsd", "nce_i2t", "nce_t2i", "pos_mean", "neg_mean", "log_n_neg")


def masks(sid):
    """(positive mask, negative mask), bool [b, b]."""
    sid = torch.as_tensor(sid).reshape(-1)
    b = sid.numel()
    pos = torch.eye(b, dtype=torch.bool)
    neg = (sid[:, None] != sid[None, :]) & ~pos
    return pos, neg


def estimates(scores, sid, taus=()):
    """dict name -> Python float (``smile``: a list, one per tau) of the fp64 estimates of ``scores`` [b, b]."""
    s = torch.as_tensor(scores).double()
    b = s.shape[0]
    pos, neg = masks(sid)
    n_neg = int(neg.sum())
    nan = float("nan")
    d = torch.diagonal(s)
    out = {"pos_mean": float(d.mean())}
    cand = neg | pos
    r = torch.logsumexp(s.masked_fill(~cand, -math.inf), dim=1)
    c = torch.logsumexp(s.masked_fill(~cand, -math.inf), dim=0)
    n_cand = cand.sum(1).double()  # |C_i| == |R_i|: the mask is symmetric
    assert torch.equal(cand.sum(0), cand.sum(1))
    out["nce_i2t"] = float((d - r + n_cand.log()).mean())
    out["nce_t2i"] = float((d - c + n_cand.log()).mean())
    if n_neg == 0:
        out.update(dv=nan, nwj=nan, jsd=nan, neg_mean=nan, log_n_neg=-math.inf, smile=[nan for _ in taus])
        return out
    sn = s[neg]
    log_n = math.log(n_neg)
    lse = float(torch.logsumexp(sn, 0))
    out["log_n_neg"] = log_n
    out["neg_mean"] = float(sn.mean())
    out["dv"] = out["pos_mean"] - (lse - log_n)
    out["nwj"] = out["pos_mean"] - math.exp(lse - log_n - 1.0)
    out["jsd"] = -(float(softplus(-d).mean()) + float(softplus(sn).mean()))
    out["smile"] = [out["pos_mean"] - (float(torch.logsumexp(sn.clamp(-float(t), float(t)), 0)) - log_n) for t in taus]
    return out
