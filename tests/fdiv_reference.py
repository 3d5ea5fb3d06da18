"""fp64 restatement of the Jensen-Shannon and NWJ bounds in torch, gradients by autograd.

Pairs are the reference's (main_utils.py:88-110): positives (i, i), negatives i != j with different study ids, other pairs
dropped.  sp(x) = log(1 + e^x).
  "jsd": L = mean_pos sp(-s) + mean_neg sp(s)
  "nwj": L = exp(LSE_neg - log n_neg - 1) - mean_pos s
"""
import torch

from oracle import mi_oracle as orc

MODES = ("jsd", "nwj")


def terms(pos, neg, mode):
    """(positive-pair term, negative-pair term) of fp64 score vectors."""
    pos, neg = pos.double(), neg.double()
    if mode == "dv":  # the reference's DV, as a yardstick for the 16-bit modes' errors
        n = torch.tensor(float(neg.numel()), dtype=torch.float64, device=neg.device)
        return -pos.mean(), torch.logsumexp(neg, 0) - torch.log(n)
    if mode == "jsd":
        return torch.nn.functional.softplus(-pos).mean(), torch.nn.functional.softplus(neg).mean()
    n = torch.tensor(float(neg.numel()), dtype=torch.float64, device=neg.device)
    return -pos.mean(), torch.exp(torch.logsumexp(neg, 0) - torch.log(n) - 1.0)


def logits_case(logits, pos_size, mode):
    """loss, terms and d loss / d logits on the reference's logits layout (first pos_size rows positive)."""
    s = logits.detach().double().reshape(-1).clone().requires_grad_(True)
    tp, tn = terms(s[:pos_size], s[pos_size:], mode)
    loss = tp + tn
    loss.backward()
    return {"loss": loss.detach(), "terms": (tp.detach(), tn.detach()), "grad": s.grad.reshape(logits.shape)}


def masks(sid_rows, sid_cols, row_offset=0, device=None):
    """(positive, negative) boolean [b_rows, b] masks of a row block."""
    codes = {}
    r = torch.tensor([codes.setdefault(str(v), len(codes)) for v in sid_rows], device=device)
    c = torch.tensor([codes.setdefault(str(v), len(codes)) for v in sid_cols], device=device)
    gi = torch.arange(len(sid_rows), device=device)[:, None] + row_offset
    gj = torch.arange(len(sid_cols), device=device)[None, :]
    pos = gi == gj
    neg = (~pos) & (r[:, None] != c[None, :])
    return pos, neg


def matrix_loss(s, sid, mode, sid_cols=None, row_offset=0):
    """Differentiable fp64 loss of a (row block of a) score matrix; n_pos is the number of columns."""
    pos, neg = masks(sid, sid if sid_cols is None else sid_cols, row_offset, s.device)
    tp, tn = terms(s[pos], s[neg], mode)
    return tp + tn, (tp, tn)


def matrix_case(scores, sid, mode):
    s = scores.detach().double().clone().requires_grad_(True)
    loss, (tp, tn) = matrix_loss(s, sid, mode)
    loss.backward()
    return {"loss": loss.detach(), "terms": (tp.detach(), tn.detach()), "grad": s.grad}


def closed_form_grad(scores, sid, mode):
    """d loss / d S from the table of DESIGN.md section 9 (no autograd)."""
    s = scores.double()
    pos, neg = masks(sid, sid, 0, s.device)
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    g = torch.zeros_like(s)
    if mode == "jsd":
        g[pos] = -torch.sigmoid(-s[pos]) / n_pos
        g[neg] = torch.sigmoid(s[neg]) / n_neg
    else:
        g[pos] = -1.0 / n_pos
        g[neg] = torch.exp(s[neg] - 1.0 - torch.log(torch.tensor(float(n_neg), dtype=torch.float64, device=s.device)))
    return g


def concat_case(x, y, params, sid, mode, block=128):
    """Concat-MLP critic: loss, terms and the gradients of every input and parameter.  The loss comes from the fp64 score
    matrix; gradients by the row-blocked pattern (s_block * g).sum().backward() with g = dL/dS of the whole batch.  Runs on
    the device of the inputs (fp64)."""
    x, y = x.double(), y.double()
    p = [q.detach().double() for q in params]
    with torch.no_grad():
        s = torch.cat([orc.concat_scores_matrix(x[i:i + block], y, p) for i in range(0, x.shape[0], block)])
    o = matrix_case(s, sid, mode)
    g = o["grad"]
    xl, yl = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    pl = [q.clone().requires_grad_(True) for q in p]
    for i0 in range(0, x.shape[0], block):
        sb = orc.concat_scores_matrix(xl[i0:i0 + block], yl, pl)
        (sb * g[i0:i0 + block]).sum().backward()
    o.update({"dx": xl.grad, "dy": yl.grad, "dparams": [q.grad for q in pl], "scores": s})
    return o
