"""fp64 restatement of the top-k retrieval over a gallery, for the tests.

Queries q and candidates g with scores ``S[q, g]``; a candidate is excluded for a query when ids are given and
``id_q == id_g``.  The result of a query is the first k candidates in the total order: score descending, then candidate
index ascending; -0.0 counts as +0.0 (they compare equal here).  ``idx`` is int64 [n_q, k], ``val`` float64 [n_q, k] =
``S[q, idx]``; where fewer than k candidates remain the tail is idx = -1, val = -inf.  Plain torch on the host."""
import torch


def topk(scores, k, q_ids=None, g_ids=None):
    """(idx, val) of ``scores`` [n_q, n_g]: each ROW's first k columns in the total order."""
    s = torch.as_tensor(scores).detach().cpu().to(torch.float64)
    n_q, n_g = s.shape
    if (q_ids is None) != (g_ids is None):
        raise ValueError("pass both id lists or neither")
    if q_ids is None:
        excl = torch.zeros(n_q, n_g, dtype=torch.bool)
    else:
        excl = torch.as_tensor(q_ids).reshape(-1, 1) == torch.as_tensor(g_ids).reshape(1, -1)
    # two stable sorts: by score descending (equal scores keep the index order), then the excluded ones to the back
    order = torch.sort(s, dim=1, descending=True, stable=True).indices
    back = torch.sort(excl.gather(1, order).to(torch.int8), dim=1, stable=True).indices
    order = order.gather(1, back)
    n_left = (~excl).sum(dim=1, keepdim=True)
    idx = torch.full((n_q, k), -1, dtype=torch.int64)
    val = torch.full((n_q, k), float("-inf"), dtype=torch.float64)
    m = min(k, n_g)
    keep = torch.arange(m).reshape(1, -1) < n_left
    idx[:, :m] = torch.where(keep, order[:, :m], idx[:, :m])
    val[:, :m] = torch.where(keep, s.gather(1, order[:, :m]), val[:, :m])
    return idx, val


def both_directions(scores, k, img_ids=None, txt_ids=None):
    """{"i2t": (idx, val), "t2i": (idx, val)} of ``scores`` [n_img, n_txt]."""
    s = torch.as_tensor(scores)
    return {"i2t": topk(s, k, img_ids, txt_ids), "t2i": topk(s.t(), k, txt_ids, img_ids)}
