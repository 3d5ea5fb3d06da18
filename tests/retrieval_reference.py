"""fp64 restatement of the retrieval ranks for the tests: plain torch on a [B, B] score matrix.

With S[i, j] = critic(img_i, txt_j), positives (i, i), and a pair i != j with equal study ids dropped:
    rank_i2t[i] = #{ j : sid_j != sid_i and S[i, j] > S[i, i] }
    rank_t2i[j] = #{ i : sid_i != sid_j and S[i, j] > S[j, j] }
0-based, strictly greater (a tie counts for the true pair)."""
import torch


def _negatives(study_id, b):
    """[B, B] bool: (i, j) is a negative pair.  Equal ids are dropped, the diagonal with them."""
    if torch.is_tensor(study_id):
        codes = study_id.detach().cpu().to(torch.int64)
    else:
        seen = {}
        codes = torch.tensor([seen.setdefault(str(s), len(seen)) for s in study_id], dtype=torch.int64)
    assert codes.numel() == b
    return codes[:, None] != codes[None, :]


def ranks(scores, study_id):
    """(rank_i2t, rank_t2i), int64 [B] each.  The comparison runs on the values as given (cast to fp64 exactly)."""
    s = scores.detach().cpu().double()
    b = s.shape[0]
    neg = _negatives(study_id, b)
    d = torch.diagonal(s)
    return (((s > d[:, None]) & neg).sum(1), ((s > d[None, :]) & neg).sum(0))


def rank_band(scores, study_id, tau):
    """(lo, hi), each a pair (i2t, t2i) of int64 [B]: the ranks that scores within ``tau`` of ``scores`` (elementwise)
    can give.  lo_i = #{neg j : S_ij > S_ii + 2 tau} -- such a pair stays above the diagonal whatever the error -- and
    hi_i = #{neg j : S_ij > S_ii - 2 tau}; the column form likewise against S_jj."""
    s = scores.detach().cpu().double()
    b = s.shape[0]
    neg = _negatives(study_id, b)
    d = torch.diagonal(s)
    lo = (((s > d[:, None] + 2 * tau) & neg).sum(1), ((s > d[None, :] + 2 * tau) & neg).sum(0))
    hi = (((s > d[:, None] - 2 * tau) & neg).sum(1), ((s > d[None, :] - 2 * tau) & neg).sum(0))
    return lo, hi
