"""fp64 restatement of the separable critic's DV / InfoNCE step, S = (X Wg)(Y Wh)^T under the reference bound
(mi_separable_fwd / _bwd / _step of csrc/mi_bilinear.hip), for one row block of a batch.

A row block (row_offset, b_rows) holds the image rows [row_offset, row_offset + b_rows) of a batch of b; every block
sees all b text rows.  With G = grad_out * dL/dS (exp(S - lse) on the negatives, -1/b on the diagonal, 0 on dropped
pairs), A = X Wg and C = Y Wh:

    dA = G[rows] C,  dC = G[rows]^T A[rows]            (dC: the block's part of the sum over all rows)
    grad_x = dA Wg^T (the block's rows),  grad_wg = X[rows]^T dA,  grad_y = dC Wh^T,  grad_wh = Y^T dC   (parts)

Rounding modes:
  "exact"      no rounding (what autograd through ``orc.separable_scores`` gives).
  "fused16"    the rounding points of ``orc.separable_step_rounded`` (the fused B x B kernels): X, Y, Wg, Wh, A, C to bf16;
               P = exp(S - lse) to bf16 before the two B x B contractions; dA, dC (scaled by grad_out) to bf16.
  "generic16"  the generic strided-operand kernels in the bf16 mode (mi_gemm.h): a GEMM rounds its operands to bf16 when it
               stages them; A, C, dA and dC are stored in fp32 (so each is rounded again by the GEMM that reads it); G,
               scaled by grad_out and including its diagonal term, is stored in bf16.
Not a test module (no test_ prefix): imported by tests/test_separable_*.py, which also share the case table below."""
import math

import torch

from oracle.mi_oracle import bound_from_matrix, negative_mask, round_bf16

MODES = ("exact", "fused16", "generic16")


def _ident(t):
    return t


def step(x, y, wg, wh, study_id, mode="exact", row_block=None, grad_out=1.0) -> dict:
    """One row block's step.  Returns
      the statistics of the whole batch: lse, pos_mean, n_neg, loss_dv, loss_infonce, scores [b, b];
      the block's loss terms: block_lse (log-sum-exp over the block's negatives), block_pos_sum, block_n_neg;
      dx [b_rows, d_img] and the block's parts dy [b, d_txt], dwg, dwh -- all of grad_out * loss."""
    if mode not in MODES:
        raise ValueError(mode)
    x, y, wg, wh = (t.detach().double() for t in (x, y, wg, wh))
    b = x.shape[0]
    r0, br = (0, b) if row_block is None else row_block
    rows = slice(r0, r0 + br)
    op = _ident if mode == "exact" else round_bf16          # what a GEMM does to an operand it loads
    st = round_bf16 if mode == "fused16" else _ident        # how A, C, dA, dC are stored
    a = st(op(x) @ op(wg))
    c = st(op(y) @ op(wh))
    s = op(a) @ op(c).t()
    neg = negative_mask(study_id)
    lse = torch.logsumexp(s[neg], dim=0)
    p = torch.where(neg, torch.exp(s - lse), torch.zeros_like(s))
    eye = torch.eye(b, dtype=s.dtype)[rows]
    ar, cr = op(a)[rows], op(c)
    if mode == "fused16":
        pr = round_bf16(p)[rows]
        da = round_bf16(grad_out * (pr @ cr - (eye @ cr) / b))
        dc = round_bf16(grad_out * (pr.t() @ ar - (eye.t() @ ar) / b))
    else:
        g = grad_out * (p[rows] - eye / b)
        if mode == "generic16":
            g = round_bf16(g)
        da, dc = g @ cr, g.t() @ ar
    sb, nb = s[rows], neg[rows]
    return {"scores": s, "lse": lse, "pos_mean": torch.diagonal(s).mean(), "n_neg": int(neg.sum()),
            "loss_dv": bound_from_matrix(s, study_id, "dv").reshape(()),
            "loss_infonce": bound_from_matrix(s, study_id, "infonce").reshape(()),
            "block_lse": torch.logsumexp(sb[nb], dim=0), "block_pos_sum": torch.diagonal(sb, r0).sum(),
            "block_n_neg": int(nb.sum()),
            "dx": op(da) @ op(wg).t(), "dwg": op(x)[rows].t() @ op(da), "dy": op(dc) @ op(wh).t(),
            "dwh": op(y).t() @ op(dc), "da": da, "dc": dc}


GRADS = ("dx", "dy", "dwg", "dwh")

# ------------------------------------------------------------------------------------------------ the shared case table
# (path, (b, d_img, d_txt, d_proj)): what plan_separable of csrc/mi_bilinear.hip is expected to answer for the shape in
# the bf16 mode (the f32 mode is generic for every shape).  tests/test_separable_cpu.py checks the claim against
# mi_separable_path; tests/test_separable_gpu.py runs the shapes.
GENERIC, FUSED, FUSED_TAIL = 0, 2, 3
FUSED_CASES = [(32, 8, 16, 128),      # one row block, one streamed tile, smallest widths
               (96, 72, 200, 128),    # widths = 8 mod 32, K of dW = 96 (no multiple of 64), partial 128-block
               (160, 64, 96, 256),    # full + partial 128-block, ragged split_plan chunks
               (224, 40, 136, 512),   # width 512, seven tiles
               (256, 72, 64, 128)]    # multiple of 128 rows, kept off the tail by d_img % 32 alone
TAIL_CASES = [(128, 32, 96, 128),     # smallest tail shape, d_img != d_txt
              (384, 96, 32, 512)]     # three 128-blocks at the widest projection
GENERIC_CASES = [(64, 64, 64, 48),    # d_proj % 64 != 0
                 (200, 24, 40, 64),   # d_proj = 64, refused by flash_width_ok; batch across 128
                 (130, 20, 12, 10),   # ragged everything, two row tiles
                 (3, 5, 7, 1),        # d_proj = 1
                 (1, 8, 8, 4)]        # one sample, no negatives
# (shape, precision name, path, rounding mode of the reference the kernels are held to)
CASES = ([(c, "bf16", FUSED, "fused16") for c in FUSED_CASES] + [(c, "bf16", FUSED_TAIL, "fused16") for c in TAIL_CASES] +
         [(c, "bf16", GENERIC, "generic16") for c in GENERIC_CASES] + [(c, "f32", GENERIC, "exact") for c in GENERIC_CASES])
# row-block partitions: (shape, precision, path of a block, mode, [(row_offset, b_rows), ...])
ROW_BLOCK_CASES = [((96, 72, 200, 128), "bf16", FUSED, "fused16", [(0, 32), (32, 32), (64, 32)]),
                   ((256, 64, 64, 256), "bf16", FUSED_TAIL, "fused16", [(0, 128), (128, 128)]),
                   ((130, 20, 12, 10), "bf16", GENERIC, "generic16", [(0, 50), (50, 50), (100, 30)]),
                   ((130, 20, 12, 10), "f32", GENERIC, "exact", [(0, 50), (50, 50), (100, 30)])]
UNALIGNED_BLOCK = ((96, 72, 200, 128), "bf16", FUSED, "fused16", (40, 32))   # rows [40, 72): offset no multiple of 32
GRAD_OUT = 0.37   # no power of two: a dropped or doubled scale shows


def case_id(case):
    (b, dx, dy, k), prec = case[0], case[1]
    return f"{b}-{dx}-{dy}-{k}-{prec}"


def ids(b, kind, offsets=()):
    """Study ids: "unique", "dup" (SURVEY.md 8d duplicates variant: sid_i = i - (i mod 2) for the first max(b / 8, 2)
    samples, as the neighbouring tests' _dup_ids) or "equal" (no negative pair at all).  ``offsets`` (with "dup"): the
    row offsets of the row blocks a test runs; for each, one more pair of samples that far apart shares an id.  In the
    block's frame such a pair sits on the main diagonal of a 32 x 32 tile that is NOT the diagonal of the pair matrix:
    equal-id tile flags computed for another offset than the block's take it for a sample paired with itself."""
    sid = list(range(b))
    if kind == "dup":
        n_dup = min(max(b // 8, 2), b)
        for n in range(n_dup):
            sid[n] = n - (n % 2)
        for k, off in enumerate(offsets):
            assert n_dup + 8 + k + off < b
            sid[n_dup + 8 + k + off] = sid[n_dup + 8 + k]
    elif kind == "equal":
        sid = [0] * b
    elif kind != "unique":
        raise ValueError(kind)
    return [str(50000000 + s) for s in sid]


def inputs(shape, seed=0):
    """Seeded inputs at the scale of the neighbouring tests (test_config1_separable_bf16): standard-normal embeddings,
    Wg ~ N(0, 1 / d_img) and Wh ~ N(0, 1 / d_txt) times 0.6."""
    b, dx, dy, k = shape
    gen = torch.Generator().manual_seed(1000 * seed + b + 7 * dx + 13 * dy + 31 * k)
    x = torch.randn(b, dx, generator=gen)
    y = torch.randn(b, dy, generator=gen)
    wg = torch.randn(dx, k, generator=gen) * (0.6 / math.sqrt(dx))
    wh = torch.randn(dy, k, generator=gen) * (0.6 / math.sqrt(dy))
    return x, y, wg, wh


def _two_hot_rows(b, d, gen):
    """[b, d] with two non-zeros (+-1) per row, the rows pairwise distinct: a seeded choice of b of the 4 * C(d, 2)
    (position pair, sign pair) combinations."""
    pairs = torch.combinations(torch.arange(d), 2)                       # [C(d, 2), 2]
    pick = torch.randperm(4 * len(pairs), generator=gen)[:b]
    assert len(pick) == b, f"{b} distinct two-hot rows do not exist at width {d}"
    pos, sign = pairs[pick // 4], pick % 4
    t = torch.zeros(b, d)
    t[torch.arange(b), pos[:, 0]] = (sign // 2) * 2.0 - 1.0
    t[torch.arange(b), pos[:, 1]] = (sign % 2) * 2.0 - 1.0
    return t


def structure_inputs(shape):
    """Inputs of the structure test, every entry from {-1, 0, 1}.  Every row of Wg has ONE non-zero, in the first half of
    the columns, every row of Wh one in the second half: S == 0 exactly, every exponential is 1.  Every row of X and Y has
    two non-zeros, so A and C hold integers in [-2, 2] (exact in bf16) and are sparse: most elements of
    dA_i = (sum_{j in neg(i)} C_j) / n_neg - C_i / b then have no diagonal term and are as small as the sum itself, so the
    rounding of dA leaves a single row of the sum visible (structure_row_swap_shows).  The rows of A and the rows of C are
    pairwise distinct (the seed is advanced until they are).  Study ids: unique but for three repeats."""
    b, dx, dy, k = shape
    h = k // 2
    for seed in range(64):
        gen = torch.Generator().manual_seed(5000 + 64 * (b + dx + dy + k) + seed)
        x, y = _two_hot_rows(b, dx, gen), _two_hot_rows(b, dy, gen)
        wg, wh = torch.zeros(dx, k), torch.zeros(dy, k)
        # features spread over the half's columns (injective where the width fits), signs seeded
        wg[torch.arange(dx), torch.randperm(max(h, dx), generator=gen)[:dx] % h] = torch.randint(0, 2, (dx,), generator=gen) * 2.0 - 1.0
        wh[torch.arange(dy), h + torch.randperm(max(h, dy), generator=gen)[:dy] % h] = torch.randint(0, 2, (dy,), generator=gen) * 2.0 - 1.0
        a, c = x @ wg, y @ wh
        if len(torch.unique(a, dim=0)) == b and len(torch.unique(c, dim=0)) == b:
            break
    else:
        raise AssertionError(f"no seed gives pairwise distinct rows of A and C at {shape}")
    sid = list(range(b))
    sid[1] = sid[0]
    sid[5] = sid[17 % b]
    sid[b - 1] = sid[b // 2]
    return x, y, wg, wh, [str(50000000 + s) for s in sid]


def structure_reference(x, y, wg, wh, study_id, grad_out):
    """The structure inputs' exact gradients in closed form (S == 0, every exponential 1, integer sums), and what a
    correct kernel may be off by, elementwise -- derived, not measured:

      dA[i, c] = grad_out * ((sum_{j in neg(i)} C[j, c]) / n_neg - C[i, c] / b),  dC likewise with A;
      the kernels form it in fp32 from an exact integer sum -- 2^-18 of either term covers it: the exponent -lse, below
      16 in size, is known to a few fp32 ulps of 16 (2^-20 each), which the exponential turns into a relative error, and
      the products and the subtraction add fp32 ulps of their own -- and round it to bf16 ONCE: half an ulp, between
      2^-9 and 2^-8 of it;
      dWg[a, c] = sum_i X[i, a] dA[i, c] sums b such terms times an integer operand; at most 32 of them are non-zero
      (asserted), each an exact fp32 product, so the fp32 accumulation is good to 32 * 2^-24 = 2^-19 of the absolute sum;
      dX = dA Wg^T is exactly 0: dA lives in the second half of the columns, where Wg is zero (dY likewise).

    Returns {"dwg": (ref, bound), "dwh": (ref, bound), "da": .., "dc": .., "n_neg": ..}."""
    x, y, wg, wh = (t.double() for t in (x, y, wg, wh))
    b = x.shape[0]
    a, c = x @ wg, y @ wh
    neg = negative_mask(study_id).double()
    n_neg = float(neg.sum())
    out = {"n_neg": int(n_neg), "a": a, "c": c}
    for name, g, other, lhs in (("dwg", neg, c, x), ("dwh", neg.t(), a, y)):
        d = grad_out * ((g @ other) / n_neg - other / b)
        d_err = half_ulp_bf16(d) + 2.0 ** -18 * grad_out * ((g @ other.abs()) / n_neg + other.abs() / b)
        assert int((lhs != 0).sum(0).max()) <= 32
        out[name] = (lhs.t() @ d, lhs.abs().t() @ d_err + 2.0 ** -19 * (lhs.abs().t() @ d.abs()))
        out["da" if name == "dwg" else "dc"] = d
    return out


def structure_row_swap_shows(x, y, wg, wh, study_id, grad_out):
    """Does the structure test see ONE wrong row in the sums?  For every j and its neighbours j' = j +- 1 (a tile-edge or
    transposed-read slip): row j' of C in place of row j in sum_{j in neg(i)} C_j moves dA_i by
    grad_out (C_j' - C_j) / n_neg for every i that pairs with j as a negative, and dWg by X^T times that.  True when for
    every such swap, on either side, at least one element of dWg (dWh) moves by more than structure_reference's bound."""
    r = structure_reference(x, y, wg, wh, study_id, grad_out)
    neg = negative_mask(study_id).double()
    for name, g, other, lhs in (("dwg", neg, r["c"], x.double()), ("dwh", neg.t(), r["a"], y.double())):
        bound = r[name][1]
        for shift in (1, -1):
            delta = grad_out / r["n_neg"] * (torch.roll(other, shift, 0) - other)            # [j][c]
            reach = lhs.t() @ g                                                               # [a][j] = sum_{i in neg(j)} X[i, a]
            for j in range(other.shape[0]):
                if not bool(((reach[:, j, None] * delta[j][None, :]).abs() > bound).any()):
                    return False
    return True


def half_ulp_bf16(t):
    """The largest error of rounding each element of t to bf16 (8 significant bits, round to nearest): 2^-9 of the top of
    its binade, between 2^-9 |t| and 2^-8 |t|.  0 for 0."""
    t = t.double().abs()
    e = torch.floor(torch.log2(torch.where(t > 0, t, torch.ones_like(t))))
    return torch.where(t > 0, torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 8.0), torch.zeros_like(t))
