"""The shapes at which the loss families' score GEMM reaches each kernel of the 16-bit launcher, and the data placed on
those kernels' seams (tests/test_gemm_variants_gpu.py runs them; tests/test_abi.py pins the table without a GPU).

Every family's B x B sweep on the 16-bit chain is one launch_gemm_bf16 call on an m x n x K problem, K = d_txt (bf16) or
3 d_txt (bf16x3), and the launcher picks one of six kernels from (m, n, K) alone (mi_gemm16_variant reports which).  Each
row below is the smallest batch that reaches its kernel and still has a ragged last tile; every size is a multiple of 8,
as the 16-bit chain requires.

Rectangular forms.  The memory bank's top block is b x (b + M) (its left block M x b is small) and the top-k gallery is
n_img x n_txt one way and n_txt x n_img the other.  Chosen here: M = EXTRA = 80 bank entries and n_txt = b + 80 gallery
reports on EVERY row -- one draw of b + 80 reports serves the batch, the bank and the gallery, and at each row b x (b + 80)
and (b + 80) x b resolve to the row's kernel (asserted by ``check_table``).  For the 256 x 256-tile kernel that is
3336 x 3416 (14 x 14 tiles either way), 2 % more elements than the smallest possible 3336 x 3344.

Not a test module (no test_ prefix)."""
import functools
import math
from typing import NamedTuple

import torch

EXTRA = 80
D_IMG = 64


class Row(NamedTuple):
    name: str        # test id
    variant: str     # MI_GEMM16_<variant> of _hip
    b: int
    d_txt: int
    precision: str   # "bf16" or "bf16x3"
    control: bool = False

    @property
    def k(self):
        return self.d_txt * (3 if self.precision == "bf16x3" else 1)


ROWS = (
    Row("plain", "PLAIN", 136, 40, "bf16"),
    Row("glds", "GLDS", 136, 64, "bf16", control=True),         # what the family files already run
    Row("glds-large-grid", "GLDS", 3000, 256, "bf16"),          # 24 x 24 = 576 tiles > 512: not the four-stage kernel
    Row("glds4", "GLDS4", 136, 256, "bf16"),
    Row("pipe128", "PIPE128", 136, 704, "bf16x3"),              # K = 2112
    Row("pipe256x128", "PIPE256X128", 2312, 704, "bf16x3"),     # 10 x 19 = 190 tiles; 2312 = 9 * 256 + 8
    Row("big", "BIG", 3336, 64, "bf16"),                        # 14 x 14 = 196 tiles; 3336 = 13 * 256 + 8
)
ALSO = (("PIPE128", 136, 136, 2048),)                           # the bf16 form of the pipe128 row
NEW_ROWS = tuple(r for r in ROWS if not r.control)
VARIANTS = ("PLAIN", "GLDS", "GLDS4", "PIPE128", "PIPE256X128", "BIG")


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def variant_code(row_or_name):
    from mutual_info_img_txt import _hip
    return getattr(_hip, "MI_GEMM16_" + (row_or_name.variant if isinstance(row_or_name, Row) else row_or_name))


def problems(row):
    """(m, n, K) of the score GEMMs a row runs: square, the bank's top block / the gallery, and the gallery transposed."""
    return ((row.b, row.b, row.k), (row.b, row.b + EXTRA, row.k), (row.b + EXTRA, row.b, row.k))


def check_row(row):
    """Every score GEMM of the row resolves to the row's kernel (host arithmetic only: needs no GPU)."""
    from mutual_info_img_txt import _hip
    lib = _hip.load()
    assert row.b % 8 == 0 and row.d_txt % 8 == 0 and D_IMG % 8 == 0
    for m, n, k in problems(row):
        got = lib.mi_gemm16_variant(m, n, k)
        assert got == variant_code(row), (row.name, (m, n, k), got, variant_code(row))


def check_table():
    from mutual_info_img_txt import _hip
    lib = _hip.load()
    for row in ROWS:
        check_row(row)
    for variant, m, n, k in ALSO:
        assert lib.mi_gemm16_variant(m, n, k) == variant_code(variant), (variant, m, n, k)
    assert {r.variant for r in ROWS} == set(VARIANTS)            # all six kernels are reached
    assert sorted(variant_code(v) for v in VARIANTS) == list(range(6))
    for row in ROWS:                                             # ragged last tiles: of 128, and of 256 on the large rows
        assert row.b % 128 != 0 and (row.b + EXTRA) % 128 != 0
        assert row.variant not in ("PIPE256X128", "BIG") or row.b % 256 == 8


# ------------------------------------------------------------------------------------------------ ids on the seams
def seam_ids(b):
    """int64 [b], unique but for: a pair inside one 64-tile (2, 3); a pair across the two far corners (0, b - 1); a group
    of five straddling a 256-row boundary (254 .. 258; 126 .. 130, across the 128-row one, where b < 259); and on the
    large rows a pair (300, b - 3) with one member in the last, 8-row tile row / column."""
    sid = torch.arange(b, dtype=torch.int64)
    sid[3] = sid[2]
    sid[b - 1] = sid[0]
    lo = 254 if b >= 259 else 126
    sid[lo:lo + 5] = sid[lo]
    if b > 400:
        sid[b - 3] = sid[300]
    return sid


def extra_ids(b):
    """int64 [EXTRA] ids of the bank entries / the gallery's extra reports: every third shares an id with the batch, the
    last one with sample b - 1 (the far corner of the top block)."""
    sid = seam_ids(b)
    out = torch.arange(EXTRA, dtype=torch.int64) + 10 ** 6
    out[::3] = sid[(7 * torch.arange(0, EXTRA, 3)) % b]
    out[EXTRA - 1] = sid[b - 1]
    return out


def strings(ids):
    return [str(50000000 + int(v)) for v in ids]


def seam_masks(b, base):
    """Label masks ``base`` [b] with the members of each id group of ``seam_ids`` given the first member's mask."""
    sid = seam_ids(b)
    return base[sid].clone()


# ------------------------------------------------------------------------------------------------ exact data
@functools.lru_cache(maxsize=None)
def exact_case(name):
    """Operands from {-1, 0, 1}, X scaled by the power of two that brings |S|max to at most 16 (as
    test_mi_estimates_gpu._int_case): x [b, 64], y_all [b + EXTRA, d_txt] (the batch's reports, then the bank / the extra
    gallery reports), bank_x [EXTRA, 64], w [64, d_txt] and the fp64 scores s_all [b + EXTRA, b + EXTRA] of (x; bank_x)
    against y_all.  T and S are integers times that power of two, so they are exact in bf16 and in bf16x3 -- asserted
    here, on the host.  Shared by every family; treat as read-only."""
    row = by_name(name)
    gen = torch.Generator().manual_seed(row.b * 7 + row.d_txt)

    def draw(r, c):
        return torch.randint(-1, 2, (r, c), generator=gen).float()

    x_all, y_all, w = draw(row.b + EXTRA, D_IMG), draw(row.b + EXTRA, row.d_txt), draw(D_IMG, row.d_txt)
    rb = lambda t: t.bfloat16().double()

    def scores(xa, rnd=lambda t: t):
        return rnd(rnd(xa.double()) @ rnd(w.double())) @ rnd(y_all.double()).t()

    s_int = scores(x_all)
    assert float((x_all.double() @ w.double()).abs().max()) <= 256.0 and float(s_int.abs().max()) < 2.0 ** 24
    scale = 2.0 ** -max(0, math.ceil(math.log2(float(s_int.abs().max()) / 16.0)))
    x_all = x_all * scale
    s_all = scores(x_all)
    assert torch.equal(s_all, s_int * scale) and 4.0 < float(s_all.abs().max()) <= 16.0
    assert torch.equal(scores(x_all, rb), s_all)        # rounding the operands and T to bf16 changes nothing
    return {"x": x_all[:row.b].contiguous(), "bank_x": x_all[row.b:].contiguous(), "y_all": y_all, "w": w, "s_all": s_all}
