"""critic_ops.resolve_critic: the one precision-name -> code resolution and parameter validation of the critics.  The
expected codes are what each caller computed before the resolver existed, from the same arguments:

* fused_mi_bound (and its per-sample InfoNCE path) and GraphedMiStep: ``_hip.resolve_precision(p, True, (b, d_img,
  d_txt))`` for a BilinearCritic, ``_precision_code(p)`` for a SeparableCritic and for GraphedMiStep's critic=None,
  ``_hip.resolve_precision(p, False, concat_hidden=(h1, h2))`` for a make_mlp critic;
* the sharded path (distributed.global_batch_mi_bound / GlobalBatchGraphStep): the same, but with the RANK's row count
  in place of b.

CPU only: the resolution is host arithmetic."""
import pytest
import torch

from mutual_info_img_txt import _hip, distributed
from mutual_info_img_txt.critic_ops import _concat_params, _precision_code, resolve_critic
from mutual_info_img_txt.model import BilinearCritic, SeparableCritic, make_mlp

PRECISIONS = ["f32", "fp32", "f32_exact", "bf16", "bf16x3", "fp8", "f16"]
SHAPES = [(64, 64, 64), (60, 64, 64), (64, 36, 36), (64, 64, 40)]  # (b, d_img, d_txt): multiples of 8 or not
HIDDEN = [(128, 256), (64, 512), (96, 256), (128, 128)]  # f16x3 sizes of the fused concat kernels, then two that are not


def _table(dx, dy):
    """(critic, kind, expected code as a function of (precision, b))."""
    yield BilinearCritic(dx, dy), "bilinear", lambda p, b: _hip.resolve_precision(p, True, (b, dx, dy))
    yield SeparableCritic(dx, dy, 16), "separable", lambda p, b: _precision_code(p)
    if dx == dy:
        yield None, "bilinear", lambda p, b: _precision_code(p)
    for h in HIDDEN:
        yield make_mlp(dx + dy, list(h)), "concat_mlp", lambda p, b, h=h: _hip.resolve_precision(p, False, concat_hidden=h)


@pytest.mark.parametrize("shape", SHAPES)
def test_resolution_table(shape):
    b, dx, dy = shape
    for critic, kind, expect in _table(dx, dy):
        for p in PRECISIONS:
            got_kind, params, code = resolve_critic(critic, p, b, dx, dy)
            assert (got_kind, code) == (kind, expect(p, b)), (type(critic).__name__, p, shape)
            if isinstance(critic, BilinearCritic):
                assert params == [critic.weight]
            elif isinstance(critic, SeparableCritic):
                assert params == [critic.wg, critic.wh]
            elif critic is None:
                assert params == []
            else:
                assert all(a is c for a, c in zip(params, _concat_params(critic))) and len(params) == 6


def test_resolution_spot_values():
    f32, bf16x3, f16x3 = _hip.MI_PREC_F32, _hip.MI_PREC_BF16X3, _hip.MI_PREC_F16X3
    assert resolve_critic(BilinearCritic(64, 64), "f32", 64, 64, 64)[2] == bf16x3
    assert resolve_critic(BilinearCritic(64, 64), "f32", 60, 64, 64)[2] == f32
    assert resolve_critic(BilinearCritic(64, 64), "f32_exact", 64, 64, 64)[2] == f32
    assert resolve_critic(BilinearCritic(64, 64), "bf16x3", 60, 64, 64)[2] == bf16x3
    # GraphedMiStep(critic=None) does not map "f32" to bf16x3 (a BilinearCritic of the same shape does)
    assert resolve_critic(None, "f32", 64, 64, 64)[2] == f32
    assert resolve_critic(SeparableCritic(64, 64, 16), "f32", 64, 64, 64)[2] == f32
    assert resolve_critic(make_mlp(128, [128, 256]), "f32", 64, 64, 64)[2] == f16x3
    assert resolve_critic(make_mlp(128, [96, 256]), "f32", 64, 64, 64)[2] == f32
    assert resolve_critic(make_mlp(128, [128, 256]), "bf16", 64, 64, 64)[2] == _hip.MI_PREC_BF16


def test_resolution_rejects():
    with pytest.raises(ValueError, match="unknown precision"):
        resolve_critic(BilinearCritic(8, 8), "f64", 8, 8, 8)
    with pytest.raises(ValueError, match="projection shapes"):
        resolve_critic(SeparableCritic(8, 16, 4), "f32", 8, 8, 8)
    with pytest.raises(ValueError, match="critic expects 32 inputs"):
        resolve_critic(make_mlp(32, [64, 256]), "f32", 8, 8, 8)
    with pytest.raises(ValueError, match="widths must agree"):
        resolve_critic(None, "f32", 8, 8, 16)
    with pytest.raises(ValueError, match="make_mlp"):
        resolve_critic(make_mlp(16, [8]), "f32", 8, 8, 8)


@pytest.fixture
def sharded_code(monkeypatch):
    """The precision code global_batch_mi_bound hands on, driven on the CPU with the exchange stubbed out."""
    got = []

    class Stub:
        @staticmethod
        def apply(ops, group, est, prec, *rest):
            got.append(prec)
            return torch.zeros(1), None
    monkeypatch.setattr(distributed, "GlobalBatchCriticFn", Stub)

    def code(kind, precision, rows, d, params):
        x, y, sid = torch.zeros(rows, d), torch.zeros(rows, d), torch.arange(rows)
        distributed.global_batch_mi_bound(x, y, sid, params, "dv", precision, kind, ops=object())
        return got.pop()
    return code


@pytest.mark.parametrize("rows", [64, 60, 4])
def test_sharded_resolution(sharded_code, rows):
    d = 64
    cases = [("bilinear", [torch.zeros(d, d)], lambda p: _hip.resolve_precision(p, True, (rows, d, d))),
             ("separable", [torch.zeros(d, 16), torch.zeros(d, 16)], _precision_code)]
    for h in HIDDEN:
        params = [p.detach() for p in _concat_params(make_mlp(2 * d, list(h)))]
        cases.append(("concat_mlp", params, lambda p, h=h: _hip.resolve_precision(p, False, concat_hidden=h)))
    for kind, params, expect in cases:
        for p in PRECISIONS:
            assert sharded_code(kind, p, rows, d, params) == expect(p), (kind, p, rows)


def test_sharded_resolution_uses_the_row_block(sharded_code):
    # not the same as one GPU: a rank holding 4 rows of a global batch of 8 resolves "f32" to exact fp32, where one GPU
    # at b = 8 runs bf16x3.  Kept as it is; pinned so that a change is deliberate.
    assert sharded_code("bilinear", "f32", 4, 64, [torch.zeros(64, 64)]) == _hip.MI_PREC_F32
    assert resolve_critic(BilinearCritic(64, 64), "f32", 8, 64, 64)[2] == _hip.MI_PREC_BF16X3
