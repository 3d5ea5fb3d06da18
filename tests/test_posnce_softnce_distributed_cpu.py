"""The study-positive and the soft-target InfoNCE over a sharded global batch (distributed.GlobalBatchPosNceFn /
distributed_label_targets.GlobalBatchSoftNceFn) on the CPU: gloo at 2 and 3 ranks with an fp64 ops object (tests/posnce_softnce_shard_worker.py)
against the single-process fp64 restatements (tests/posnce_reference.py, tests/softnce_reference.py) at the global batch;
plus the C ABI of the row-block entry points, host side only."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posnce_reference as pref  # noqa: E402
import posnce_softnce_shard_worker as worker  # noqa: E402
import softnce_reference as sref  # noqa: E402


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _close(got, want, what):
    got, want = got.detach().double().numpy(), want.detach().double().numpy()
    scale = max(float(np.abs(want).max()) if want.size else 0.0, 1e-300)
    err = float(np.abs(got - want).max()) / scale if want.size else 0.0
    assert err <= 1e-9 or np.allclose(got, want, rtol=1e-9, atol=1e-12), (what, err)


def _check_ranks(outs, key, want, want_extra, extra, b_local):
    for r, o in enumerate(outs):
        got = o[key]
        sl = slice(r * b_local, (r + 1) * b_local)
        tag = (key, r)
        _close(got["loss"], want["loss"].reshape(1), tag + ("loss",))
        _close(got["loss_no_grad"], want["loss"].reshape(1), tag + ("loss, no_grad",))
        assert not got["no_grad_requires_grad"]
        _close(got["lse_rows"], want["lse_rows"][sl], tag + ("lse_rows",))
        _close(got["lse_cols"], want["lse_cols"], tag + ("lse_cols",))
        _close(got[extra], want_extra[sl], tag + (extra,))
        _close(got["dx"], want["grads"][0][sl], tag + ("dx",))
        _close(got["dy"], want["grads"][1][sl], tag + ("dy",))
        for n, (g, w) in enumerate(zip(got["dparams"], want["grads"][2:])):
            _close(g, w, tag + (f"dparam{n}",))
        # every rank merges the same gathered parts in rank order: identical bits
        assert torch.equal(got["loss"], outs[0][key]["loss"]), tag
        assert torch.equal(got["lse_cols"], outs[0][key]["lse_cols"]), tag
        for g, g0 in zip(got["dparams"], outs[0][key]["dparams"]):
            assert torch.equal(g, g0), tag


def test_cases_meet_the_conditions():
    """Same-study pairs and similar masks that straddle two ranks exist at both worlds; mix = 0 is at most a third."""
    assert sum(1 for _, _, mix in worker.LABEL_CASES if mix == 0.0) * 3 <= len(worker.LABEL_CASES)
    assert {mix for _, _, mix in worker.LABEL_CASES} == {0.0, 0.5, 1.0}
    assert len({tau for _, tau, _ in worker.LABEL_CASES}) == 2
    for world in (2, 3):
        b_local, b = 5, 5 * world
        rank_of = torch.arange(b) // b_local
        for pattern in ("dup_across", "majority", "all_equal"):
            sid = worker.id_pattern(pattern, b, b_local)
            same = (sid[:, None] == sid[None, :]) & (rank_of[:, None] != rank_of[None, :])
            assert bool(same.any()), (world, pattern)
        sid = worker.id_pattern("dup_in_rank", b, b_local)
        same = (sid[:, None] == sid[None, :]) & ~torch.eye(b, dtype=torch.bool)
        assert bool(same.any()) and not bool((same & (rank_of[:, None] != rank_of[None, :])).any())
        lab = worker.label_pattern("random", b, b_local)
        overlap = ((lab[:, None] & lab[None, :]) != 0) & (rank_of[:, None] != rank_of[None, :])
        assert bool(overlap.any())
        lab = worker.label_pattern("one_bit_per_study", b, b_local)
        assert bool(((lab[:, None] == lab[None, :]) & (rank_of[:, None] != rank_of[None, :])).any())
        assert all(bin(v).count("1") == 1 for v in lab.tolist())
        assert int(worker.label_pattern("bit63", b, b_local)[0]) < 0


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("critic", ["bilinear", "separable"])
@pytest.mark.parametrize("estimator", ["infonce_rowwise", "infonce_symmetric"])
def test_sharded_losses_equal_single_process(tmp_path, world, critic, estimator):
    b_local, d, k = 5, 4, 3
    mp.spawn(worker.run, args=(world, _free_port(), b_local, d, k, critic, estimator, str(tmp_path)), nprocs=world,
             join=True)
    b = world * b_local
    x, y, params = worker.problem(critic, b, d, k, salt=b + d)
    outs = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=True) for r in range(world)]
    for pattern in worker.ID_PATTERNS:
        sid = worker.id_pattern(pattern, b, b_local)
        want = pref.step(worker.SCORERS[critic], [x, y, *params], sid, estimator)
        n_pos = pref.positives(sid).sum(dim=1)
        _check_ranks(outs, f"pos/{pattern}", want, n_pos, "n_pos", b_local)
        if pattern == "unique":
            for o in outs:
                assert int(o[f"pos/{pattern}"]["n_pos"].max()) == 1
    for pattern, tau, mix in worker.LABEL_CASES:
        lab = worker.label_pattern(pattern, b, b_local)
        want = sref.step(worker.SCORERS[critic], [x, y, *params], lab, estimator, tau, mix)
        z = sref.targets(lab, tau, mix)[2]
        _check_ranks(outs, f"soft/{pattern}/{tau}/{mix}", want, z, "target_norm", b_local)
    # bit 63 is ignored: the masks with it give what the masks without it give
    for o in outs:
        _close(o["soft/bit63/0.5/0.5"]["loss"], o["soft/random/0.5/0.5"]["loss"], "bit 63")


def test_public_functions_reject_bad_arguments():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "mutual-information-multimodal_amd"))
    from mutual_info_img_txt import _hip
    from mutual_info_img_txt.distributed import global_batch_study_positive_infonce
    from mutual_info_img_txt.distributed_label_targets import global_batch_soft_target_infonce
    x, y, codes = torch.zeros(4, 3), torch.zeros(4, 3), torch.arange(4)
    with pytest.raises(ValueError, match="bilinear and separable"):
        global_batch_study_positive_infonce(x, y, codes, [], critic="concat_mlp")
    with pytest.raises(ValueError, match="bilinear and separable"):
        global_batch_soft_target_infonce(x, y, codes, [], tau=0.5, mix=0.5, critic="concat_mlp")
    with pytest.raises(ValueError, match="tau"):
        global_batch_soft_target_infonce(x, y, codes, [torch.zeros(3, 3)], tau=0.0, mix=0.5)
    with pytest.raises(ValueError, match="mix"):
        global_batch_soft_target_infonce(x, y, codes, [torch.zeros(3, 3)], tau=0.5, mix=1.5)
    with pytest.raises(TypeError):
        global_batch_soft_target_infonce(x, y, codes, [torch.zeros(3, 3)])  # tau and mix are required keywords
    with pytest.raises(ValueError, match="precision"):
        global_batch_study_positive_infonce(x, y, codes, [torch.zeros(3, 3)], precision="fp8")
    with pytest.raises(ValueError, match="int64"):
        global_batch_study_positive_infonce(x, y, codes.float(), [torch.zeros(3, 3)])
    # training losses, not estimator names
    assert not any("pos" in n or "soft" in n for n in _hip.ESTIMATOR_TABLE)


# ------------------------------------------------------------------------------------------------ C ABI, host side
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mutual_info_img_txt import _hip
    return _hip.load()


SHARD_SYMBOLS = tuple(f"mi_{loss}_{name}" for loss in ("posnce", "softnce") for name in (
    "part_floats", "bilinear_shard_workspace_bytes", "bilinear_shard_fwd", "bilinear_shard_bwd", "merge_workspace_bytes",
    "merge_parts", "separable_shard_workspace_bytes", "separable_shard_fwd", "separable_shard_bwd"))


def test_shard_symbols_exported(lib):
    from mutual_info_img_txt import _hip
    for name in SHARD_SYMBOLS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES, name
    assert lib.mi_abi_version() == 4


def test_shard_sizes_host_only(lib):
    assert lib.mi_posnce_part_floats(512, 4096) == 3 * 4096 + 2 * 512
    assert lib.mi_softnce_part_floats(512, 4096) == 3 * 4096 + 512
    for loss in ("posnce", "softnce"):
        part_floats = getattr(lib, f"mi_{loss}_part_floats")
        merge_bytes = getattr(lib, f"mi_{loss}_merge_workspace_bytes")
        bil = getattr(lib, f"mi_{loss}_bilinear_shard_workspace_bytes")
        sep = getattr(lib, f"mi_{loss}_separable_shard_workspace_bytes")
        assert part_floats(0, 4096) == 0 and part_floats(512, 0) == 0 and part_floats(-1, 8) == 0
        assert merge_bytes(4096) >= 2 * 4096 * 4
        assert merge_bytes(0) == 0 and merge_bytes(-3) == 0
        for prec in (0, 1, 2):
            part = bil(1024, 4096, 512, 512, prec)
            whole = bil(4096, 4096, 512, 512, prec)
            assert 0 < part < whole
            assert 0 < sep(96, 192, 64, 64, 32, prec)
        assert bil(0, 64, 8, 8, 1) == 0 and bil(8, 64, 0, 8, 1) == 0 and bil(8, -64, 8, 8, 1) == 0
        assert sep(8, 64, 8, 8, 0, 1) == 0 and sep(0, 64, 8, 8, 4, 1) == 0


# argument lists of the four shard calls with every pointer valid-looking (never dereferenced: each call below fails a
# host-side check) and the defaults b_rows = 64, b = 128, row_offset = 0, widths 64, d_proj = 32, rowwise, bf16
FAKE = ctypes.c_void_p(1 << 20).value
BIG = 1 << 40


def _args(loss, critic, half, **kw):
    a = dict(x=FAKE, y=FAKE, w=FAKE, wg=FAKE, wh=FAKE, rows=FAKE, cols=FAKE, br=64, b=128, off=0, dx=64, dy=64, k=32,
             mode=0, prec=1, tau=0.5, mix=0.5, part=FAKE, lse_cols=FAKE, gx=FAKE, gy=FAKE, gw=FAKE, gwg=FAKE, gwh=FAKE,
             ws=FAKE)
    a.update(kw)
    head = [a["x"], a["y"]] + ([a["w"]] if critic == "bilinear" else [a["wg"], a["wh"]]) + [a["rows"], a["cols"]]
    sizes = [a["br"], a["b"], a["off"], a["dx"], a["dy"]] + ([] if critic == "bilinear" else [a["k"]])
    cfg = [a["mode"], a["prec"]] + ([a["tau"], a["mix"]] if loss == "softnce" else [])
    if half == "fwd":
        tail = [a["part"], None, None]
    else:
        grads = [a["gx"], a["gy"]] + ([a["gw"]] if critic == "bilinear" else [a["gwg"], a["gwh"]])
        tail = [a["lse_cols"], None] + grads
    return head + sizes + cfg + tail + [a["ws"], BIG, None]


CALLS = [(loss, critic, half) for loss in ("posnce", "softnce") for critic in ("bilinear", "separable")
         for half in ("fwd", "bwd")]


def _rejected(lib, loss, critic, half, needle=None, **kw):
    rc = getattr(lib, f"mi_{loss}_{critic}_shard_{half}")(*_args(loss, critic, half, **kw))
    assert rc == -1, (loss, critic, half, kw, rc)
    if needle is not None:
        assert needle in lib.mi_last_error(), (loss, critic, half, kw, lib.mi_last_error())


@pytest.mark.parametrize("loss,critic,half", CALLS)
def test_shard_arguments_rejected_without_gpu(lib, loss, critic, half):
    """Every MI_EINVAL of the row-block calls, answered from fake device pointers and a null stream: before the device
    is touched.  Each case breaks ONE argument of an otherwise acceptable list, and names the check that caught it."""
    # null pointers, one at a time
    nulls = ["x", "y", "rows", "cols", "ws"] + (["part"] if half == "fwd" else ["gx", "gy"])
    nulls += ["wg", "wh"] if critic == "separable" else []
    nulls += ["gwg", "gwh"] if (critic, half) == ("separable", "bwd") else []
    for name in nulls:
        _rejected(lib, loss, critic, half, b"null", **{name: None})
    # sizes
    for kw in (dict(br=0), dict(b=0, br=0), dict(dx=0), dict(dy=0)):
        _rejected(lib, loss, critic, half, **kw)
    if critic == "separable":
        _rejected(lib, loss, critic, half, b"projection", k=0)
    # b_rows <= b and the row block inside [0, b)
    _rejected(lib, loss, critic, half, b"b_rows", br=256, b=128)
    _rejected(lib, loss, critic, half, b"row block", off=96)
    _rejected(lib, loss, critic, half, b"row block", off=-1)
    # counts travel as floats
    _rejected(lib, loss, critic, half, b"2^24", br=64, b=1 << 24)
    # mode and precision
    _rejected(lib, loss, critic, half, b"mode", mode=2)
    for prec in (3, 4, 5):
        _rejected(lib, loss, critic, half, b"precision", prec=prec)
    # tau and mix
    if loss == "softnce":
        for tau in (0.0, -1.0, float("inf"), float("nan")):
            _rejected(lib, loss, critic, half, b"tau", tau=tau)
        for mix in (-0.1, 1.1, float("nan")):
            _rejected(lib, loss, critic, half, b"mix", mix=mix)
    # the weightless form needs equal widths; a partial gradient set
    if critic == "bilinear":
        if half == "fwd":
            _rejected(lib, loss, critic, half, b"d_img == d_txt", w=None, dy=32)
        else:
            _rejected(lib, loss, critic, half, b"grad_w", w=None, gw=None, dy=32)
            _rejected(lib, loss, critic, half, b"grad_w", gw=None)
            _rejected(lib, loss, critic, half, b"grad_w", w=None)
    # the symmetric backward needs the merged column LSEs
    if half == "bwd":
        _rejected(lib, loss, critic, half, b"lse_cols", mode=1, lse_cols=None)


@pytest.mark.parametrize("loss", ["posnce", "softnce"])
def test_merge_arguments_rejected_without_gpu(lib, loss):
    merge = getattr(lib, f"mi_{loss}_merge_parts")
    ok = [FAKE, 2, 64, 128, 0, FAKE, FAKE, FAKE, BIG, None]
    for at in (0, 5, 6, 7):
        bad = list(ok)
        bad[at] = None
        assert merge(*bad) == -1
        assert b"null" in lib.mi_last_error()
    assert merge(FAKE, 3, 64, 128, 0, FAKE, FAKE, FAKE, BIG, None) == -1
    assert b"n_ranks" in lib.mi_last_error()
    assert merge(FAKE, 0, 64, 0, 0, FAKE, FAKE, FAKE, BIG, None) == -1
    assert merge(FAKE, 2, 1 << 23, 1 << 24, 0, FAKE, FAKE, FAKE, BIG, None) == -1
    assert b"2^24" in lib.mi_last_error()
    assert merge(FAKE, 2, 64, 128, 7, FAKE, FAKE, FAKE, BIG, None) == -1
    assert b"mode" in lib.mi_last_error()
    assert merge(FAKE, 2, 64, 128, 0, FAKE, FAKE, FAKE, 16, None) == -3  # a short workspace: MI_EWORKSPACE
