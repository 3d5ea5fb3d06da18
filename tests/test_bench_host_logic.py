"""Host-side logic of bench.py that needs no GPU: the algorithmic flop counts behind `roofline.achieved`, the source
fingerprint that decides whether a committed PMC pass may be attached, and the refusal of a stale pass."""
import json

import pytest

import bench


def test_algorithmic_flops_match_design():
    b, d = 4096, 512
    # fused B x B launch: scores + two gradient contractions, no credit for the recomputed score product
    assert bench.kernel_flops("bilinear fused S | P Y | P^T T", b, b, d, d) == 6.0 * b * b * d
    # whole step: three B x B x d products and three B x d x d products, 2 flops per multiply-add
    assert bench.algorithmic_flops("bilinear", b, d, d) == 6.0 * b * b * d + 6.0 * b * d * d
    assert bench.PEAK_TFLOPS["bf16"] == 2500.0 and bench.PEAK_TFLOPS["f32"] == 157.3


def test_committed_pmc_pass_belongs_to_these_sources():
    """profiles/*_pmc_traffic.json of the newest round must have been taken on the kernel sources in the tree (otherwise
    `roofline.traffic` silently goes null in the judged bench line)."""
    c = bench.measured_counters("bilinear fused S | P Y | P^T T", 4096, 512)
    assert c is not None, "no profiles/*_pmc_traffic.json"
    if c.get("stale"):
        pytest.skip("the committed PMC pass predates the kernel sources: re-run tools/profile_round.sh before the round ends")
    assert abs(c["bytes"] - (c["fetch"] + c["write"])) <= 2 and 0.0 < c["mfma_busy_frac"] < 1.0  # (each is rounded)
    # the separable leg at B = 256 runs the same kernel in the same passes: the lookup must take the headline's launch
    assert 90e6 < c["bytes"] < 130e6 and c["mfma_busy_frac"] > 0.3
    f8 = bench.measured_counters("fp8 mode dT = G Y | dY = G^T T", 8192, 1024, "fp8")
    assert f8 and not f8.get("stale") and f8["bytes"] > 400e6 and 0.3 < f8["mfma_busy_frac"] < 0.9
    assert bench.measured_counters("bilinear fused S | P Y | P^T T", 2048, 512) is None  # only the profiled configuration


def test_stale_pmc_pass_is_refused(tmp_path, monkeypatch):
    root = tmp_path / "repo"
    (root / "profiles").mkdir(parents=True)
    doc = {"csrc_sha": "0" * 12, "kernels": {"void mi::bilinear_flash_kernel<512, true>(mi::FlashArgs) grid=1":
                                              {"fetch_bytes": 1.0, "write_bytes": 2.0, "total_bytes": 3.0}}}
    (root / "profiles" / "zz_pmc_traffic.json").write_text(json.dumps(doc))
    monkeypatch.setattr(bench, "ROOT", str(root))
    c = bench.measured_counters("bilinear fused S | P Y | P^T T", 4096, 512)
    assert c == {"stale": True, "source": "zz_pmc_traffic.json",
                 "note": "PMC pass predates the current kernel sources: not attached"}
    doc["csrc_sha"] = bench.csrc_sha()
    (root / "profiles" / "zz_pmc_traffic.json").write_text(json.dumps(doc))
    c = bench.measured_counters("bilinear fused S | P Y | P^T T", 4096, 512)
    assert c["bytes"] == 3 and c["source"] == "zz_pmc_traffic.json"


def test_cpu_leg_thread_count(monkeypatch):
    """`cpu_baseline.cores`: affinity mask, cgroup quota or the pool's 16-thread share, whichever is smallest; an explicit
    MI_BENCH_CPU_THREADS wins."""
    import os
    import bench
    monkeypatch.delenv("MI_BENCH_CPU_THREADS", raising=False)
    n = bench.host_cpu_share()
    assert 1 <= n <= min(len(os.sched_getaffinity(0)), 16) or n <= len(os.sched_getaffinity(0))
    monkeypatch.setenv("MI_BENCH_CPU_THREADS", "3")
    assert bench.host_cpu_share() == 3


def test_dump_outputs_of_the_last_step(tmp_path):
    """`--dump-outputs DIR`: the step's outputs as float32 .npy files under their names (bf16 gradients widened, the loss
    as one element); below the budget every value is written."""
    import types

    import numpy as np
    import torch
    gx = torch.randn(64, 8, generator=torch.Generator().manual_seed(1))
    step_obj = types.SimpleNamespace(loss_buf=torch.tensor([1.25]), grad_x=gx.bfloat16(), grad_y=gx * 2,
                                     grad_params=[torch.ones(8, 8), torch.zeros(8)])
    st = object.__new__(bench.Stepper)
    st.step_obj, st.dist_mode, st.world = step_obj, False, 1
    outs = st.host_outputs()
    assert sorted(outs) == ["grad_param0", "grad_param1", "grad_x", "grad_y", "loss"]
    bench.dump_outputs(outs, str(tmp_path / "d"))
    got = {p.stem: np.load(p) for p in (tmp_path / "d").glob("*.npy")}
    assert sorted(got) == sorted(outs) and all(a.dtype == np.float32 for a in got.values())
    assert got["loss"].tolist() == [1.25]
    np.testing.assert_array_equal(got["grad_x"], gx.bfloat16().float().numpy())
    np.testing.assert_array_equal(got["grad_y"], (gx * 2).numpy())
    assert got["grad_param1"].shape == (8,)


def test_dump_outputs_sample_a_large_step(tmp_path):
    """Beyond the budget every multi-row array keeps the same share of its rows, the same rows on every run."""
    import numpy as np
    import torch
    outs = {"loss": torch.tensor([0.5]), "grad_x": torch.arange(4000 * 16, dtype=torch.float32).reshape(4000, 16),
            "grad_param0": torch.arange(1000 * 16, dtype=torch.float32).reshape(1000, 16)}
    budget = 100_000
    for run in ("a", "b"):
        bench.dump_outputs(outs, str(tmp_path / run), budget=budget)
    a = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    b = {p.stem: np.load(p) for p in (tmp_path / "b").glob("*.npy")}
    assert sum(v.nbytes for v in a.values()) <= budget
    assert a["loss"].tolist() == [0.5] and a["grad_param0"].shape[0] > 0
    assert abs(a["grad_x"].shape[0] / 4000 - a["grad_param0"].shape[0] / 1000) < 1e-3  # the same share (up to a row)
    for name, v in a.items():
        np.testing.assert_array_equal(v, b[name])
    rows = a["grad_x"][:, 0] / 16  # the sampled rows are whole rows of the output, in order
    assert np.all(np.diff(rows) > 0) and np.array_equal(a["grad_x"], outs["grad_x"].numpy()[rows.astype(int)])


def test_steps_must_be_positive(monkeypatch):
    """`ms_per_step` divides by --steps: a run of no timed steps is refused at the command line."""
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args()
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "7", "--warmup", "0", "--dump-outputs", "out"])
    args = bench.parse_args()
    assert args.steps == 7 and args.dump_outputs == "out"


def test_full_is_opt_in(monkeypatch):
    """A plain run measures the headline only; the other legs, baselines and per-kernel figures need `--full`."""
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert bench.parse_args().full is False
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "5", "--full", "--no-cpu-baseline"])
    args = bench.parse_args()
    assert args.full is True and args.no_cpu_baseline and args.steps == 5
