#!/usr/bin/env python3
"""Benchmark of the MI-critic hot path: one critic forward + backward over a synthetic batch per step.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
      N > 1: either launched by torch.distributed.run (one rank per GPU; RANK / LOCAL_RANK / WORLD_SIZE from the
      environment) or, when WORLD_SIZE is not set, bench.py starts the N ranks itself as child processes and relays
      rank 0's line; --gpus must equal the number of ranks, anything else is an error
      --dump-outputs DIR: after the K timed steps of the headline, what its last step handed back (loss, dX, dY and the
      critic's parameter gradients) goes to DIR/<name>.npy, so that two builds can be compared output for output on the
      same seeded inputs
      --full: everything else the benchmark measures (see below); without it a run does only what the headline needs

Headline workload (BASELINE.json configs[3], the configuration its metric is quoted on; it fits one GPU):
  global-batch "InfoNCE" (reference semantics, mi_critics.py:14-23), bilinear critic S = (X W) Y^T, B_global = 4096,
  d = 512, bf16 MFMA operands / fp32 accumulate, unique study ids, inputs resident in HBM.  With N GPUs the SAME global
  batch is sharded by row blocks (strong scaling) and the text embeddings are all-gathered over RCCL.
A step = pair enumeration + scorer + bound + ALL gradients (dX, dY, d theta) through the product API
`graphed.GraphedMiStep` (one GPU) / `distributed.GlobalBatchGraphStep` (N GPUs): the C-ABI launches of the step,
issued as direct calls or replayed from hipGraphs (`--graph auto`, the default, times both during warm-up and keeps the
faster; `--graph on|off` forces one).  Encoders, optimisers and data loading are not in the metric.

Before the W warm-up steps the GPU is brought to the clocks of a sustained run by about 300 ms of untimed steps
(`--clock-warmup-ms`, 0 = off; reported in `timing.clock_warmup`): 20 timed steps that start cold take ~5 % longer each
than the same steps inside a long run.

One JSON line on stdout (rank 0): the driver's contract (`value` from exactly K steps between barriers / synchronize).
A plain run sets up, probes the launch mode, warms the clocks, takes the W + K steps, writes --dump-outputs and prints the
line; nothing else.  With `--full` the line also carries `cold_ms_per_step` (the same W + K steps taken first, before the
clock warm-up), `timing` (median / p10 / p90 of >= 50 individually hipEvent-timed steps, graph and eager), `roofline`
(dominant kernel, HIP-event timed through the library's profiling hook; measured HBM bytes and matrix-pipe busy fraction
from the newest committed PMC pass of the SAME kernel sources) and `kernels_us`, and the legs that take runs of their own:
`other_boundary` (the headline step through the other dtype boundary), `parity_mode` (the same step in the modes held to
fp32 tolerances: "f32_exact" and "bf16x3"), `fp8_mode` (BASELINE configs[4] on one GPU: B = 8192, d = 1024),
`separable_mode` (BASELINE configs[1]), `secondary` (the reference's own critic, make_mlp(2d,[1024,512])) and
`cpu_baseline` (the oracle timed on this box's host cores, rank 0, N = 1 only).  --timed-iters, --profile-steps, the
--no-* switches, --secondary-steps and --cpu-seconds shape those extras and matter only with `--full`.
"""
import argparse
import glob
import hashlib
import json
import math
import os
import statistics
import sys
import time

# multi-process GPU work on this pool needs dmabuf IPC: set before anything initialises HIP
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "mutual-information-multimodal_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_TFLOPS = {"bf16": 2500.0, "f16": 2500.0,  # fp16 MFMA runs at the bf16 rate (guide, Matrix cores)
               "f32": 157.3,  # dense MFMA peaks, /opt/skills/guides/MI355X_MICROARCH.md
               "f32_exact": 157.3,       # v_mfma_f32_32x32x2_f32 products ("f32" on the bilinear critic runs bf16x3)
               "bf16x3": 2500.0 / 3,     # three bf16 MFMAs per algorithmic product
               "f16x3": 2500.0 / 3,      # concat-MLP "f32": two-part fp16 operands, three MFMAs per product in the forward (two in the backward kernels)
               "fp8": 5000.0}            # the dense fp8 peak: the forward products run on v_mfma_scale_f32_32x32x64_f8f6f4
                                         # with unit block scales; the backward's contractions are bf16
PEAK_HBM_GBS = 8000.0
# the secondary leg (the reference's concat-MLP critic): fast 16-bit modes, the first one is the `secondary` number; and
# the modes that hold the fp32 tolerances
SECONDARY_FAST = {"concat_mlp": ["f16", "bf16"]}
SECONDARY_PARITY = ["f32", "f32_exact"]  # "f32" = the two-part fp16 scheme (MI_PREC_F16X3); "f32_exact" = fp32-input MFMA
# --dump-outputs: array bytes of one dump at most (the .npy headers stay well inside the 64 MB a dump may take)
DUMP_BYTES = 60 * 10**6


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--batch", type=int, default=4096, help="GLOBAL batch")
    p.add_argument("--dim", type=int, default=512)
    p.add_argument("--critic", default="bilinear", choices=["bilinear", "concat_mlp"])
    p.add_argument("--estimator", default="infonce", choices=["dv", "infonce"])
    p.add_argument("--precision", default="bf16", choices=["bf16", "f32", "f32_exact", "bf16x3", "fp8", "f16"])
    p.add_argument("--boundary", default="f32", choices=["bf16", "f32"],
                   help="dtype of the embeddings handed to the step and of the gradients handed back (one GPU, bilinear "
                        "critic, precision bf16): f32 = the reference's boundary (fp32 embeddings, model.py:540-555; the "
                        "headline of every round); bf16 = mi_bilinear_step_bf16, what encoders under autocast emit (the kernels "
                        "round fp32 embeddings to bf16 as their first act: same bits).  The line carries the other one as "
                        "`other_boundary`")
    p.add_argument("--graph", default="auto", choices=["auto", "on", "off", "full"],
                   help="on: replay the step from a hipGraph (one GPU: GraphedMiStep; N GPUs: the two compute sections "
                        "are graphs, the RCCL collectives stay eager between them).  off: the same C-ABI calls issued one "
                        "by one.  auto (default): one GPU times both during warm-up and keeps the faster; N GPUs = off.  full (N GPUs, "
                        "opt-in): ONE graph per step with the RCCL collectives captured in it")
    p.add_argument("--clock-warmup-ms", type=float, default=300.0,
                   help="untimed steps for about this long before the W warm-up steps (sustained-run clocks; 0 = off)")
    p.add_argument("--timed-iters", type=int, default=50, help="individually hipEvent-timed steps for the median (>= 50)")
    p.add_argument("--no-secondary", action="store_true")
    p.add_argument("--secondary-steps", type=int, default=5)
    p.add_argument("--no-parity-mode", action="store_true")
    p.add_argument("--no-fp8", action="store_true")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--cpu-seconds", type=float, default=15.0)
    p.add_argument("--profile-steps", type=int, default=5)
    p.add_argument("--master-port", type=int, default=0, help="rendezvous port when bench.py starts its own ranks")
    p.add_argument("--rendezvous-only", action="store_true",
                   help="start the ranks, form the process group (backend: MI_BENCH_BACKEND, default nccl), all-reduce one "
                        "number and print {world, sum}: the launcher's own test (runs under gloo without a GPU)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the outputs of the headline's last timed step to DIR/<name>.npy (float32): loss, grad_x, "
                        "grad_y (whole global batch) and grad_param<i> (the critic's parameters in C-ABI order); beyond "
                        f"{DUMP_BYTES // 10**6} MB in all, every array keeps the same share of its rows, picked by a "
                        "fixed seed")
    p.add_argument("--full", action="store_true",
                   help="also measure what the headline does not need: cold_ms_per_step, event-timed statistics, per-kernel "
                        "times and roofline, the other boundary, parity, fp8, separable and secondary legs, CPU baselines")
    args = p.parse_args()
    if args.steps < 1 or args.warmup < 0:
        p.error("--steps must be >= 1 and --warmup >= 0")
    return args


def launch_ranks(args):
    """`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment: start N ranks of this same script
    (one per GPU) under torch.distributed.run -- as CHILD processes, before this process has touched the GPU (a process
    that has initialised HIP must not exec or fork GPU work on this pool) -- relay rank 0's JSON line and the exit code."""
    import socket
    import subprocess
    port = args.master_port
    if not port:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE)
    out = proc.stdout.decode(errors="replace")
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    if proc.returncode != 0 or not lines:
        sys.stderr.write(out)
        sys.stderr.write(f"bench.py: the {args.gpus}-rank run failed (exit code {proc.returncode}); no result line\n")
        raise SystemExit(proc.returncode or 1)
    sys.stdout.write(lines[-1] + "\n")
    sys.stdout.flush()
    raise SystemExit(0)


def rendezvous_only(args, world, rank):
    backend = os.environ.get("MI_BENCH_BACKEND", "nccl")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    if backend == "nccl":
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    else:
        dev = torch.device("cpu")
    dist.init_process_group(backend, rank=rank, world_size=world)
    t = torch.tensor([float(rank + 1)], device=dev)
    dist.all_reduce(t)
    dist.barrier()
    if rank == 0:
        print(json.dumps({"world": dist.get_world_size(), "gpus_arg": args.gpus, "sum": float(t.item()), "backend": backend}),
              flush=True)
    dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------------
def make_inputs(batch, d_img, d_txt, seed, rank, world, device):
    """X, Y ~ N(0,1) from a seeded generator; every rank draws the full batch and keeps its row block, so
    an N-GPU run sees exactly the single-GPU data."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, d_img, generator=gen)
    y = torch.randn(batch, d_txt, generator=gen)
    br = batch // world
    sl = slice(rank * br, (rank + 1) * br)
    sid = torch.arange(batch, dtype=torch.int64)
    return x[sl].to(device), y[sl].to(device), sid[sl].to(device)


def make_critic(kind, d_img, d_txt, seed, device):
    from mutual_info_img_txt.model import BilinearCritic, make_mlp
    torch.manual_seed(seed)
    if kind == "bilinear":
        m = BilinearCritic(d_img, d_txt)
    elif kind == "separable":
        from mutual_info_img_txt.model import SeparableCritic
        m = SeparableCritic(d_img, d_txt, d_txt)
    else:
        m = make_mlp(d_img + d_txt, [1024, 512])  # reference main_utils.py:77 with 2d inputs
    return m.to(device)


def algorithmic_flops(kind, b, d_img, d_txt, h1=1024, h2=512):
    """fwd + bwd, no recompute credit."""
    if kind == "bilinear":
        return 6.0 * b * b * d_txt + 6.0 * b * d_img * d_txt
    if kind == "separable":  # two heads [d, d_proj = d_txt]
        return 6.0 * b * b * d_txt + 6.0 * b * (d_img + d_txt) * d_txt
    return 6.0 * b * b * h1 * h2 + 6.0 * b * b * h2 + 12.0 * b * (d_img + d_txt) / 2 * h1


def kernel_flops(name, br, b, d_img, d_txt, h1=1024, h2=512):
    """Algorithmic flops of ONE launch of a named kernel (0 for HBM-bound helper kernels)."""
    if name.startswith("bilinear"):
        if "fused S |" in name:  # scores + both B x B gradient contractions in one launch (no recompute credit)
            return 6.0 * br * b * d_txt
        if "fused S + LSE" in name:
            return 2.0 * br * b * d_txt
        if "from the fused sums" in name:
            return 0.0
        if "sums ->" in name:  # partial sums -> dT, dY fused with dX = dT W^T
            return 2.0 * br * d_img * d_txt
        if "dW" in name and "|" in name:  # two-problem launch: dW = X^T dT and dX = dT W^T
            return 4.0 * br * d_img * d_txt
        if "|" in name:  # two-problem launch: dT = G Y and dY = G^T T
            return 4.0 * br * b * d_txt
        if any(t in name for t in ("score+LSE", "bilinear G", "dT = G Y", "dY = G^T T")):
            return 2.0 * br * b * d_txt
        if "prep" in name or "slabs" in name or "flags" in name:
            return 0.0
        return 2.0 * br * d_img * d_txt
    if name in ("concat_fwd_kernel", "concat_bwd_duv_kernel", "concat_bwd_dw2_kernel"):
        return 2.0 * br * b * h1 * h2
    if name.startswith("concat U") or name.startswith("concat dX") or name.startswith("concat dW1x"):
        return 2.0 * br * d_img * h1
    if name.startswith("concat V") or name.startswith("concat dY") or name.startswith("concat dW1y"):
        return 2.0 * b * d_txt * h1
    return 0.0


class Stepper:
    """One critic forward + backward through the product API (no autograd anywhere in the timed path)."""

    def __init__(self, kind, args, rank, world, device, group, precision=None, graph=True, batch=None, dim=None,
                 boundary="f32"):
        from mutual_info_img_txt.graphed import GraphedMiStep
        self.kind, self.world, self.device = kind, world, device
        d = dim or args.dim
        batch = batch or args.batch
        precision = precision or args.precision
        x, y, sid = make_inputs(batch, d, d, 3, rank, world, device)
        self.critic = make_critic(kind, d, d, 3, device)
        self.dist_mode = world > 1 or bool(os.environ.get("MI_BENCH_FORCE_DIST"))
        self.graph_used = bool(graph)
        self.use_eager = not graph
        self.launch_probe_ms = None
        if self.dist_mode and args.graph == "auto":
            # between RCCL calls a replay only adds its fixed cost: measured with one rank through the RCCL path, direct
            # calls 0.183 ms / step against 0.197 ms for the two replays.  No per-rank probe (all ranks must agree).
            graph = False
            self.graph_used = False
            self.use_eager = True
        if self.dist_mode:
            from mutual_info_img_txt.distributed import GlobalBatchGraphStep
            from mutual_info_img_txt.mi_critics import _concat_params
            params = [self.critic.weight] if kind == "bilinear" else list(_concat_params(self.critic))
            if kind != "bilinear":
                params[4] = params[4].reshape(-1)
            self.step_obj = GlobalBatchGraphStep(x, y, sid, [p.detach() for p in params], args.estimator, precision,
                                                 critic=kind, group=group,
                                                 capture="full" if args.graph == "full" else bool(graph))
            self.eager_obj = self.step_obj if not graph else None
        else:
            self.step_obj = GraphedMiStep(self.critic, batch, d, d, args.estimator, precision, device, capture=bool(graph),
                                          boundary=boundary)
            # both boundaries see the same VALUES: the synthetic embeddings rounded to bf16 (exact in fp32)
            if precision == "bf16" and kind == "bilinear":
                x, y = x.bfloat16().float(), y.bfloat16().float()
            self.step_obj.set_inputs(x.to(self.step_obj.x.dtype), y.to(self.step_obj.y.dtype), sid)
            self.eager_obj = self.step_obj

    def step(self):
        if self.use_eager:
            return self.eager_step()
        return self.step_obj.step()

    def choose_launch_mode(self, world):
        """--graph auto: time a few steps of graph replay and of direct calls and keep the faster (a replay has ~10 us of
        fixed cost; direct calls need a host that keeps ahead of the kernels).  Single GPU only."""
        if self.dist_mode or not self.graph_used:
            return
        res = {}
        for mode in ("graph", "eager"):
            self.use_eager = mode == "eager"
            for _ in range(5):
                self.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(30):
                self.step()
            torch.cuda.synchronize()
            res[mode] = (time.perf_counter() - t0) / 30 * 1e3
        self.use_eager = res["eager"] < res["graph"]
        self.launch_probe_ms = {k: round(v, 5) for k, v in res.items()}

    def eager_step(self):
        """The same C-ABI calls issued one by one (per-kernel event profiling needs real launches)."""
        o = self.step_obj
        if self.dist_mode:
            return o.step_eager()
        o._step()  # one C-ABI call for the bilinear critic (mi_bilinear_step), forward + backward calls otherwise
        return o.loss_buf

    def loss(self):
        o = self.step_obj
        return float((o.loss if self.dist_mode else o.loss_buf).detach().float().sum().item())

    def host_outputs(self):
        """What the last step handed its caller, as float32 host tensors: the loss, dX, dY and the gradients of the
        critic's parameters.  With several ranks the row blocks of dX and dY are gathered in rank order (a collective:
        every rank calls this), so the arrays are those of the whole global batch."""
        o = self.step_obj
        out = {"loss": (o.loss if self.dist_mode else o.loss_buf).reshape(-1), "grad_x": o.grad_x, "grad_y": o.grad_y}
        if self.dist_mode:
            for k in ("grad_x", "grad_y"):
                parts = [torch.empty_like(out[k]) for _ in range(self.world)]
                dist.all_gather(parts, out[k].contiguous())
                out[k] = torch.cat(parts)
        for i, g in enumerate(o.grad_params):
            out[f"grad_param{i}"] = g
        return {k: v.detach().to("cpu", torch.float32) for k, v in out.items()}


def dump_outputs(outputs, out_dir, budget=DUMP_BYTES):
    """``outputs`` (name -> float32 host tensor) as ``out_dir/<name>.npy``.  Beyond ``budget`` bytes in all, every array
    of more than one row keeps the same share of its rows; the rows are drawn from a fixed seed and kept in order, so two
    runs of the same shapes keep the same rows."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: v.numpy() for k, v in outputs.items()}
    fixed = sum(a.nbytes for a in arrays.values() if a.ndim == 0 or a.shape[0] <= 1)
    rows_bytes = sum(a.nbytes for a in arrays.values()) - fixed
    for name, a in arrays.items():
        if fixed + rows_bytes > budget and a.ndim and a.shape[0] > 1:
            keep = max(1, a.shape[0] * (budget - fixed) // rows_bytes)
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def clock_warmup(stepper, budget_s, world):
    """Untimed steps for about ``budget_s`` seconds BEFORE the contract's W warm-up steps, so that the timed region sees
    the clocks of a sustained run.  Measured (profiles/README.md): the same 20 timed steps take 0.1083 ms each when they
    start ~15 ms after the first launch and 0.102 ms deep into a long run -- the GPU's clock governor needs a few hundred
    milliseconds of load, and a training job is never that young.  ``--clock-warmup-ms 0`` switches it off.  Returns the
    number of steps it ran (the same on every rank: collectives are issued inside a step)."""
    if budget_s <= 0:
        return 0
    for _ in range(3):
        stepper.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        stepper.step()
    torch.cuda.synchronize()
    est = max((time.perf_counter() - t0) / 5, 1e-6)
    n = torch.tensor([max(0, min(5000, int(budget_s / est)))], dtype=torch.int64, device=stepper.device)
    if world > 1:
        dist.broadcast(n, src=0)
    n = int(n.item())
    for k in range(n):
        stepper.step()
        if k % 256 == 255:
            torch.cuda.synchronize()  # bound the launch queue
    torch.cuda.synchronize()
    return n


def timed_run(stepper, steps, warmup, world):
    """The driver's contract: W warm-up steps, then EXACTLY K steps between barrier + synchronize, max over ranks."""
    for _ in range(warmup):
        stepper.step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        stepper.step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=stepper.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed


def event_timed(fn, iters):
    """Each step individually bracketed by HIP events on the launch stream (torch's current stream is the stream the
    library launches on).  Returns milliseconds per step."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def timing_summary(stepper, iters):
    iters = max(50, int(iters))
    out = {"iters": iters}
    ms = sorted(event_timed(stepper.step, iters))
    out["launch_mode"] = "direct calls" if stepper.use_eager else "hipGraph replay"
    out["launch_probe_ms"] = stepper.launch_probe_ms
    out["timed_mode"] = {
        "median_ms": round(statistics.median(ms), 5), "p10_ms": round(ms[int(0.1 * (iters - 1))], 5),
        "p90_ms": round(ms[int(0.9 * (iters - 1))], 5)}
    return out


def profile_kernels(stepper, steps):
    from mutual_info_img_txt import _hip
    if stepper.eager_obj is None and not stepper.dist_mode:
        return {}
    stepper.eager_step()
    torch.cuda.synchronize()
    with _hip.kernel_profile() as prof:
        for _ in range(steps):
            stepper.eager_step()
    return prof.by_name()


# profiling-hook kernel name -> substring of the rocprofv3 kernel name in profiles/*_pmc_traffic.json
PMC_KERNEL_OF = {
    "bilinear prep + T = X W (bf16 in)": "bilinear_prep_t_kernel",
    "bilinear prep + T = X W": "bilinear_prep_t_kernel",
    "bilinear fused S | P Y | P^T T": "bilinear_flash_kernel",
    "bilinear sums -> dT, dY | dX = dT W^T": "flash_tail_kernel",
    "bilinear sums -> loss, dT, dY | dX = dT W^T": "flash_tail_kernel",
    "bilinear dW = X^T dT": "bilinear_dw_kernel",
    "bilinear dT = G Y | dY = G^T T": "gemm_bf16_pipe_kernel",
    "bilinear G": "gemm_bf16_big_kernel<mi::EpiGradScore2>",
    "bilinear score+LSE": "gemm_bf16_big_kernel<mi::EpiScoreLse2>",
    # concat-MLP critic: a regular expression on the rocprofv3 kernel name (demangled or mangled form) per precision mode
    "concat_fwd_kernel": {"bf16": r"concat_fwd_dma_kernel", "f16": r"concat_fwd_f16_kernel", "f16x3": r"concat_fwd_f16x3_kernel"},
    "concat_bwd_duv_kernel": {"bf16": r"concat_bwd_duv3_kernel(<__bf16|IDF16b)",
                              "f16": r"concat_bwd_duv3_kernel(<_Float16, _Float16|IDF16_DF16_)",
                              "f16x3": r"concat_bwd_duv3_kernel(<_Float16, float|IDF16_f)"},
    "concat_bwd_dw2_kernel": {"bf16": r"concat_bwd_dw2_kernel(<__bf16|IDF16b)", "f16": r"concat_bwd_dw2_f16_kernel",
                              "f16x3": r"concat_bwd_dw2_kernel(<_Float16|IDF16_)"},
    # fp8 mode (B = 8192, d = 1024): regular expressions; the (kernel, grid) keys of the PMC file keep the shapes apart
    "fp8 mode dT = G Y | dY = G^T T": {"fp8": r"gemm_bf16_big_kernel<mi::EpiScaled<mi::EpiStoreMulti>.*grid=\(?(65536|131072)"},
    "fp8 G": {"fp8": r"gemm_bf16_big_kernel<mi::EpiScaled<mi::EpiGradScore2>, true>"},
    "fp8 score+LSE": {"fp8": r"gemm_bf16_big_kernel<mi::EpiScaled<mi::EpiScoreLse2>, true>"},
}


def csrc_sha():
    """Fingerprint of the kernel sources: a committed PMC pass is only valid for the sources it profiled."""
    h = hashlib.sha1()
    for f in sorted(glob.glob(os.path.join(PKG, "csrc", "*.h")) + glob.glob(os.path.join(PKG, "csrc", "*.hip"))):
        with open(f, "rb") as fh:
            h.update(os.path.basename(f).encode() + b"\0" + fh.read())
    return h.hexdigest()[:12]


def measured_counters(name, b, d, mode="bf16"):
    """HBM bytes per launch and MFMA-busy fraction of a kernel from the newest committed PMC pass
    (tools/profile_round.sh: FETCH_SIZE, WRITE_SIZE and the SQ counters in separate rocprofv3 --pmc runs, gfx950
    corrections applied there).  bench.py cannot run the profiler itself; it REFUSES a pass whose recorded source
    fingerprint differs from the sources of this build (a stale pass would silently describe other kernels), and only
    accepts the configuration those passes ran (B=4096, d=512, one GPU)."""
    # (the PMC passes run bench.py's defaults: the headline at d = 512, the concat-MLP leg at d = 768)
    shape = (4096, 768) if name.startswith("concat") else ((8192, 1024) if name.startswith("fp8") else (4096, 512))
    if name not in PMC_KERNEL_OF or (b, d) != shape:
        return None
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic.json")))
    if not files:
        return None
    try:
        with open(files[-1]) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        return None
    src = os.path.basename(files[-1])
    if doc.get("csrc_sha") != csrc_sha():
        return {"stale": True, "source": src, "note": "PMC pass predates the current kernel sources: not attached"}
    import re
    want = PMC_KERNEL_OF[name]
    want = want.get(mode) if isinstance(want, dict) else re.escape(want)
    if not want:
        return None
    # several (kernel, grid) entries may match (the separable leg at B = 256 runs the same kernels as the headline): the
    # configurations this function accepts are the largest launches of their kernels in the passes
    hits = [val for key, val in doc.get("kernels", {}).items() if re.search(want, key)]
    if not hits:
        return None
    val = max(hits, key=lambda v: v["total_bytes"])
    return {"bytes": round(val["total_bytes"]), "fetch": round(val["fetch_bytes"]), "write": round(val["write_bytes"]),
            "mfma_busy_frac": val.get("mfma_busy_frac"), "source": src, "commit": doc.get("commit")}


def roofline_of(kernels, br, b, d, precision):
    if not kernels:
        return None
    name = max(kernels, key=lambda k: kernels[k]["ms_total"])
    k = kernels[name]
    fl = kernel_flops(name, br, b, d, d)
    if fl <= 0:
        return {"kernel": name, "bound": "hbm", "achieved": None, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": None,
                "traffic": None, "avg_us": k["ms_avg"] * 1e3}
    achieved = fl / (k["ms_avg"] * 1e-3) / 1e12
    peak = PEAK_TFLOPS[precision]
    c = measured_counters(name, b, d, precision) if br == b else None
    ok = c is not None and not c.get("stale")
    return {"kernel": name, "bound": "mfma", "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4), "traffic": c["bytes"] if ok else None,
            # achieved HBM-side rate of the same launch: counter bytes (committed PMC pass) / this run's event-timed duration
            "hbm_gbs": round(c["bytes"] / (k["ms_avg"] * 1e-3) / 1e9, 1) if ok else None, "hbm_peak_gbs": PEAK_HBM_GBS,
            "mfma_busy_frac": c.get("mfma_busy_frac") if ok else None, "counters": c,
            "avg_us": round(k["ms_avg"] * 1e3, 2), "flops_per_launch": fl}


def fp8_roofline(kernels, b, d):
    """fp8 mode: the dominant kernel of the step against the peak of the MFMA it runs -- the dense fp8 peak (5 PFLOP/s) for
    the kernels whose products are fp8 (score+LSE, G, T), the bf16 peak for the bf16 backward contractions."""
    if not kernels:
        return None
    name = max(kernels, key=lambda k: kernels[k]["ms_total"])
    k = kernels[name]
    two = "|" in name
    if name in ("fp8 score+LSE", "fp8 G") or two or name.startswith("fp8 mode dT") or name.startswith("fp8 mode dY"):
        fl = (4.0 if two else 2.0) * b * b * d
    elif name in ("fp8 T = X W", "fp8 mode dW = X^T dT", "fp8 mode dX = dT W^T"):
        fl = 2.0 * b * d * d
    else:
        fl = 0.0
    fp8_products = name in ("fp8 score+LSE", "fp8 G", "fp8 T = X W")
    peak = PEAK_TFLOPS["fp8"] if fp8_products else PEAK_TFLOPS["bf16"]
    if fl <= 0:
        return {"kernel": name, "bound": "hbm", "achieved": None, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": None,
                "traffic": None, "avg_us": round(k["ms_avg"] * 1e3, 2)}
    achieved = fl / (k["ms_avg"] * 1e-3) / 1e12
    c = measured_counters(name, b, d, "fp8")
    ok = c is not None and not c.get("stale")
    return {"kernel": name, "bound": "mfma", "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4), "traffic": c["bytes"] if ok else None,
            "hbm_gbs": round(c["bytes"] / (k["ms_avg"] * 1e-3) / 1e9, 1) if ok else None, "hbm_peak_gbs": PEAK_HBM_GBS,
            "mfma_busy_frac": c.get("mfma_busy_frac") if ok else None, "counters": c,
            "avg_us": round(k["ms_avg"] * 1e3, 2),
            "flops_per_launch": fl, "operands": "fp8 e4m3" if fp8_products else "bf16"}


def host_cpu_share(default_cap=16):
    """Threads for the CPU leg: the smallest of the affinity mask, the cgroup CPU quota and -- when neither restricts
    the process (a 1-GPU box of the pool shows all 256 hardware threads of its host but is granted 16; 256 BLAS threads
    there ran the oracle 14 x SLOWER than 16) -- `default_cap`.  MI_BENCH_CPU_THREADS overrides."""
    env = os.environ.get("MI_BENCH_CPU_THREADS")
    if env:
        return max(1, int(env))
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:  # cgroup v2: "<quota> <period>" or "max <period>"
            q, per = f.read().split()
            if q != "max":
                quota = max(1, int(int(q) / int(per)))
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                q, per = int(f.read()), int(g.read())
                if q > 0:
                    quota = max(1, q // per)
        except (OSError, ValueError):
            pass
    if quota is not None:
        return max(1, min(avail, quota))
    return max(1, min(avail, default_cap))


def cpu_baseline(kind, args, dim=None):
    """The oracle (a CPU port of the reference algorithm, pinned to the reference by tests/golden) timed on this box's
    host cores on a bounded sample of the same workload."""
    from oracle import mi_oracle as orc
    threads = host_cpu_share()
    torch.set_num_threads(threads)
    d = dim or args.dim
    if kind == "bilinear":
        b = args.batch
        gen = torch.Generator().manual_seed(3)
        x, y = torch.randn(b, d, generator=gen), torch.randn(b, d, generator=gen)
        w = torch.randn(d, d, generator=gen) / math.sqrt(d)
        sid = list(range(b))
        fn = lambda: orc.matrix_step(lambda a, c, ww: orc.bilinear_scores(a, c, ww), [x, y, w], sid, args.estimator)  # noqa: E731
        sample = f"full workload B={b} d={d} fp32, oracle matrix_step"
    else:
        b = min(args.batch, 256)  # the CPU needs ~4 s per step at B=256; larger B is infeasible in-budget
        x, y, sid, params = orc.synthetic_case(b, d, d, salt=1)
        fn = lambda: orc.concat_matrix_step(x, y, sid, params, args.estimator)  # noqa: E731
        sample = f"B={b} of {args.batch} (pairs/s falls further with B), d={d}, fp32, oracle concat_matrix_step"
    fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        el = time.perf_counter() - t0
        if el > args.cpu_seconds or n >= 200:
            break
    return {"value": round(b * n / el, 2), "unit": "pairs/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{sample}; {n} steps in {el:.1f} s"}


def main():
    args = parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        launch_ranks(args)  # does not return
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if world_env != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world_env}: launch with "
                         f"`python bench.py --gpus N` (starts its own ranks) or torch.distributed.run --nproc-per-node N "
                         f"bench.py --gpus N")
    if args.rendezvous_only:
        return rendezvous_only(args, world_env, int(os.environ.get("RANK", "0")))
    # The contract is ONE JSON line on stdout.  Libraries print there too (RCCL writes its version banner to stdout when
    # the first communicator is made): keep the real stdout aside and point fd 1 at stderr for the rest of the run.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the MI critic path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    group = None
    if world > 1 or os.environ.get("MI_BENCH_FORCE_DIST"):  # the latter: rehearse the RCCL path with one rank
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        group = dist.group.WORLD
    if args.batch % world:
        raise SystemExit("--batch must be divisible by the number of GPUs")
    from mutual_info_img_txt import _hip
    _hip.load()
    want_graph = args.graph in ("on", "auto", "full")
    b, d, br = args.batch, args.dim, args.batch // world

    def run(kind, steps, warmup, precision=None, timed_iters=0, batch=None, dim=None, clock_ms=None, cold_first=False,
            boundary="f32", probe=True, keep_outputs=False):
        st = Stepper(kind, args, rank, world, device, group, precision=precision, graph=want_graph and probe, batch=batch,
                     dim=dim, boundary=boundary)
        if args.graph == "auto" and probe:
            st.choose_launch_mode(world)
        # the contract's W + K steps from a young process first (no clock warm-up): `cold_ms_per_step`
        st.cold_elapsed = timed_run(st, steps, warmup, world) if cold_first else None
        st.clock_warmup_steps = clock_warmup(st, (args.clock_warmup_ms if clock_ms is None else clock_ms) * 1e-3, world)
        elapsed = timed_run(st, steps, warmup, world)
        st.outputs = st.host_outputs() if keep_outputs else None  # (after the timed region: the later steps overwrite them)
        timing = timing_summary(st, timed_iters) if timed_iters else None
        kernels = profile_kernels(st, args.profile_steps) if args.full else {}
        return st, elapsed, kernels, timing

    # the bf16 boundary exists for the bilinear critic in bf16 precision on one GPU (sharded runs gather fp32 rows)
    boundary = args.boundary if (args.critic == "bilinear" and args.precision == "bf16" and world == 1 and
                                 not os.environ.get("MI_BENCH_FORCE_DIST")) else "f32"
    st, elapsed, kernels, timing = run(args.critic, args.steps, args.warmup, timed_iters=args.timed_iters if args.full else 0,
                                       cold_first=args.full, boundary=boundary, keep_outputs=bool(args.dump_outputs))
    if args.dump_outputs and rank == 0:
        dump_outputs(st.outputs, args.dump_outputs)
    ms = elapsed / args.steps * 1e3
    flops = algorithmic_flops(args.critic, b, d, d)
    graph_mode = "none (direct C-ABI calls)" if st.use_eager else \
        ("one graph: kernels + the five RCCL collectives" if st.dist_mode and args.graph == "full" else
         "compute sections; collectives eager between them" if st.dist_mode else "one graph: forward + backward")
    out = {
        "metric": "img-txt pairs/sec (MI critic fwd+bwd), global-batch InfoNCE",
        "value": round(b / (ms * 1e-3), 1),
        "unit": "pairs/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms, 5),
        "warmup_effective_steps": args.warmup + st.clock_warmup_steps,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": args.precision,
        "data": "synthetic",
        "config": {"workload": f"BASELINE configs[3]: global-batch {args.estimator} (reference semantics), "
                               f"{args.critic} critic fwd+bwd, B_global={b}, d={d}",
                   "global_batch": b, "embed_dim": d, "critic": args.critic, "estimator": args.estimator,
                   "parallelism": f"row-block sharding x{world}, RCCL all-gather of text embeddings" if world > 1 else "single GPU",
                   "boundary": ("bf16 embeddings in, bf16 dX / dY out (mi_bilinear_step_bf16); W, dW, loss fp32" if boundary == "bf16"
                                else "fp32 embeddings in, fp32 gradients out"),
                   "hip_graph": not st.use_eager, "graph_mode": graph_mode},
        "loss": st.loss(),
        "timing": dict(timing or {}, clock_warmup={"budget_ms": args.clock_warmup_ms, "untimed_steps": st.clock_warmup_steps,
                                                   "note": "`ms_per_step`: untimed steps for budget_ms before the W warm-up "
                                                           "steps (sustained-run clocks; the same budget for every leg of "
                                                           "this line)" + ("; `cold_ms_per_step`: the same W + K steps "
                                                                           "taken first, without them" if args.full else "")}),
        "step_algorithmic_tflops": round(flops / (ms * 1e-3) / 1e12, 2),
        "step_frac_of_peak": round(flops / (ms * 1e-3) / 1e12 / (PEAK_TFLOPS[args.precision] * world), 5),
    }
    if args.full:
        out["cold_ms_per_step"] = round(st.cold_elapsed / args.steps * 1e3, 5)
        out["roofline"] = roofline_of(kernels, br, b, d, args.precision)
        out["kernels_us"] = {k: round(v["ms_avg"] * 1e3, 2) for k, v in sorted(kernels.items(), key=lambda kv: -kv[1]["ms_total"])}
    del st
    torch.cuda.empty_cache()
    if args.full and args.critic == "bilinear" and args.precision == "bf16" and world == 1 and \
            not os.environ.get("MI_BENCH_FORCE_DIST"):
        # the same step on the same values through the other boundary (measured round 4: the bf16 boundary moves 25 MB less
        # per step and is NOT faster -- the conversion launch is bound by its chain of dependent k-steps, not by bytes)
        other = "f32" if boundary == "bf16" else "bf16"
        try:
            stf, elf, kf, _ = run(args.critic, args.steps, args.warmup, cold_first=True, boundary=other)
            msf = elf / args.steps * 1e3
            out["other_boundary"] = {
                "boundary": "bf16 embeddings in, bf16 dX / dY out (mi_bilinear_step_bf16)" if other == "bf16"
                            else "fp32 embeddings in, fp32 gradients out (mi_bilinear_step)",
                "ms_per_step": round(msf, 5), "cold_ms_per_step": round(stf.cold_elapsed / args.steps * 1e3, 5),
                "value": round(b / (msf * 1e-3), 1), "unit": "pairs/s", "loss": stf.loss(),
                "step_frac_of_peak": round(flops / (msf * 1e-3) / 1e12 / (PEAK_TFLOPS[args.precision] * world), 5),
                "kernels_us": {k: round(v["ms_avg"] * 1e3, 2) for k, v in sorted(kf.items(), key=lambda kv: -kv[1]["ms_total"])},
                "note": "bit-identical loss, statistics and dW on the same bf16-representable values "
                        "(tests/test_graphed_step.py::test_bf16_boundary_equals_fp32_boundary)"}
            del stf
        except Exception as e:
            out["other_boundary"] = {"error": f"{type(e).__name__}: {e}"}
        torch.cuda.empty_cache()
    if args.full and not args.no_parity_mode and args.precision not in ("f32", "f32_exact"):
        # the same step in the mode whose results match the fp32 reference
        out["parity_mode"] = {}
        exact = "f32_exact" if args.critic == "bilinear" else "f32"  # "f32" on the bilinear critic resolves to bf16x3
        notes = {exact: "v_mfma_f32_32x32x2_f32: exact fp32 products (precision=\"f32_exact\" on the bilinear critic; "
                        "\"f32\" on the concat-MLP critic)",
                 "bf16x3": "two-part bf16 operands, three bf16 MFMAs per product (K tripled), fp32 accumulate: held to the "
                           "fp32 tolerances of DESIGN.md section 2 (tests/test_parity_configs.py); what precision=\"f32\" "
                           "runs on the bilinear critic"}
        for mode in ([exact, "bf16x3"] if args.critic == "bilinear" and world == 1 else [exact]):
            try:
                n2 = max(3, args.steps // 10)
                st2, el2, k2, _ = run(args.critic, n2, 2, precision=mode)
                ms2 = el2 / n2 * 1e3
                out["parity_mode"][mode] = {
                    "ms_per_step": round(ms2, 4), "value": round(b / (ms2 * 1e-3), 1), "unit": "pairs/s",
                    "step_frac_of_peak": round(flops / (ms2 * 1e-3) / 1e12 / (PEAK_TFLOPS[mode] * world), 5),
                    "peak": round(PEAK_TFLOPS[mode], 1), "loss": st2.loss(), "note": notes[mode]}
                del st2
            except Exception as e:
                out["parity_mode"][mode] = {"error": f"{type(e).__name__}: {e}"}
            torch.cuda.empty_cache()
        torch.cuda.empty_cache()
    if args.full and not args.no_fp8 and args.critic == "bilinear" and world == 1:
        # BASELINE configs[4] on ONE GPU (the whole 8192 x 8192 score matrix, not a rank's 1024-row share)
        try:
            b8, d8, n8 = 8192, 1024, max(3, args.steps // 10)
            st4, el4, k4, _ = run("bilinear", n8, 2, precision="fp8", batch=b8, dim=d8)
            ms4 = el4 / n8 * 1e3
            fl4 = algorithmic_flops("bilinear", b8, d8, d8)
            out["fp8_mode"] = {
                "workload": f"BASELINE configs[4] on one GPU: fp8 (e4m3, per-tensor scale absmax / 448) bilinear critic "
                            f"fwd+bwd, B={b8}, d={d8}; forward products on v_mfma_scale_f32_32x32x64_f8f6f4 (unit block scales), backward on bf16 MFMA",
                "value": round(b8 / (ms4 * 1e-3), 1), "unit": "pairs/s", "ms_per_step": round(ms4, 4), "steps": n8,
                "loss": st4.loss(), "step_algorithmic_tflops": round(fl4 / (ms4 * 1e-3) / 1e12, 2),
                "step_frac_of_peak": round(fl4 / (ms4 * 1e-3) / 1e12 / PEAK_TFLOPS["fp8"], 5),
                "roofline": fp8_roofline(k4, b8, d8),
                "kernels_us": {k: round(v["ms_avg"] * 1e3, 2) for k, v in sorted(k4.items(), key=lambda kv: -kv[1]["ms_total"])}}
            del st4
        except Exception as e:
            out["fp8_mode"] = {"error": f"{type(e).__name__}: {e}"}
        torch.cuda.empty_cache()
    if args.full and not args.no_fp8 and args.critic == "bilinear" and world == 1:
        # BASELINE configs[1]: InfoNCE separable critic S = (X Wg)(Y Wh)^T, 256-d, batch 256, bf16, one GPU
        try:
            bs, ds, ns = 256, 256, max(20, args.steps)
            st5, el5, k5, _ = run("separable", ns, 5, precision="bf16", batch=bs, dim=ds)
            ms5 = el5 / ns * 1e3
            fl5 = algorithmic_flops("separable", bs, ds, ds)
            out["separable_mode"] = {
                "workload": f"BASELINE configs[1]: separable critic fwd+bwd (projections included), B={bs}, d={ds}, d_proj={ds}, bf16",
                "value": round(bs / (ms5 * 1e-3), 1), "unit": "pairs/s", "ms_per_step": round(ms5, 4), "steps": ns,
                "hip_graph": not st5.use_eager, "loss": st5.loss(),
                "step_algorithmic_tflops": round(fl5 / (ms5 * 1e-3) / 1e12, 2),
                "note": "0.3 GFLOP per step: launch- and latency-bound at this size, not a roofline case",
                "kernels_us": {k: round(v["ms_avg"] * 1e3, 2) for k, v in sorted(k5.items(), key=lambda kv: -kv[1]["ms_total"])}}
            del st5
        except Exception as e:
            out["separable_mode"] = {"error": f"{type(e).__name__}: {e}"}
        torch.cuda.empty_cache()
    if args.full and not args.no_secondary:
        other = "concat_mlp" if args.critic == "bilinear" else "bilinear"
        # the concat-MLP leg runs at the reference's own embedding width (768 per modality)
        d2 = 768 if other == "concat_mlp" else d
        fl3 = algorithmic_flops(other, b, d2, d2)

        def leg(mode, n):
            # (steps of tens to hundreds of milliseconds: direct calls, no launch-mode probe, a short clock warm-up)
            st3, el3, k3, _ = run(other, n, 1, precision=mode, dim=d2, probe=False, clock_ms=min(args.clock_warmup_ms, 100.0))
            ms3 = el3 / n * 1e3
            peak_key = "f16x3" if (other == "concat_mlp" and mode == "f32") else mode
            peak = PEAK_TFLOPS[peak_key] * world
            res = {"precision": mode, "value": round(b / (ms3 * 1e-3), 1), "unit": "pairs/s", "ms_per_step": round(ms3, 4),
                   "steps": n, "hip_graph": not st3.use_eager, "loss": st3.loss(),
                   "step_algorithmic_tflops": round(fl3 / (ms3 * 1e-3) / 1e12, 2),
                   "step_frac_of_peak": round(fl3 / (ms3 * 1e-3) / 1e12 / peak, 5), "peak": round(peak, 1),
                   "roofline": roofline_of(k3, br, b, d2, peak_key),
                   "kernels_us": {k: round(v["ms_avg"] * 1e3, 2) for k, v in sorted(k3.items(), key=lambda kv: -kv[1]["ms_total"])}}
            del st3
            torch.cuda.empty_cache()
            return res
        try:
            fast = SECONDARY_FAST.get(other, [args.precision])
            out["secondary"] = dict(leg(fast[0], args.secondary_steps),
                                    workload=f"{other} critic fwd+bwd, B_global={b}, d={d2}" +
                                    (" (the reference's mi_discriminator, make_mlp(1536,[1024,512]))" if other == "concat_mlp" else ""))
            for mode in fast[1:]:
                try:
                    out["secondary"].setdefault("other_fast_modes", {})[mode] = leg(mode, args.secondary_steps)
                except Exception as e:
                    out["secondary"].setdefault("other_fast_modes", {})[mode] = {"error": f"{type(e).__name__}: {e}"}
            if not args.no_parity_mode and other == "concat_mlp":
                # the reference's critic in the modes held to the fp32 tolerances
                out["secondary"]["parity_mode"] = {}
                for mode in SECONDARY_PARITY:
                    try:
                        out["secondary"]["parity_mode"][mode] = leg(mode, 3)
                    except Exception as e:
                        out["secondary"]["parity_mode"][mode] = {"error": f"{type(e).__name__}: {e}"}
        except Exception as e:
            out["secondary"] = {"error": f"{type(e).__name__}: {e}"}
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args.critic, args)
        if "secondary" in out and "error" not in out["secondary"]:
            other = "concat_mlp" if args.critic == "bilinear" else "bilinear"
            out["secondary"]["cpu_baseline"] = cpu_baseline(other, args, dim=768 if other == "concat_mlp" else None)
    if rank == 0:  # the line first: a tear-down problem must not cost the measurement
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if dist.is_initialized():  # several ranks, or the one-rank rehearsal of the RCCL path (MI_BENCH_FORCE_DIST)
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
