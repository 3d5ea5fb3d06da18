"""The study-positive and the soft-target InfoNCE over a sharded global batch on the product's HIP ops: two and three
ranks sharing the box's one GPU over gloo (tests/posnce_softnce_shard_gpu_worker.py).  One world at a time: at most three
processes open the GPU, this process opens none.  Nothing is retried; when a worker fails or runs out of time the others
are killed."""
import os
import socket
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = {2: 14, 3: 8}  # cases per world in the worker
TIMEOUT = 600


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_losses_ranks_one_gpu_over_gloo(world):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "posnce_softnce_shard_gpu_worker.py")],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [""] * world
    deadline = time.monotonic() + TIMEOUT
    try:
        # a worker that failed leaves the others waiting in a collective: find it first, then end them
        pending = set(range(world))
        while pending:
            for rank in sorted(pending):
                try:
                    outs[rank], _ = procs[rank].communicate(timeout=max(0.1, min(1.0, deadline - time.monotonic())))
                except subprocess.TimeoutExpired:
                    continue
                pending.discard(rank)
                if procs[rank].returncode != 0:
                    pending.clear()
                    break
            if time.monotonic() >= deadline:
                break
    finally:
        for rank, p in enumerate(procs):
            if p.poll() is None:
                p.kill()
                outs[rank] = (outs[rank] or "") + (p.communicate()[0] or "")
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {rank} (exit {p.returncode}):\n{out[-4000:]}"
    print(outs[0])  # the "shard-err <what> <error / tolerance>" figures of rank 0 (pytest -s shows them)
    assert outs[0].count("posnce softnce shard gpu ok") == EXPECTED[world], outs[0][-3000:]
