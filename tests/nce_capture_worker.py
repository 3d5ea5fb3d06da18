"""Child process of tests/test_nce_gpu.py::test_graph_capture_replay: the per-sample InfoNCE step (fused_mi_bound forward
+ loss.backward(), bilinear critic) captured into a hipGraph with PyTorch's whole-network recipe (see capture_worker.py),
replayed on new inputs and compared with the eager result.  A capture only succeeds when the call neither synchronises
nor allocates outside torch's graph pool.  Run in a child because a capture that goes wrong aborts the process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mutual-information-multimodal_amd"))

import torch  # noqa: E402

from mutual_info_img_txt import mi_critics  # noqa: E402
from mutual_info_img_txt.model import BilinearCritic  # noqa: E402


def run(precision: str) -> None:
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    b, d = 256, 128
    critic = BilinearCritic(d, d).to(dev)
    sid = torch.arange(b, dtype=torch.int64)
    sid[5] = sid[4]
    sid = sid.to(dev)  # a device tensor: a host list would be copied inside the capture
    sx = torch.randn(b, d, device=dev, requires_grad=True)
    sy = torch.randn(b, d, device=dev, requires_grad=True)
    leaves = [sx, sy, critic.weight]

    def step():
        loss = mi_critics.fused_mi_bound(sx, sy, sid, critic, "infonce_symmetric", precision=precision)
        loss.backward()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            for t in leaves:
                t.grad = None
            step()
    torch.cuda.current_stream().wait_stream(side)
    for t in leaves:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = step()
    static_grads = [t.grad for t in leaves]

    for trial in range(2):
        nx, ny = torch.randn(b, d, device=dev), torch.randn(b, d, device=dev)
        with torch.no_grad():
            sx.copy_(nx)
            sy.copy_(ny)
        graph.replay()
        torch.cuda.synchronize()
        replay = [static_loss.detach().clone()] + [g.detach().clone() for g in static_grads]
        ex, ey = nx.clone().requires_grad_(True), ny.clone().requires_grad_(True)
        w = critic.weight.detach().clone().requires_grad_(True)
        eager_critic = BilinearCritic(d, d).to(dev)
        with torch.no_grad():
            eager_critic.weight.copy_(w)
        loss = mi_critics.fused_mi_bound(ex, ey, sid, eager_critic, "infonce_symmetric", precision=precision)
        loss.backward()
        torch.cuda.synchronize()
        eager = [loss.detach(), ex.grad, ey.grad, eager_critic.weight.grad]
        for n, (a, e) in enumerate(zip(replay, eager)):
            if not torch.equal(a, e):
                print(f"trial {trial}: output {n} differs by {float((a - e).abs().max())}")
                sys.exit(1)
    print("capture ok")


if __name__ == "__main__":
    run(sys.argv[1])
