"""Child process of tests/test_dw_xcd_order_gpu.py: one step of the bilinear critic (B = 4096, d = 512) and one of the
separable critic (B = 256, d = 256) through the one-call entry points, every output saved to the .npz named on the command
line.  A child because the library reads MI_DW_XCD_NATURAL once, on its first dW launch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mutual-information-multimodal_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mutual_info_img_txt.graphed import GraphedMiStep  # noqa: E402
from mutual_info_img_txt.model import BilinearCritic, SeparableCritic  # noqa: E402


def run(out_path: str) -> None:
    dev = torch.device("cuda:0")
    out = {}
    for kind, b, d in (("bilinear", 4096, 512), ("separable", 256, 256)):
        torch.manual_seed(7)
        critic = (BilinearCritic(d, d) if kind == "bilinear" else SeparableCritic(d, d, d)).to(dev)
        gen = torch.Generator().manual_seed(11)
        x, y = torch.randn(b, d, generator=gen), torch.randn(b, d, generator=gen)
        sid = torch.arange(b, dtype=torch.int64)
        sid[9] = sid[8]
        step = GraphedMiStep(critic, b, d, d, "infonce", "bf16", dev, capture=False)
        step.set_inputs(x.to(dev), y.to(dev), sid.to(dev))
        step._step()
        torch.cuda.synchronize()
        out[f"{kind}_path"] = np.array([-1 if step.path is None else step.path])
        out[f"{kind}_loss"] = step.loss_buf.cpu().numpy()
        out[f"{kind}_grad_x"] = step.grad_x.cpu().numpy()
        out[f"{kind}_grad_y"] = step.grad_y.cpu().numpy()
        for i, g in enumerate(step.grad_params):
            out[f"{kind}_grad_param{i}"] = g.cpu().numpy()
    np.savez(out_path, **out)
    print("dw order worker ok")


if __name__ == "__main__":
    run(sys.argv[1])
