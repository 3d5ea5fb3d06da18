"""Child process of tests/test_prep_t_forms_gpu.py: one step of the bilinear critic per shape of CASES (and one of the
separable critic) through the one-call entry points, every output saved to the .npz named on the command line.  A child
because the library reads MI_PREP_T_TALL once, on its first prep launch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mutual-information-multimodal_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mutual_info_img_txt.graphed import GraphedMiStep  # noqa: E402
from mutual_info_img_txt.model import BilinearCritic, SeparableCritic  # noqa: E402

# (B, d_img, d_txt): B = 128 is two 64-row tiles of one panel, 384 an odd number of 128-row panels (the grid's XCD padding);
# d_img = 64 is one k-step with one X^T writer, 192 three k-steps (the writers' round-robin has a remainder), 512 eight;
# d_txt = 128 is one column tile, which then writes every k-step, 512 four
CASES = [(b, dx, dy) for b in (128, 384) for dx in (64, 192, 512) for dy in (128, 512)]
POISONED = (384, 192, 512)   # once more on a workspace of NaN bit patterns: an X^T block nobody wrote would show
SEPARABLE = (128, 64, 96, 128)  # (B, d_img, d_txt, d_proj): a caller that keeps the 128-row form and its conversion jobs


def one_step(critic, b, dx, dy, dev, poison=False):
    gen = torch.Generator().manual_seed(11 + b + dx + dy)
    x, y = torch.randn(b, dx, generator=gen), torch.randn(b, dy, generator=gen)
    sid = torch.arange(b, dtype=torch.int64)
    sid[9] = sid[8]  # repeated study ids: next to each other, across 32-row blocks, across 64-row tiles
    sid[70] = sid[5]
    sid[b - 1] = sid[0]
    step = GraphedMiStep(critic, b, dx, dy, "infonce", "bf16", dev, capture=False)
    step.set_inputs(x.to(dev), y.to(dev), sid.to(dev))
    step.stats.zero_()  # (torch.empty: padding bytes the library never writes)
    if poison:
        step.ws.fill_(0xFF)  # bf16 0xFFFF and fp32 0xFFFFFFFF are NaNs
    step._step()
    torch.cuda.synchronize()
    out = {"path": np.array([-1 if step.path is None else step.path]), "loss": step.loss_buf.cpu().numpy(),
           "stats": step.stats.cpu().numpy(), "grad_x": step.grad_x.cpu().numpy(), "grad_y": step.grad_y.cpu().numpy()}
    for i, g in enumerate(step.grad_params):
        out[f"grad_param{i}"] = g.cpu().numpy()
    return out


def run(out_path: str) -> None:
    dev = torch.device("cuda:0")
    out = {}
    for b, dx, dy in CASES:
        torch.manual_seed(7)
        critic = BilinearCritic(dx, dy).to(dev)
        for k, v in one_step(critic, b, dx, dy, dev).items():
            out[f"b{b}_{dx}_{dy}/{k}"] = v
        if (b, dx, dy) == POISONED:
            for k, v in one_step(critic, b, dx, dy, dev, poison=True).items():
                out[f"poisoned/{k}"] = v
    b, dx, dy, dp = SEPARABLE
    torch.manual_seed(7)
    for k, v in one_step(SeparableCritic(dx, dy, dp).to(dev), b, dx, dy, dev).items():
        out[f"separable/{k}"] = v
    np.savez(out_path, **out)
    print("prep t forms worker ok")


if __name__ == "__main__":
    run(sys.argv[1])
