"""Child process of tests/test_prep_lds_layout_gpu.py: one step of the bilinear critic per shape of PREP_CASES and
DW_CASES, one of the separable critic per shape of DW_SEPARABLE, through the one-call entry points; every output and
every input (for the float64 oracle in the parent) saved to the .npz named on the command line.  A child because the library reads
MI_PREP_T_TALL and MI_DW_XCD_NATURAL once, on its first prep / dW launch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mutual-information-multimodal_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mutual_info_img_txt.graphed import GraphedMiStep  # noqa: E402
from mutual_info_img_txt.model import BilinearCritic, SeparableCritic  # noqa: E402

# (B, d_img, d_txt) for the W image of the prep launch's T role: d_img = 64 / 128 / 192 / 512 is one, two, three and eight
# k-steps of 64 rows (the swizzle of the image repeats every 4 rows: every step wraps it 16 times, both buffers are in use
# from two steps on); d_txt = 128 .. 512 is one to four column tiles; B = 128 / 256 / 384 is 2 / 4 / 6 of the 64-row tiles,
# each leaving XCD rounds of the grid unfilled
# (d_txt = 384 is no width of the fused B x B kernel -- 128 / 256 / 512 are: that step runs the G-materialising plan, whose
# prep launch keeps the 128-row tiles; (256, 192, 256) beside it is the three-k-step case on the fused plan)
PREP_CASES = [(128, 64, 128), (128, 128, 256), (256, 192, 384), (256, 192, 256), (384, 512, 512), (128, 512, 128)]
PREP_POISONED = (384, 512, 512)  # once more on a workspace of 0xFF bytes (NaNs as bf16 and as fp32)
# dW: d_img / 32 = 1, 3, 5 tile rows -- no multiple of 4, the natural-order fallback of the tile decode
DW_CASES = [(128, 32, 128), (128, 96, 128), (128, 160, 256)]
# (B, d_img, d_txt, d_proj): two products in one dW launch; 2 x 4 + 3 x 4 and 3 x 4 + 2 x 4 tiles -- the second problem
# behind 8 and behind 12 tiles of the first (12 % 8 != 0: no XCD blocks for it)
DW_SEPARABLE = [(128, 64, 96, 128), (128, 96, 64, 128)]


def one_step(critic, b, dx, dy, dev, poison=False, keep_inputs=False):
    gen = torch.Generator().manual_seed(23 + b + dx + 3 * dy)
    x, y = torch.randn(b, dx, generator=gen), torch.randn(b, dy, generator=gen)
    sid = torch.arange(b, dtype=torch.int64)
    sid[9] = sid[8]  # repeated study ids: next to each other, across 32-row blocks, across 64-row tiles
    sid[70] = sid[5]
    sid[b - 1] = sid[0]
    step = GraphedMiStep(critic, b, dx, dy, "infonce", "bf16", dev, capture=False)
    step.set_inputs(x.to(dev), y.to(dev), sid.to(dev))
    step.stats.zero_()  # (torch.empty: padding bytes the library never writes)
    if poison:
        step.ws.fill_(0xFF)
    step._step()
    torch.cuda.synchronize()
    out = {"path": np.array([-1 if step.path is None else step.path]), "loss": step.loss_buf.cpu().numpy(),
           "stats": step.stats.cpu().numpy(), "grad_x": step.grad_x.cpu().numpy(), "grad_y": step.grad_y.cpu().numpy()}
    for i, g in enumerate(step.grad_params):
        out[f"grad_param{i}"] = g.cpu().numpy()
    if keep_inputs:
        out.update(x=x.numpy(), y=y.numpy(), sid=sid.numpy())
        for i, p in enumerate(critic.parameters()):
            out[f"param{i}"] = p.detach().cpu().numpy()
    return out


def run(out_path: str) -> None:
    dev = torch.device("cuda:0")
    out = {}
    for b, dx, dy in PREP_CASES:
        torch.manual_seed(7)
        critic = BilinearCritic(dx, dy).to(dev)
        for k, v in one_step(critic, b, dx, dy, dev, keep_inputs=True).items():
            out[f"prep{b}_{dx}_{dy}/{k}"] = v
        if (b, dx, dy) == PREP_POISONED:
            for k, v in one_step(critic, b, dx, dy, dev, poison=True).items():
                out[f"poisoned/{k}"] = v
    for b, dx, dy in DW_CASES:
        torch.manual_seed(7)
        critic = BilinearCritic(dx, dy).to(dev)
        for k, v in one_step(critic, b, dx, dy, dev, keep_inputs=True).items():
            out[f"dw{b}_{dx}_{dy}/{k}"] = v
    for b, dx, dy, dp in DW_SEPARABLE:
        torch.manual_seed(7)
        critic = SeparableCritic(dx, dy, dp).to(dev)
        for k, v in one_step(critic, b, dx, dy, dev, keep_inputs=True).items():
            out[f"sep{b}_{dx}_{dy}_{dp}/{k}"] = v
    np.savez(out_path, **out)
    print("side launch worker ok")


if __name__ == "__main__":
    run(sys.argv[1])
