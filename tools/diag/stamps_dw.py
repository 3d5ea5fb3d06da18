"""Diagnostic: s_memtime stamps of the dW = X^T dT launch of the headline step (needs lib_stamps/, make STAMPS=1;
MI_CRITIC_LIB names another stamps build, MI_DW_XCD_NATURAL selects the tile order as in any run).
Slots (wave 0 of every workgroup): 0 entry, 1 first operand loads issued, 2 first MFMA issued, 3 last MFMA issued,
4 the tile's stores issued.  s_memtime is compared within one workgroup only (the counters of different XCDs are far
apart): every figure is a difference of two stamps of the same workgroup, in shader cycles."""
import os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
os.environ.setdefault("MI_CRITIC_LIB", os.path.join(ROOT, "mutual-information-multimodal_amd", "lib_stamps", "libmi_critic_hip.so"))
os.environ["MI_STAMP_KERNEL"] = "bilinear dW"
sys.path.insert(0, os.path.join(ROOT, "mutual-information-multimodal_amd"))
sys.path.insert(0, ROOT)
import ctypes
import numpy as np
import torch
from mutual_info_img_txt import mi_critics, _hip
from mutual_info_img_txt.model import BilinearCritic

dev = torch.device("cuda:0")
b, d = 4096, 512
x = torch.randn(b, d, device=dev, requires_grad=True)
y = torch.randn(b, d, device=dev, requires_grad=True)
sid = torch.arange(b, device=dev)
critic = BilinearCritic(d, d).to(dev)
lib = _hip.load()
lib.mi_debug_set_stamps.argtypes = [ctypes.c_void_p]
buf = torch.zeros(8192 * 8, dtype=torch.int64, device=dev)
lib.mi_debug_set_stamps(buf.data_ptr())

def step():
    loss = mi_critics.fused_mi_bound(x, y, sid, critic, "infonce", precision="bf16")
    loss.sum().backward()

for _ in range(5): step()
torch.cuda.synchronize()
rows = []
for _ in range(5):  # five stamped steps: the medians below are over all their workgroups
    buf.zero_()
    step()
    torch.cuda.synchronize()
    s = buf.cpu().numpy().reshape(-1, 8)
    rows.append(s[(s[:, 0] != 0) & (s[:, 4] != 0)][:, :5])
print("library:", os.environ["MI_CRITIC_LIB"], " MI_DW_XCD_NATURAL =", os.environ.get("MI_DW_XCD_NATURAL"))
print("workgroups stamped per step:", [len(r) for r in rows])
S = np.concatenate(rows)
for i, n in enumerate(["entry -> first loads issued", "first loads -> first MFMA", "first MFMA -> last MFMA", "last MFMA -> tile stored"]):
    dlt = S[:, i + 1] - S[:, i]
    print(f"   {n:28s} median {np.median(dlt):8.0f}  p10 {np.percentile(dlt, 10):8.0f}  p90 {np.percentile(dlt, 90):8.0f}  max {dlt.max():8.0f}")
whole = S[:, 4] - S[:, 0]
print(f"   {'whole workgroup':28s} median {np.median(whole):8.0f}  p10 {np.percentile(whole, 10):8.0f}  p90 {np.percentile(whole, 90):8.0f}  max {whole.max():8.0f}")
