"""Diagnostic: s_memtime stamps of the fused conversion + T = X W launch (needs lib_stamps/, make STAMPS=1; MI_CRITIC_LIB
names another stamps build, MI_PREP_T_TALL selects the form as in any run).
Slots: 0 entry, 1 first tile in LDS, 2 first k-step's MFMAs issued, 3 first k-step's barrier passed, 4 loop end, 5 block end,
6 where the workgroup ran and what it did: (role << 40) | (XCC_ID << 32) | HW_ID, role 0 = T tile, q + 1 = conversion job q."""
import os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
os.environ.setdefault("MI_CRITIC_LIB", os.path.join(ROOT, "mutual-information-multimodal_amd", "lib_stamps", "libmi_critic_hip.so"))
os.environ["MI_STAMP_KERNEL"] = "bilinear prep + T"
sys.path.insert(0, os.path.join(ROOT, "mutual-information-multimodal_amd"))
sys.path.insert(0, ROOT)
import collections
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
buf.zero_()
step()
torch.cuda.synchronize()
s = buf.cpu().numpy().reshape(-1, 8)
live = s[:, 0] != 0
is_t = live & (s[:, 1] != 0)              # only the T role stamps slot 1
is_c = live & ~is_t & (s[:, 5] != 0)      # (the flag blocks stamp slot 0 alone)
t0 = s[live, 0].min()
T, C = s[is_t], s[is_c]
print("library:", os.environ["MI_CRITIC_LIB"], " MI_PREP_T_TALL =", os.environ.get("MI_PREP_T_TALL"))
print("blocks stamped:", int(live.sum()), "T tiles:", len(T), "conversion blocks:", len(C))
print(f"kernel span: {s[live, 5].max() - t0} cycles")
print(f"T tiles : start median {np.median(T[:,0]-t0):.0f} max {np.max(T[:,0]-t0):.0f};  end median {np.median(T[:,5]-t0):.0f} max {np.max(T[:,5]-t0):.0f}")
for i, n in enumerate(["entry -> first tile in LDS", "first k-step MFMAs", "first k-step store+barrier", "remaining k-steps", "epilogue"]):
    dlt = T[:, i + 1] - T[:, i]
    print(f"   {n:28s} median {np.median(dlt):8.0f}  p10 {np.percentile(dlt,10):8.0f}  p90 {np.percentile(dlt,90):8.0f}")
print(f"   {'whole tile':28s} median {np.median(T[:,5]-T[:,0]):8.0f}  p10 {np.percentile(T[:,5]-T[:,0],10):8.0f}  p90 {np.percentile(T[:,5]-T[:,0],90):8.0f}")
dur = C[:, 5] - C[:, 0]
print(f"conversion blocks: duration median {np.median(dur):.0f} p90 {np.percentile(dur,90):.0f};  start median {np.median(C[:,0]-t0):.0f} p90 {np.percentile(C[:,0]-t0,90):.0f} max {np.max(C[:,0]-t0):.0f};  last end {np.max(C[:,5]-t0):.0f}")
hist, edges = np.histogram(C[:, 0] - t0, bins=8)
print("conversion block start histogram:", list(zip(edges[:-1].astype(int).tolist(), hist.tolist())))

# ---- the per-CU view (slot 6).  s_memtime is compared within one CU only (the counters of different XCDs are far apart,
# and blocks of one XCD were seen 1e8 cycles apart): every time below is taken from the first entry stamp on the block's CU.
def place(rows):
    p = rows[:, 6]
    hw = p & 0xFFFFFFFF
    xcc = (p >> 32) & 0xF
    cu = (xcc << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 0xF)  # XCC, SE, SH, CU
    return xcc, cu, (p >> 40) & 0xFF
t_xcc, t_cu, _ = place(T)
c_xcc, c_cu, c_job = place(C)
cu_t0 = {}
for c, e in zip(t_cu.tolist() + c_cu.tolist(), T[:, 0].tolist() + C[:, 0].tolist()):
    cu_t0[c] = min(cu_t0.get(c, e), e)
xcd_t0 = set(t_xcc.tolist()) | set(c_xcc.tolist())
t_rel = np.array([cu_t0[c] for c in t_cu.tolist()])
c_rel = np.array([cu_t0[c] for c in c_cu.tolist()])
tiles_on = collections.Counter(t_cu.tolist())
cvt_on = collections.Counter(c_cu.tolist())
cus = sorted(set(tiles_on) | set(cvt_on))
print(f"CUs seen: {len(cus)} on {len(xcd_t0)} XCDs;  T tiles per CU: {sorted(collections.Counter(tiles_on[c] for c in cus).items())}")
for name, sel in (("CUs with a T tile", [c for c in cus if tiles_on[c]]), ("CUs without one", [c for c in cus if not tiles_on[c]])):
    n = np.array([cvt_on[c] for c in sel]) if sel else np.zeros(1)
    print(f"   conversion blocks per CU, {name:18s} ({len(sel):3d}): min {n.min():.0f} median {np.median(n):.0f} max {n.max():.0f} total {n.sum():.0f}")
shares = np.array([tiles_on[c] > 0 for c in c_cu.tolist()])
for job in sorted(set(c_job.tolist())):
    for sh in (True, False):
        m = (c_job == job) & (shares == sh)
        if m.any():
            print(f"   conversion job {job - 1} ({'beside a T tile' if sh else 'CU without tile '}): {int(m.sum()):4d} blocks, duration median "
                  f"{np.median(dur[m]):6.0f} p90 {np.percentile(dur[m], 90):6.0f}")
t_end_cu = {}
for c, e in zip(t_cu.tolist(), (T[:, 5] - t_rel).tolist()):
    t_end_cu[c] = max(t_end_cu.get(c, 0), e)
c_end_cu = {}
for c, e in zip(c_cu.tolist(), (C[:, 5] - c_rel).tolist()):
    c_end_cu[c] = max(c_end_cu.get(c, 0), e)
te, ce = np.array(list(t_end_cu.values())), np.array(list(c_end_cu.values()))
print(f"end of the T role per CU (from the CU's first entry):           median {np.median(te):.0f} p90 {np.percentile(te, 90):.0f} max {te.max():.0f}")
print(f"end of the conversion role per CU (last block):                 median {np.median(ce):.0f} p90 {np.percentile(ce, 90):.0f} max {ce.max():.0f}")
both = [c for c in t_end_cu if c in c_end_cu]
late = [c_end_cu[c] - t_end_cu[c] for c in both if c_end_cu[c] > t_end_cu[c]]
print(f"CUs with both roles: {len(both)}, conversion role ends after the CU's last T tile on {len(late)} of them"
      + (f" (by median {np.median(late):.0f}, max {max(late):.0f} cycles)" if late else ""))
for k in sorted(xcd_t0):
    tk = (T[:, 5] - t_rel)[t_xcc == k]
    ck = (C[:, 5] - c_rel)[c_xcc == k]
    print(f"   XCD {k}: last T tile ends {tk.max() if len(tk) else 0:6.0f} after its CU's first entry, last conversion block {ck.max() if len(ck) else 0:6.0f}")
