"""The stores that cross a kernel boundary of the fused bilinear step carry a cache policy (csrc/mi_common.h: seam_store
and MI_SEAM_TABLE).  This test compiles the kernels to gfx950 assembly and holds every global store of the four kernels
against THAT table, so that a later edit cannot fall back to plain stores unseen; kernels the table does not name must
carry no cache bits at all.  Runs on the CPU (hipcc cross-compiles for gfx950)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mutual-information-multimodal_amd", "csrc")
BITS = {"NT": "nt", "WT": "sc0 sc1", "PLAIN": ""}
# plain stores a table kernel may keep: words written once per launch by one thread or a handful, not seam traffic
PLAIN_ALLOWED = {
    "bilinear_prep_t_kernel": lambda ops: all(op == "global_store_byte" for op in ops),       # the equal-id tile flags
    "flash_tail_kernel": lambda ops: len(ops) <= 8,   # MERGE form: workgroup 0 publishes the statistics block and the loss
}
UNTOUCHED = ("gemm_bf16_big_kernel", "cvt_transpose3_kernel", "flash_reduce_kernel")


def seam_table():
    """(group, kernel, policy) rows of MI_SEAM_TABLE."""
    src = open(os.path.join(CSRC, "mi_common.h")).read()
    body = src[src.index("#define MI_SEAM_TABLE(X)"):]
    body = body[:body.index("#ifndef MI_SEAM_OFF")]
    rows = re.findall(r"X\((\d+),\s*(\w+),\s*(\w+),\s*(\w+)\)", body)
    assert rows, "MI_SEAM_TABLE not found in mi_common.h"
    return [(g, k, p) for _, g, k, p in rows]


def stores_by_kernel(asm):
    out = {}
    for m in re.finditer(r"^(_ZN2mi\w+):[^\n]*\n", asm, re.M):
        end = asm.find(".Lfunc_end", m.end())
        if end < 0:
            continue
        st = []
        lines = [ln.split(";")[0].split() for ln in asm[m.end():end].split("\n")]
        lines = [t for t in lines if t and not t[0].startswith((".", "#")) and not t[0].endswith(":")]
        for i, t in enumerate(lines):
            if re.match(r"(global|flat|buffer)_store", t[0]):
                bits = " ".join(w for w in t[1:] if w in ("sc0", "sc1", "nt"))
                st.append((t[0], bits))
                # the write-through stores come from inline asm, where hipcc's hazard recognizer does not see them: a
                # store wider than 8 bytes needs two wait states before a VALU write to its data registers (gfx940+)
                if bits == "sc0 sc1" and t[0].endswith("dwordx4"):
                    nxt = lines[i + 1] if i + 1 < len(lines) else ["s_endpgm"]
                    assert nxt[0] == "s_nop" and int(nxt[1]) >= 1, f"{m.group(1)}: `{' '.join(t)}` without its s_nop"
        out[m.group(1)] = st
    return out


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_seam_stores_carry_the_cache_bits_of_the_table(tmp_path):
    out = tmp_path / "mi_bilinear.s"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "--offload-arch=gfx950", "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "mi_bilinear.hip")], check=True,
                   stderr=subprocess.DEVNULL, timeout=900)
    kernels = stores_by_kernel(out.read_text())
    table = seam_table()
    assert {k for _, k, _ in table} == {"bilinear_prep_t_kernel", "bilinear_flash_kernel", "flash_tail_kernel", "bilinear_dw_kernel"}
    for kernel in sorted({k for _, k, _ in table}):
        want = {BITS[p] for _, k, p in table if k == kernel}
        inst = {n: s for n, s in kernels.items() if kernel in n}
        assert inst, f"no instantiation of {kernel} in the assembly"
        for name, st in inst.items():
            assert st, f"{name}: no global store at all"
            seen = {bits for _, bits in st}
            plain = [op for op, bits in st if bits == ""]
            # every policy the table names for this kernel is on at least one store (the forward-only fused kernel has the
            # record store alone, the other forms of the tail both of theirs) ...
            assert (want - {""}) & seen == want - {""} or ("flash_kernel" in kernel and seen == {"sc0 sc1"}), \
                f"{name}: stores carry {sorted(seen)}, the table names {sorted(want)}"
            # ... no store carries bits the table does not name for it ...
            assert seen - {""} <= want, f"{name}: stores carry {sorted(seen)}, the table names {sorted(want)}"
            # ... and what stays plain is on the short list above
            if plain and "" not in want:
                ok = PLAIN_ALLOWED.get(kernel)
                assert ok is not None and ok(plain), f"{name}: {len(plain)} plain global stores: {sorted(set(plain))}"
    for kernel in UNTOUCHED:
        inst = {n: s for n, s in kernels.items() if kernel in n}
        assert inst, f"no instantiation of {kernel} in the assembly"
        for name, st in inst.items():
            assert all(bits == "" for _, bits in st), f"{name}: a kernel outside the table carries cache bits"
