"""What two side launches of the bilinear step do before their first useful instruction, held on the compiled code.

bilinear_dw_kernel (csrc/mi_bilinear_tail.h) reads both problem records in one batch: at most two waits for scalar loads
stand in front of its first operand load (it was five, each a round trip to a cold kernel-argument segment, with ~170
instructions of software 64-bit division between them), and no 64-bit division is left in the kernel.

bilinear_prep_t_kernel<false, 64, true> (csrc/mi_gemm_bf16.h), the form the headline step takes, runs three workgroups per
CU: at most 168 registers per lane and no scratch (its LDS is held by a static_assert beside prep_t_smem).

Runs on the CPU (hipcc cross-compiles for gfx950)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mutual-information-multimodal_amd", "csrc")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """name -> (instruction lines, metadata comment block) of every kernel in mi_bilinear.hip."""
    out = tmp_path_factory.mktemp("isa") / "mi_bilinear.s"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "--offload-arch=gfx950", "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "mi_bilinear.hip")], check=True,
                   stderr=subprocess.DEVNULL, timeout=900)
    asm = out.read_text()
    found = {}
    for m in re.finditer(r"^(_ZN2mi\w+):[^\n]*\n", asm, re.M):
        end = asm.find(".Lfunc_end", m.end())
        if end < 0:
            continue
        lines = [ln.split(";")[0].split() for ln in asm[m.end():end].split("\n")]
        lines = [t for t in lines if t and not t[0].startswith((".", "#")) and not t[0].endswith(":")]
        nxt = asm.find(".Lfunc_begin", end)  # the "; NumVgprs: ..." block follows the function's end
        found[m.group(1)] = (lines, asm[end:nxt if nxt > 0 else len(asm)])
    return found


def _one(kernels, needle):
    hit = {n: v for n, v in kernels.items() if needle in n}
    assert len(hit) == 1, f"{needle}: {sorted(hit)}"
    return next(iter(hit.items()))


def _meta(block, key):
    m = re.search(rf";\s*{key}:\s*(\d+)", block)
    assert m, f"no `{key}` in the kernel's metadata comments"
    return int(m.group(1))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_dw_kernel_reaches_its_first_load_behind_two_scalar_waits(kernels):
    name, (lines, meta) = _one(kernels, "bilinear_dw_kernel")
    first = next((i for i, t in enumerate(lines) if t[0].startswith("global_load")), None)
    assert first is not None, f"{name}: no global load"
    waits = [t for t in lines[:first] if t[0] == "s_waitcnt" and "lgkmcnt(0)" in t[1:]]
    print(f"{name}: {first} instructions and {len(waits)} scalar-load waits before the first global_load")
    assert len(waits) <= 2, f"{name}: {len(waits)} waits for scalar loads before the first global_load"
    # hipcc expands a 64-bit integer division inline (~85 instructions each); its reciprocal estimate scales by the float
    # constant 0x5f7ffffc (just under 2^64) -- the 32-bit expansion (v_rcp_iflag_f32, 0x4f7ffffe) has no such literal
    text = " ".join(" ".join(t) for t in lines)
    assert "0x5f7ffffc" not in text, f"{name}: a software 64-bit division is back in the kernel"
    assert _meta(meta, "ScratchSize") == 0


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_prep_kernel_headline_form_fits_three_workgroups_per_cu(kernels):
    name, (_, meta) = _one(kernels, "bilinear_prep_t_kernelILb0ELi64ELb1E")
    vgprs, scratch = _meta(meta, "NumVgprs"), _meta(meta, "ScratchSize")
    print(f"{name}: {vgprs} VGPRs, {scratch} bytes of scratch")
    assert vgprs <= 168, f"{name}: {vgprs} VGPRs -- three 256-thread workgroups per CU need <= 168"
    assert scratch == 0, f"{name}: {scratch} bytes of scratch"
