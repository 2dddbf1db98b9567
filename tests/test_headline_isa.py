"""Instruction budget of the headline rollout step (PredatorPrey map 10, teams of 4, two hops, carried, full workgroups:
rollout_w_kernel<2, true, true, false, true, 1>).  That kernel runs ONE wave per SIMD, so every vector instruction of its step
loop is ~4 clk of the step; this pins the counts the step was brought down to, on the ISA hipcc emits with the
Makefile's flags.  Needs hipcc, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "_ZN2cm16rollout_w_kernelILi2ELb1ELb1ELb0ELb1ELi1EEE"       # <LHOPS 2, PRE, FULLWG, !TAPE, CARRY, SHAPE 1>

MFMA = re.compile(r"^v_mfma_")
# what issues on the vector ALU: v_* without the matrix pipe; the AGPR copies are VALU instructions as well
VALU = re.compile(r"^v_(?!mfma_)")


def compile_isa(out):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "com-marl_amd", "csrc", "cm_rollout_w.hip")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-mllvm",
                           "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize", "-S", "--cuda-device-only", "-w", "-o", str(out), src])
    return open(out).read()


def kernel_body(asm, prefix):
    """The instruction lines of the one kernel whose mangled name starts with `prefix` (labels kept, directives and comments
    dropped), and its metadata block."""
    bodies = [m for m in re.finditer(r"^(_ZN2cm16rollout_w_kernel\S+):[^\n]*\n(.*?)\n\.Lfunc_end", asm, re.M | re.S)
              if m.group(1).startswith(prefix)]
    assert len(bodies) == 1, f"expected one kernel {prefix}*, found {[m.group(1) for m in bodies]}"
    lines = []
    for ln in bodies[0].group(2).splitlines():
        ln = ln.split(";")[0].strip()
        if ln and (not ln.startswith(".") or re.match(r"\.LBB\d+_\d+:", ln)):
            lines.append(ln)
    meta = [b for b in re.split(r"\n\s+- \.agpr_count:", asm)[1:] if re.search(r"\.name:\s+" + re.escape(bodies[0].group(1)) + r"\s", b)]
    assert len(meta) == 1, "no metadata block for " + bodies[0].group(1)
    return lines, meta[0]


def step_loop(lines):
    """The largest span closed by a backward branch: the step loop (everything else in the body is straight-line set-up, the
    staging rounds and the short element loops of the env phase)."""
    label_at = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":")}
    best = None
    for i, ln in enumerate(lines):
        m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)$", ln)
        if m and m.group(1) in label_at and label_at[m.group(1)] < i:
            if best is None or i - label_at[m.group(1)] > best[1] - best[0]:
                best = (label_at[m.group(1)], i)
    assert best is not None, "no backward branch in the kernel body: the step loop was not found"
    loop = [ln for ln in lines[best[0]:best[1] + 1] if not ln.endswith(":")]
    return loop


def counts(loop):
    mfma = [ln for ln in loop if MFMA.match(ln)]
    return {
        "insts": len(loop),
        "mfma": len(mfma),
        # an A / B source operand in AGPRs: `v_mfma_... v[0:3], a[8:11], v[..], v[..]` (operands 2 and 3)
        "mfma_agpr_src": sum(1 for ln in mfma if any(op.strip().startswith("a[") for op in ln.split(None, 1)[1].split(", ")[1:3])),
        "accvgpr_read": sum(1 for ln in loop if ln.startswith("v_accvgpr_read_b32")),
        "accvgpr_write": sum(1 for ln in loop if ln.startswith("v_accvgpr_write_b32")),
        "valu": sum(1 for ln in loop if VALU.match(ln)),
        "cvt_f32_f16": sum(1 for ln in loop if ln.startswith("v_cvt_f32_f16")),
        "readlane": sum(1 for ln in loop if ln.startswith("v_readlane_b32")),
        "s_nop": sum(1 for ln in loop if ln.startswith("s_nop")),
        "salu": sum(1 for ln in loop if ln.startswith("s_")),
        "ds_read_b128": sum(1 for ln in loop if ln.startswith("ds_read_b128")),
    }


def test_headline_step_loop_instruction_budget(tmp_path):
    asm = compile_isa(tmp_path / "cm_rollout_w.s")
    lines, meta = kernel_body(asm, HEADLINE)
    loop = step_loop(lines)
    n = counts(loop)
    print("headline step loop:", n)
    # the loop found must be the step: the whole policy tile (288 MFMAs: 264 of 16x16x32, 24 of 16x16x16) sits inside it
    assert n["mfma"] >= 288, n
    assert re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1) == "0"
    assert re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1) == "0"
    # the resident 128 -> 64 layer (4 tiles x 4 k blocks x 3 products) is read by the MFMAs where it lives, in AGPRs ...
    assert n["mfma_agpr_src"] >= 48, n
    # ... so the copies in front of them are gone (158 before; what remains are ordinary spill reloads)
    assert n["accvgpr_read"] <= 30, n
    # 3 088 before; 2 959 with the copies gone; 2 658 with the split's residual written by v_fma_mixlo_f16 / v_fma_mixhi_f16
    # (no v_cvt_f32_f16 + v_sub_f32 per value, no second v_cvt_pk_f16_f32 per pair)
    assert n["valu"] <= 2658, n
    assert n["cvt_f32_f16"] == 0, n
