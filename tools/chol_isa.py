#!/usr/bin/env python3
"""ISA summary of the LDS Cholesky read-out kernel (readout_chol_kernel in esn_solve.hip).  Needs hipcc, no GPU.

Compiles esn_solve.hip to gfx950 assembly with the product flags of esn_ofdm_mimo_amd/build.py and prints, per
instance of readout_chol_kernel and readout_chol_big_kernel: VGPRs, spilled VGPRs / SGPRs and scratch bytes; and for
the instances of readout_chol_kernel the instruction mix of the stretch between the two s_barrier that bracket the
diagonal-block factorisation (the last barrier in front of the first v_rsq_f64 -- the square root of the pivot, the
kernel has no other -- and the first barrier behind the last one).  tests/test_chol_structure.py holds the scratch
size, the VGPR count and the lane-traffic count of that stretch to bounds.

    python tools/chol_isa.py                      # all instances
    python tools/chol_isa.py --asm FILE.s         # an assembly file made earlier (another commit's, say)
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADLINE = "_ZN3esn19readout_chol_kernelIfLb1ELb0EEEvNS_11SolveParamsE"      # float32 E, wide, no ridge


def compile_asm(out):
    from esn_ofdm_mimo_amd import build
    src = os.path.join(build.CSRC, "esn_solve.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = os.environ.get("ESN_EXTRA_FLAGS", "").split()
    subprocess.check_call([hipcc, *build.FLAGS, *extra, "--cuda-device-only", "-S", src, "-o", out],
                          stderr=subprocess.DEVNULL)


def functions(lines):
    """{name: (body lines, {metadata key: value})} of the Cholesky kernels"""
    out, name, body = {}, None, []
    for ln in lines:
        m = re.match(r"^(_ZN3esn(?:19readout_chol_kernel|23readout_chol_big_kernel)\w+):", ln)
        if m:
            name, body = m.group(1), []
            out[name] = (body, {})
        elif name and ln.startswith(".Lfunc_end"):
            name = None
        elif name:
            body.append(ln)
    cur = None
    for ln in lines:
        m = re.match(r"^\s+\.name:\s+(\S+)", ln)
        if m:
            cur = out.get(m.group(1))
        m = re.match(r"^\s+\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", ln)
        if m and cur:
            cur[1][m.group(1)] = int(m.group(2))
    return out


def is_inst(ln):
    s = ln.strip()
    return bool(s) and not s.startswith((";", ".", "//")) and not re.match(r"^[\w.$]+:", s)


def diag_stretch(body):
    """Counter of the opcodes between the barriers that bracket the diagonal-block factorisation"""
    ops = [ln.split()[0] for ln in body if is_inst(ln)]
    rsq = [i for i, op in enumerate(ops) if op.startswith("v_rsq_f64")]
    bars = [i for i, op in enumerate(ops) if op == "s_barrier"]
    first = max(b for b in bars if b < rsq[0])
    last = min(b for b in bars if b > rsq[-1])
    return collections.Counter(ops[first + 1:last])


def lane_traffic(mix):
    """v_readlane_b32 + v_writelane_b32: values that travel lane -> SGPR -> operand, and SGPR spills"""
    return mix["v_readlane_b32"] + mix["v_writelane_b32"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    args = ap.parse_args()
    if args.asm:
        path = args.asm
    else:
        path = os.path.join(tempfile.mkdtemp(prefix="chol_isa_"), "esn_solve.s")
        compile_asm(path)
    with open(path) as f:
        fns = functions(f.read().splitlines())
    for name, (body, meta) in fns.items():
        print(f"{name}\n  VGPRs {meta.get('vgpr_count')}  spilled VGPRs {meta.get('vgpr_spill_count')}  spilled SGPRs "
              f"{meta.get('sgpr_spill_count')}  scratch bytes {meta.get('private_segment_fixed_size')}")
        if "big" in name:
            continue
        mix = diag_stretch(body)
        print(f"  diagonal-block stretch: {sum(mix.values())} instructions, v_readlane + v_writelane {lane_traffic(mix)}")
        print("   " + "  ".join(f"{op} {n}" for op, n in mix.most_common(12)))


if __name__ == "__main__":
    main()
