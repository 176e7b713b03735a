#!/usr/bin/env python3
"""ISA summary of the LDS Cholesky read-out kernel (readout_chol_kernel in esn_solve_chol.hip).  Needs hipcc, no GPU.

Compiles esn_solve_chol.hip and esn_solve_chol_big.hip (--all: esn_solve_qr.hip, esn_loo.hip, esn_gram.hip and
esn_holdout.hip too, whose kernels share code with them or must not notice a change to them) to gfx950 assembly with the
product flags of esn_ofdm_mimo_amd/build.py and prints, per
kernel instance: VGPRs, spilled VGPRs / SGPRs and scratch bytes; and for
the instances of readout_chol_kernel the instruction mix of the stretch between the two s_barrier that bracket the
diagonal-block factorisation (the last barrier in front of the first v_rsq_f64 -- the square root of the pivot, the
kernel has no other -- and the first barrier behind the last one).  tests/test_chol_structure.py holds the scratch
size, the VGPR count and the lane-traffic count of that stretch to bounds.

    python tools/chol_isa.py                      # all instances
    python tools/chol_isa.py --asm FILE.s         # an assembly file made earlier (another commit's, say)
    python tools/chol_isa.py --all --against FILE.s      # one row per kernel: VGPRs, spilled SGPRs and instructions of
                                                  # FILE.s -> this tree, and whether the opcode sequences are equal
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
SOURCES = ("esn_solve_chol.hip", "esn_solve_chol_big.hip", "esn_solve_qr.hip", "esn_loo.hip", "esn_gram.hip",
           "esn_holdout.hip")


def compile_asm(out, sources=SOURCES[:2]):
    """The gfx950 assembly of `sources`, one after the other, in the file `out` (the two Cholesky files by default)"""
    from esn_ofdm_mimo_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = os.environ.get("ESN_EXTRA_FLAGS", "").split()
    with open(out, "w") as f:
        for src in sources:
            pr = subprocess.run([hipcc, *build.FLAGS, *extra, "--cuda-device-only", "-S",
                                 os.path.join(build.CSRC, src), "-o", "-"], capture_output=True, text=True)
            if pr.returncode != 0:                  # (the warnings of a compile that succeeds are not shown)
                sys.stderr.write(pr.stderr)
                raise RuntimeError(f"hipcc failed on {src}")
            f.write(pr.stdout)


def functions(lines):
    """{name: (body lines, {metadata key: value})} of every esn::*_kernel in the assembly: the Cholesky kernels and,
    where compiled in, those of the QR, leave-one-out, running-normal-equations and hold-out files"""
    out, name, body = {}, None, []
    for ln in lines:
        m = re.match(r"^(_ZN3esn\d+[a-z0-9_]+_kernel\w+):", ln)
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


def compare(old, new):
    """One row per kernel of `old` that `new` has too (both from functions())"""
    print(f"{'kernel':68s} {'VGPRs':>11s} {'spilled SGPRs':>14s} {'instructions':>24s}")
    for name, (body, meta) in old.items():
        if name not in new:
            continue
        a, b = ([ln.split()[0] for ln in bd if is_inst(ln)] for bd in (body, new[name][0]))
        m = new[name][1]
        print(f"{name:68s} {meta['vgpr_count']:4d} -> {m['vgpr_count']:4d} {meta['sgpr_spill_count']:6d} -> "
              f"{m['sgpr_spill_count']:4d} {len(a):7d} -> {len(b):5d} {100.0 * (len(b) - len(a)) / len(a):+6.2f} %"
              + ("  same opcode sequence" if a == b else ""))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--all", action="store_true", help="compile the other read-out files as well")
    ap.add_argument("--against", help="an earlier assembly file: print the comparison table instead of the summary")
    args = ap.parse_args()
    if args.asm:
        path = args.asm
    else:
        path = os.path.join(tempfile.mkdtemp(prefix="chol_isa_"), "esn_solve_chol.s")
        compile_asm(path, SOURCES if args.all else SOURCES[:2])
    with open(path) as f:
        fns = functions(f.read().splitlines())
    if args.against:
        with open(args.against) as f:
            return compare(functions(f.read().splitlines()), fns)
    for name, (body, meta) in fns.items():
        print(f"{name}\n  VGPRs {meta.get('vgpr_count')}  spilled VGPRs {meta.get('vgpr_spill_count')}  spilled SGPRs "
              f"{meta.get('sgpr_spill_count')}  scratch bytes {meta.get('private_segment_fixed_size')}")
        if "readout_chol_kernel" not in name:
            continue
        mix = diag_stretch(body)
        print(f"  diagonal-block stretch: {sum(mix.values())} instructions, v_readlane + v_writelane {lane_traffic(mix)}")
        print("   " + "  ".join(f"{op} {n}" for op, n in mix.most_common(12)))


if __name__ == "__main__":
    main()
