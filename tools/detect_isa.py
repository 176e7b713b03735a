#!/usr/bin/env python3
"""ISA summary of the fixed-shape instances of the detector tail (detect_count_fixed_kernel in esn_detect.hip).  Needs
hipcc, no GPU.

Compiles esn_detect.hip to gfx950 assembly with the product flags of esn_ofdm_mimo_amd/build.py and prints, per
instance: VGPRs, scratch bytes and LDS bytes; and the instruction mix of the frame loop -- the outermost loop of the
kernel, found as the longest stretch between a label and a backward branch to it: vector instructions, float64 vector
instructions, LDS instructions, s_barrier and v_mul_hi_u32.  The loop takes FRAMES_PER_TRIP frames per trip (two
register sets for the loads in flight); the tool checks that against the row loads it finds in the loop.  One wave
executes the loop, so "vector instructions per frame" is the static count over the frames per trip.
tests/test_detect_structure.py holds these numbers to bounds.

    python tools/detect_isa.py                    # both instances
    python tools/detect_isa.py --asm FILE.s       # an assembly file made earlier
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
FRAMES_PER_TRIP = 2
ROW_LOADS_PER_FRAME = 8                  # a lane's eight rows; float64 Y: global_load_dwordx4, float32 Y: dwordx2
TX_LOADS_PER_FRAME = 2                   # global_load_dwordx4


def instance_name(io32):
    return f"_ZN3esn25detect_count_fixed_kernelILb{int(io32)}ELi7ELi4ELi4EEEvNS_12DetectParamsE"


def compile_asm(out):
    from esn_ofdm_mimo_amd import build
    src = os.path.join(build.CSRC, "esn_detect.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = os.environ.get("ESN_EXTRA_FLAGS", "").split()
    subprocess.check_call([hipcc, *build.FLAGS, *extra, "--cuda-device-only", "-S", src, "-o", out],
                          stderr=subprocess.DEVNULL)


def functions(lines):
    """{name: (body lines, {metadata key: value})} of the fixed instances"""
    out, name, body = {}, None, []
    for ln in lines:
        m = re.match(r"^(_ZN3esn25detect_count_fixed_kernel\w+):", ln)
        if m:
            name, body = m.group(1), []
            out[name] = (body, {})
        elif name and ln.startswith(".Lfunc_end"):
            name = None
        elif name:
            body.append(ln)
    entry = {}                                       # amdhsa.kernels: one "  - .key: value" list entry per kernel
    for ln in lines + ["  - .end: 0"]:
        m = re.match(r"^\s+(- )?\.(\w+):\s+(\S+)", ln)
        if not m:
            continue
        if m.group(1):
            if entry.get("name") in out:
                out[entry["name"]][1].update({k: int(v) for k, v in entry.items() if v.isdigit()})
            entry = {}
        entry.setdefault(m.group(2), m.group(3))
    return out


def is_inst(ln):
    s = ln.strip()
    return bool(s) and not s.startswith((";", ".", "//")) and not re.match(r"^[\w.$]+:", s)


def frame_loop(body):
    """the instructions (opcode, operands) of the outermost loop: the longest label .. backward branch stretch"""
    label_at, insts = {}, []
    for ln in body:
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            label_at[m.group(1)] = len(insts)
        elif is_inst(ln):
            parts = ln.split(None, 1)
            insts.append((parts[0], parts[1].split(";")[0].strip() if len(parts) > 1 else ""))
    best = None
    for i, (op, args) in enumerate(insts):
        if op.startswith(("s_cbranch", "s_branch")) and args in label_at and label_at[args] <= i:
            if best is None or i - label_at[args] > best[1] - best[0]:
                best = (label_at[args], i)
    if best is None:
        raise ValueError("no loop in the kernel")
    return insts[best[0]:best[1] + 1]


def is_valu(op):
    return op.startswith("v_") and not op.startswith(("v_readlane", "v_readfirstlane", "v_writelane"))


def loop_stats(body, io32):
    """counts of the frame loop, per trip, and the frames per trip checked against the loads in it"""
    loop = frame_loop(body)
    ops = collections.Counter(op for op, _ in loop)
    x4, x2 = ops["global_load_dwordx4"], ops["global_load_dwordx2"]
    frames = (x4 / TX_LOADS_PER_FRAME) if io32 else (x4 / (ROW_LOADS_PER_FRAME + TX_LOADS_PER_FRAME))
    if frames != FRAMES_PER_TRIP or (io32 and x2 != ROW_LOADS_PER_FRAME * FRAMES_PER_TRIP):
        raise ValueError(f"the loop found holds {x4} dwordx4 and {x2} dwordx2 loads: not {FRAMES_PER_TRIP} frames per trip")
    return {
        "instructions": len(loop),
        "valu": sum(n for op, n in ops.items() if is_valu(op)),
        "valu_f64": sum(n for op, n in ops.items() if is_valu(op) and "_f64" in op),
        "lds": sum(n for op, n in ops.items() if op.startswith("ds_")),
        "s_barrier": ops["s_barrier"],
        "v_mul_hi_u32": ops["v_mul_hi_u32"],
        "readlane": ops["v_readlane_b32"] + ops["v_readfirstlane_b32"],
        "frames_per_trip": FRAMES_PER_TRIP,
        "valu_per_frame": sum(n for op, n in ops.items() if is_valu(op)) / FRAMES_PER_TRIP,
        "top": ops.most_common(14),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    args = ap.parse_args()
    if args.asm:
        path = args.asm
    else:
        path = os.path.join(tempfile.mkdtemp(prefix="detect_isa_"), "esn_detect.s")
        compile_asm(path)
    with open(path) as f:
        fns = functions(f.read().splitlines())
    for io32 in (False, True):
        body, meta = fns[instance_name(io32)]
        st = loop_stats(body, io32)
        print(f"{instance_name(io32)}   (Y {'float32' if io32 else 'float64'})")
        print(f"  VGPRs {meta.get('vgpr_count')}  spilled VGPRs {meta.get('vgpr_spill_count')}  scratch bytes "
              f"{meta.get('private_segment_fixed_size')}  LDS bytes {meta.get('group_segment_fixed_size')}")
        print(f"  frame loop, {st['frames_per_trip']} frames per trip: {st['instructions']} instructions, vector {st['valu']} "
              f"({st['valu_per_frame']:.0f} per frame), float64 vector {st['valu_f64']}, LDS {st['lds']}, "
              f"s_barrier {st['s_barrier']}, v_mul_hi_u32 {st['v_mul_hi_u32']}, v_readlane / v_readfirstlane {st['readlane']}")
        print("   " + "  ".join(f"{op} {n}" for op, n in st["top"]))


if __name__ == "__main__":
    main()
