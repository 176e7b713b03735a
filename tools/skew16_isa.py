#!/usr/bin/env python3
"""ISA summary of the 16x16x32 skewed predict kernel (esn_recur_skew16_impl.h).  Needs hipcc, no GPU.

Compiles esn_recur_skew16.hip to gfx950 assembly with the product flags of esn_ofdm_mimo_amd/build.py and prints,
per selected instance: VGPRs, spilled VGPRs / SGPRs, scratch bytes, s_barrier / s_swappc / scratch-instruction counts
of the whole kernel and of its step loops, and per Depth=2 loop (the GEMM trip loops; the short ones are the
readfirstlane loops of a buffer descriptor) the counts of instructions, MFMAs, ds_read, buffer_load, s_waitcnt,
scratch operations and the vmcnt values waited for; and the structure counters of structure() below (readfirstlane-loop
latches between the barriers of the step loops, element-wise LDS fill loops in front of them, scratch inside trip loops),
which tests/test_skew16_structure.py holds to bounds.

    python tools/skew16_isa.py                      # headline instance: TraitsF16, counter noise, float64 I/O
    python tools/skew16_isa.py --all                # all twelve, one summary line each
    python tools/skew16_isa.py --asm FILE.s         # an assembly file made earlier (another commit's, say)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADLINE = "recur_skew16_kernelINS_9TraitsF16ELi2ELb0EEE"


def compile_asm(out):
    from esn_ofdm_mimo_amd import build
    src = os.path.join(build.CSRC, "esn_recur_skew16.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = os.environ.get("ESN_EXTRA_FLAGS", "").split()
    subprocess.check_call([hipcc, *build.FLAGS, *extra, "--cuda-device-only", "-S", src, "-o", out])


def functions(lines, kernel="_ZN3esn19recur_skew16_kernel"):
    """{name: (body lines, {metadata key: value})} of the instances of `kernel` (the head of the mangled name)"""
    out, name, body = {}, None, []
    head = re.compile(r"^(" + re.escape(kernel) + r"\w+):")
    for ln in lines:
        m = head.match(ln)
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


def count(body):
    c = dict(inst=0, mfma=0, ds_read=0, ds_write=0, buffer_load=0, waitcnt=0, scratch=0, barrier=0, swappc=0, vmcnt=[])
    for ln in body:
        if not is_inst(ln):
            continue
        op = ln.split()[0]
        c["inst"] += 1
        c["mfma"] += op.startswith("v_mfma")
        c["ds_read"] += op.startswith("ds_read")
        c["ds_write"] += op.startswith("ds_write")
        c["buffer_load"] += op.startswith("buffer_load")
        c["scratch"] += op.startswith("scratch_")
        c["barrier"] += op == "s_barrier"
        c["swappc"] += op.startswith("s_swappc")
        if op == "s_waitcnt":
            c["waitcnt"] += 1
            m = re.search(r"vmcnt\((\d+)\)", ln)
            if m:
                c["vmcnt"].append(int(m.group(1)))
    return c


def loops(body):
    """[(depth, first line index, last line index)] from the compiler's loop comments"""
    labels = {}
    for i, ln in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            labels[m.group(1)] = i
    found, starts = [], sorted(labels.values())
    for lab, i in labels.items():
        depth = None
        j = i
        while j < len(body) and (j == i or body[j].strip().startswith(";")):      # the label's comment lines
            m = re.search(r"Loop Header: Depth=(\d+)", body[j])
            if m:
                depth = int(m.group(1))
            j += 1
        if depth is None:
            continue
        # the loop's blocks carry "in Loop: Header=BBf_n" / "Parent Loop BBf_n" comments (a rotated loop has blocks in
        # front of its header); it ends where the last of them does
        ref = re.compile(r"(Header=|Parent Loop )" + re.escape(lab[2:]) + r"\b")
        members = [k for k, ln in enumerate(body) if ref.search(ln)] + [i]
        first = max([k for k in starts if k <= min(members)], default=0)
        last = min([k for k in starts if k > max(members)], default=len(body)) - 1
        back = [k for k in range(max(members), last + 1)
                if re.match(r"\s+s_c?branch\w*\s+" + re.escape(lab) + r"\s*$", body[k])]
        if back:                      # the code behind the latch branch, up to the next label, is not the loop's
            last = max(back)
        found.append((depth, first, last))
    return sorted(found, key=lambda t: t[1])


def step_loops(body, lp):
    return [(a, b) for d, a, b in lp if d == 1 and count(body[a:b + 1])["mfma"] > 100]


def ops(body, a, b):
    return [(i, body[i].split()[0]) for i in range(a, b + 1) if is_inst(body[i])]


def structure(body, meta):
    """What surrounds the recurrence slots, as numbers (tests/test_skew16_structure.py holds them to bounds):
    execnz_in_steps   s_cbranch_execnz (the latch of a readfirstlane loop around a buffer operation whose descriptor the
                      compiler holds in VGPRs) between the first and the last s_barrier of a step loop, summed over both
    b16_loops_before  loops in front of the first step loop that hold a ds_write_b16 (element-wise LDS fills)
    spilled_vgprs     of the whole kernel
    trip_scratch      scratch instructions inside the GEMM trip loops (Depth=2 loops with MFMAs)"""
    lp = loops(body)
    steps = step_loops(body, lp)
    execnz = 0
    for a, b in steps:
        bars = [i for i, op in ops(body, a, b) if op == "s_barrier"]
        execnz += sum(op == "s_cbranch_execnz" for _, op in ops(body, bars[0], bars[-1])) if bars else 0
    first = min((a for a, _ in steps), default=len(body))
    b16 = sum(1 for _, a, b in lp if b < first and any(op.startswith("ds_write_b16") for _, op in ops(body, a, b)))
    trip = sum(count(body[x:y + 1])["scratch"] for d, x, y in lp
               if d == 2 and any(a <= x and y <= b for a, b in steps) and count(body[x:y + 1])["mfma"])
    return dict(step_loops=len(steps), execnz_in_steps=execnz, b16_loops_before=b16,
                spilled_vgprs=meta.get("vgpr_spill_count"), trip_scratch=trip)


def report(name, body, meta, brief):
    whole = count(body)
    lp = loops(body)
    steps = step_loops(body, lp)
    head = (f"{name}\n  VGPRs {meta.get('vgpr_count')}  spilled VGPRs {meta.get('vgpr_spill_count')}  spilled SGPRs "
            f"{meta.get('sgpr_spill_count')}  scratch bytes {meta.get('private_segment_fixed_size')}  instructions "
            f"{whole['inst']}  s_barrier {whole['barrier']}  s_swappc {whole['swappc']}  scratch instructions {whole['scratch']}")
    print(head)
    st = structure(body, meta)
    print(f"  s_cbranch_execnz between the barriers of the step loops {st['execnz_in_steps']}  loops with ds_write_b16 in front "
          f"of the step loops {st['b16_loops_before']}  scratch instructions inside the trip loops {st['trip_scratch']}")
    if brief:
        for a, b in steps:
            c = count(body[a:b + 1])
            print(f"  step loop: {c['inst']} instructions, {c['mfma']} MFMA, {c['barrier']} s_barrier, {c['scratch']} scratch")
        return
    for n, (a, b) in enumerate(steps):
        c = count(body[a:b + 1])
        print(f"  step loop {n} (lines {a}-{b} of the function): instructions {c['inst']}  MFMA {c['mfma']}  ds_read {c['ds_read']}  "
              f"ds_write {c['ds_write']}  buffer_load {c['buffer_load']}  s_waitcnt {c['waitcnt']}  s_barrier {c['barrier']}  "
              f"scratch {c['scratch']}  vmcnt(0) waits {c['vmcnt'].count(0)}")
        sc = [i for i in range(a, b + 1) if is_inst(body[i]) and body[i].split()[0].startswith("scratch_")]
        inner = [(x, y) for d, x, y in lp if d == 2 and a <= x and y <= b]
        for x, y in inner:
            k = count(body[x:y + 1])
            if k["mfma"] == 0:
                continue
            # scratch instructions between the previous GEMM loop / barrier and this loop's header (the reload trap)
            j = x
            while j > a and not (is_inst(body[j]) and body[j].split()[0] in ("s_barrier",)):
                j -= 1
            pre = sum(1 for i in sc if j <= i < x)
            print(f"    Depth-2 loop lines {x}-{y}: instructions {k['inst']}  MFMA {k['mfma']}  ds_read {k['ds_read']}  "
                  f"buffer_load {k['buffer_load']}  s_waitcnt {k['waitcnt']}  scratch {k['scratch']}  "
                  f"vmcnt waited for {sorted(set(k['vmcnt']))}  scratch between the barrier before and the loop {pre}")
        if sc:
            print(f"    scratch instructions of the step loop at lines {sc}")
    outside = whole["barrier"] - sum(count(body[a:b + 1])["barrier"] for a, b in steps)
    print(f"  s_barrier outside the step loops: {outside}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--all", action="store_true", help="all instances, brief")
    ap.add_argument("--match", default=HEADLINE, help="substring of the mangled instance name")
    args = ap.parse_args()
    if args.asm:
        path = args.asm
    else:
        path = os.path.join(tempfile.mkdtemp(prefix="skew16_isa_"), "esn_recur_skew16.s")
        compile_asm(path)
    with open(path) as f:
        fns = functions(f.read().splitlines())
    for name, (body, meta) in fns.items():
        if args.all or args.match in name:
            report(name, body, meta, args.all)


if __name__ == "__main__":
    main()
