#!/usr/bin/env python3
"""Register summary of every instance of the MFMA recurrence kernel (esn::recur_mfma_kernel).  Needs hipcc, no GPU.

Compiles esn_recur_mfma_{f32,f16,bf16}.hip to gfx950 assembly with the product flags of esn_ofdm_mimo_amd/build.py (the
three files in parallel) and prints, per instance: VGPRs, spilled VGPRs / SGPRs and private-segment bytes from the
code-object metadata, and the s_swappc count (a call: a function that was meant to be inlined was not).

    python tools/mfma_isa.py                        # the table
    python tools/mfma_isa.py --record               # ... and write it to tests/golden/mfma_parent_regs.json
    python tools/mfma_isa.py --asm A.s B.s C.s      # assembly files made earlier (another commit's, say)

tests/test_mfma_structure.py holds the instances of the working tree to the recorded ones."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skew16_isa  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "mfma_parent_regs.json")
KERNEL = "_ZN3esn17recur_mfma_kernel"
FILES = ("esn_recur_mfma_f32.hip", "esn_recur_mfma_f16.hip", "esn_recur_mfma_bf16.hip")
KEYS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "swappc")


def compile_asm(outdir):
    """the three instantiation files -> assembly, in parallel; returns the paths"""
    from esn_ofdm_mimo_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = os.environ.get("ESN_EXTRA_FLAGS", "").split()
    outs = [os.path.join(outdir, f.replace(".hip", ".s")) for f in FILES]
    procs = [subprocess.Popen([hipcc, *build.FLAGS, *extra, "--cuda-device-only", "-S", os.path.join(build.CSRC, f), "-o", o])
             for f, o in zip(FILES, outs)]
    for f, pr in zip(FILES, procs):
        if pr.wait() != 0:
            raise RuntimeError(f"hipcc failed on {f}")
    return outs


def table(paths):
    """{mangled instance name: {key of KEYS: value}}"""
    out = {}
    for path in paths:
        with open(path) as f:
            fns = skew16_isa.functions(f.read().splitlines(), KERNEL)
        for name, (body, meta) in fns.items():
            out[name] = dict(meta, swappc=skew16_isa.count(body)["swappc"])
    return out


def short(name):
    """TraitsF16 8,2,4 harvest=0 noise=2 skew=1 io32=0"""
    m = re.match(KERNEL + r"INS_\d+(Traits\w+?)ELi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELi(\d)ELb(\d)ELb(\d)EEE", name)
    if not m:
        return name
    tr, nw, mt, nt, hv, nz, sk, io = m.groups()
    return f"{tr:<10} {nw + ',' + mt + ',' + nt:<7} harvest={hv} noise={nz} skew={sk} io32={io}"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", nargs="+", help="read these assembly files instead of compiling")
    ap.add_argument("--record", action="store_true", help=f"write the table to {os.path.relpath(GOLDEN, ROOT)}")
    ap.add_argument("--commit", default="", help="with --record: hash of the commit the table was made from")
    args = ap.parse_args()
    t = table(args.asm or compile_asm(tempfile.mkdtemp(prefix="mfma_isa_")))
    print(f"{'instance':<58} VGPRs  spilled VGPRs  spilled SGPRs  private bytes  s_swappc")
    for name in sorted(t, key=short):
        r = t[name]
        print(f"{short(name):<58} {r['vgpr_count']:>5}  {r['vgpr_spill_count']:>13}  {r['sgpr_spill_count']:>13}  "
              f"{r['private_segment_fixed_size']:>13}  {r['swappc']:>8}")
    print(f"{len(t)} instances")
    if args.record:
        with open(GOLDEN, "w") as f:
            json.dump({"commit": args.commit, "keys": list(KEYS),
                       "instances": {n: [t[n][k] for k in KEYS] for n in sorted(t)}}, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"wrote {GOLDEN}")


if __name__ == "__main__":
    main()
