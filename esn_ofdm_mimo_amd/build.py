"""Builds libesn_hip.so (the C-ABI library of include/esn_hip.h) in-tree with hipcc
for gfx950.  Called by __graft_entry__.build(); also runnable as a script."""
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libesn_hip.so")
SOURCES = ["esn_api.hip", "esn_host.hip", "esn_pack.hip", "esn_recur_f64.hip", "esn_recur_f64_mfma.hip", "esn_recur_mfma.hip",
           "esn_big_predict.hip", "esn_big_harvest.hip", "esn_recur_cluster.hip", "esn_recur_mfma_f32.hip", "esn_recur_mfma_f16.hip", "esn_recur_mfma_bf16.hip", "esn_recur_skew16.hip", "esn_harvest_cluster.hip",
           "esn_solve_qr.hip", "esn_solve_chol.hip", "esn_solve_chol_big.hip", "esn_loo.hip", "esn_holdout.hip", "esn_gram.hip", "esn_detect.hip", "esn_ensemble.hip", "esn_remod.hip", "esn_gen.hip", "esn_reservoir.hip", "esn_specrad_split.hip", "esn_baseline.hip", "esn_equalize.hip", "esn_dcc.hip", "esn_chantrack.hip", "esn_chanstat.hip", "esn_coded.hip", "esn_soft.hip",
           "esn_elm.hip", "esn_fnn.hip", "esn_cnn.hip", "esn_lstm.hip"]
# -fno-slp-vectorize: SLP turns adjacent float32 adds/fmas into v_pk_*_f32, which issue far slower
# than two scalar ops beside MFMAs (measured: predict kernel 13.97 -> 13.42 ms)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
         "-Wall", "-Wno-unused-function"]


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + \
           [os.path.join(PKG, "..", "include", "esn_hip.h"), os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force=False, verbose=True, stamps=False):
    """stamps=True builds the diagnostic variant libesn_hip_stamps.so (-DESN_STAMPS: in-kernel
    s_memtime phase stamps; never used for timing or by the product)."""
    global LIB
    if stamps:
        extra = ["-DESN_STAMPS"] + os.environ.get("ESN_EXTRA_FLAGS", "").split()
        return _build(os.path.join(PKG, "libesn_hip_stamps.so"), "build_stamps", extra, verbose)
    if not force and not _stale():
        return LIB
    return _build(LIB, "build", [], verbose)


def _build(LIB, bdir, extra, verbose):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    procs = []
    os.makedirs(os.path.join(PKG, bdir), exist_ok=True)
    for src in SOURCES:
        obj = os.path.join(PKG, bdir, src.replace(".hip", ".o"))
        objs.append(obj)
        per_file = os.environ.get("ESN_FLAGS_" + src.replace(".hip", "").upper(), "").split()
        cmd = [hipcc, *FLAGS, *extra, *per_file, "-c", os.path.join(CSRC, src), "-o", obj]
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, pr in procs:
        out, _ = pr.communicate()
        if pr.returncode != 0:
            sys.stderr.write(out.decode())
            raise RuntimeError(f"hipcc failed on {src}")
        if verbose and out.strip():
            sys.stderr.write(out.decode())
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs]
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    if "--variant" in sys.argv:     # tuning builds: libesn_hip_<name>.so with ESN_EXTRA_FLAGS (load via ESN_HIP_LIB)
        name = sys.argv[sys.argv.index("--variant") + 1]
        print(_build(os.path.join(PKG, f"libesn_hip_{name}.so"), "build_" + name,
                     os.environ.get("ESN_EXTRA_FLAGS", "").split(), True))
    else:
        print(build_library(force="--force" in sys.argv, stamps="--stamps" in sys.argv))
