"""Records what the eight read-out solve entry points of libesn_hip.so (QR, Cholesky and leave-one-out; pinv and
ridge; float64 and float32 E) answer to calls they must refuse -- the return code and the full esn_last_error() text --
into tests/golden/readout_abi_errors.json, for tests/test_readout_abi_table_cpu.py to replay: a rewrite of the
argument checks that is meant to keep their answers keeps every code and every byte of every message.  Needs no GPU.

    python tools/record_readout_abi_errors.py <tree of the commit to pin>/esn_ofdm_mimo_amd/libesn_hip.so --commit <hash>

Every row is refused by the argument checks of esn_api.hip themselves, before any launcher or device call: the
pointers are small integers that are never valid.  Per entry point: each mandatory pointer null in turn; n_groups = 0,
transient = T, cols = 0, n_out = 0; n_out = 9; n_ridge = 0 and (leave-one-out) 17; at Gram dimension 129 a null
workspace, a workspace one byte short, E at address 72, the workspace at address 72; Gram dimension 513.  Left out,
because the checks let them through to a launcher: for the two QR entry points n_out = 9, Gram dimension 513 and the
short / misaligned rows (they take no workspace size and any alignment); for the two pinv Cholesky entry points
n_out = 9 at an LDS shape (recorded at Gram dimension 129 instead) and a null workspace at an LDS shape.  Added: the
leave-one-out workspace rows at its own small shape, since Gram dimension 129 is already refused there."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "readout_abi_errors.json")
HEAD = ["E", "D", "n_groups", "T", "transient", "cols", "n_out", "t_scale", "t_shift"]
RIDGE = ["ridge", "n_ridge"]
QR_TAIL = ["W_out", "status", "workspace", "stream"]
CHOL_TAIL = ["W_out", "status", "workspace", "workspace_bytes", "stream"]
LOO_TAIL = ["W_out", "score", "choice", "status", "workspace", "workspace_bytes", "stream"]
# entry point -> (parameter names in order, mandatory pointers, workspace query or None)
ENTRY_POINTS = {
    "esn_readout_solve_batch": (HEAD + QR_TAIL, ["E", "D", "W_out", "status", "workspace"], None),
    "esn_readout_solve_ridge_batch": (HEAD + RIDGE + QR_TAIL, ["E", "D", "ridge", "W_out", "status", "workspace"], None),
    "esn_readout_solve_chol_batch": (HEAD + CHOL_TAIL, ["E", "D", "W_out", "status"], "esn_readout_chol_workspace_bytes"),
    "esn_readout_solve_chol_batch_f32": (HEAD + CHOL_TAIL, ["E", "D", "W_out", "status"], "esn_readout_chol_workspace_bytes"),
    "esn_readout_solve_chol_ridge_batch": (HEAD + RIDGE + CHOL_TAIL, ["E", "D", "ridge", "W_out", "status"],
                                           "esn_readout_chol_ridge_workspace_bytes"),
    "esn_readout_solve_chol_ridge_batch_f32": (HEAD + RIDGE + CHOL_TAIL, ["E", "D", "ridge", "W_out", "status"],
                                               "esn_readout_chol_ridge_workspace_bytes"),
    "esn_readout_ridge_loo_batch": (HEAD + RIDGE + LOO_TAIL, ["E", "D", "ridge", "W_out", "score", "choice", "status"],
                                    "esn_readout_ridge_loo_workspace_bytes"),
    "esn_readout_ridge_loo_batch_f32": (HEAD + RIDGE + LOO_TAIL, ["E", "D", "ridge", "W_out", "score", "choice", "status"],
                                        "esn_readout_ridge_loo_workspace_bytes"),
}
PTR, ODD = 64, 72                  # a 16-byte aligned address and one that is only 8-byte aligned
SMALL = dict(n_groups=3, T=45, transient=5, cols=72, n_out=4, n_ridge=2)        # Gram dimension 40
GRAM_129 = dict(T=140, transient=0, cols=129)
GRAM_513 = dict(T=600, transient=0, cols=513)


def open_library(path):
    from esn_ofdm_mimo_amd import _lib
    lib = C.CDLL(path)
    for name in ["esn_last_error", "esn_abi_version"] + [n for n in _lib.SIGNATURES if n.startswith("esn_readout_")]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def need(lib, name, v):
    """What the entry point's workspace query says for the sizes in v."""
    query = ENTRY_POINTS[name][2]
    lam = (v["n_ridge"],) if "ridge" in query else ()
    return getattr(lib, query)(v["n_groups"], *lam, v["T"] - v["transient"], v["cols"])


def cases(lib):
    """[(entry point, case label, argument list)], None for a null pointer; `lib` answers the workspace queries."""
    out = []
    for name, (params, mandatory, query) in ENTRY_POINTS.items():
        kind = "qr" if query is None else "loo" if "loo" in name else "chol"
        base = {p: PTR for p in params}
        base.update({k: v for k, v in SMALL.items() if k in params}, t_scale=None, t_shift=None, stream=None)

        def row(label, short=0, **change):
            v = dict(base, **change)
            if "workspace_bytes" in params:         # what the query says for the row's sizes (0 at an LDS shape)
                v["workspace_bytes"] = need(lib, name, v) - short
            out.append((name, label, [v[p] for p in params]))

        for p in mandatory:
            row(f"null {p}", **{p: None})
        row("n_groups = 0", n_groups=0)
        row("transient = T", transient=base["T"])
        row("cols = 0", cols=0)
        row("n_out = 0", n_out=0)
        if kind != "qr" and "ridge" in params:
            row("n_out = 9", n_out=9)
        if "ridge" in params:
            row("n_ridge = 0", n_ridge=0)
        if kind == "loo":
            row("n_ridge = 17", n_ridge=17)
            row("null workspace", workspace=None)
            row("workspace one byte short", short=1)
            row("workspace at 68", workspace=68)
        row("Gram 129, null workspace", workspace=None, **GRAM_129)
        if kind != "qr":
            if "ridge" not in params:
                row("Gram 129, n_out = 9", n_out=9, **GRAM_129)
            row("Gram 129, workspace one byte short", short=1, **GRAM_129)
            row("Gram 129, E at 72", E=ODD, **GRAM_129)
            row("Gram 129, workspace at 72", workspace=ODD, **GRAM_129)
            row("Gram 513", **GRAM_513)
    return out


def answer(lib, name, args):
    rc = getattr(lib, name)(*args)
    return rc, lib.esn_last_error().decode()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("library", help="libesn_hip.so of the commit whose answers are to be pinned")
    ap.add_argument("--commit", required=True, help="hash of the commit that library was built from")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    lib = open_library(args.library)
    rows = []
    for name, label, a in cases(lib):
        rc, text = answer(lib, name, a)
        # a row that got past the argument checks is a wrong row: the launchers answer with other codes, or not at all
        assert rc in (-1, -2) and text.startswith(name + ": ") and "HIP error" not in text, (name, label, rc, text)
        rows.append({"fn": name, "case": label, "args": a, "rc": rc, "error": text})
    with open(args.out, "w") as f:
        f.write('{"abi": %d, "commit": %s, "rows": [\n' % (lib.esn_abi_version(), json.dumps(args.commit)))
        f.write(",\n".join(json.dumps(r, sort_keys=True) for r in rows))          # one call per line
        f.write("\n]}\n")
    print(f"{args.out}: {len(rows)} rows from {args.library}")


if __name__ == "__main__":
    main()
