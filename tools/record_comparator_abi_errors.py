"""Records what the eight comparator entry points of libesn_hip.so (esn_elm_features, esn_elm_predict and the train /
predict pairs of the FNN, the CNN and the LSTM) answer to calls they must refuse -- the return code and the full
esn_last_error() text -- and what the three workspace queries answer over a grid of shapes, into
tests/golden/comparator_abi_errors.json, for tests/test_comparator_abi_table_cpu.py to replay: a rewrite of the argument
checks that is meant to keep their answers keeps every code, every byte of every message and which check fires first.
Needs no GPU.

    python tools/record_comparator_abi_errors.py <tree of the commit to pin>/esn_ofdm_mimo_amd/libesn_hip.so --commit <hash>

Every row is refused by the argument checks of esn_api.hip themselves, before any launcher or device call: the pointers
are small integers that are never valid.  Per entry point, where it has the argument: each mandatory pointer null in
turn; n_in 0 and 65; channels / n_hidden one above the limit; n_out 0 and 9; kernel 2 and 9; window 0 and 17;
window * n_in 257; T 4097 (the ELM's checks: 2^20 + 1); T_in > T; transient -1 and T; n_groups / n_frames 0;
frames_per_group 0; n_wsets / n_isets 0; epochs 0; lr -1 and NaN, beta1 1, beta2 -0.1, eps 0; precision ESN_F32,
ESN_F16, ESN_BF16 and 99; the workspace null, one byte short and at address 68; Y (E) at address 72; the FNN's three
size limits and its LDS limit; the ELM's bias_col and e_cols ranges; and the rows of PAIRS with two faults at once, which
pin the order of the checks.  Left out, because the checks let them through to a launcher: n_in 65 for the ELM and the
FNN (no limit but window * n_in), T 4097 for them (the FNN's training meets its LDS limit first, recorded as such),
ESN_F16 for esn_elm_predict and esn_fnn_predict (served), Y at address 72 for esn_cnn_predict and esn_lstm_predict (any
alignment is served)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "comparator_abi_errors.json")
SCALINGS = ["in_scale", "in_shift", "t_scale", "t_shift"]
ADAM = ["epochs", "lr", "beta1", "beta2", "eps"]
WORK = ["workspace", "workspace_bytes", "stream"]
SEQ = ["n_groups", "T_in", "T", "transient", "group_offset"]
FRAMES = ["n_frames", "frames_per_group", "T_in", "T", "transient"]
FNN_SET, CNN_SET = ["W1", "b1", "W2", "b2"], ["W1", "b1", "W2", "b2", "W3", "b3"]
LSTM_SET = ["W_ih", "W_hh", "b_ih", "b_hh", "W_fc", "b_fc"]


def _pair(head, names, query):
    """(train, predict) parameter lists of an Adam-trained comparator whose sizes are `head` and arrays `names`."""
    init = [n + "_0" for n in names]
    train = (["precision"] + head + ["n_isets"] + init + SCALINGS + ["U", "D"] + SEQ + ADAM + names + ["loss"] + WORK,
             init + ["U", "D"] + names, query)
    work = WORK if query != "esn_fnn_workspace_bytes" else ["stream"]
    predict = (["precision"] + head + names + SCALINGS + ["U"] + FRAMES + ["Y"] + work, names + ["U", "Y"],
               query if len(work) > 1 else None)
    return train, predict


# entry point -> (parameter names in order, mandatory pointers, workspace query or None)
ENTRY_POINTS = {
    "esn_elm_features": (["precision", "n_in", "n_hidden", "window", "bias_col", "n_wsets", "W_in", "b", "in_scale",
                          "in_shift", "U", "n_groups", "T_in", "T", "group_offset", "E", "e_f32", "e_cols", "stream"],
                         ["W_in", "b", "U", "E"], None),
    "esn_elm_predict": (["precision", "n_in", "n_hidden", "window", "bias_col", "n_wsets", "n_out", "W_in", "b", "W_out",
                         "e_cols"] + SCALINGS + ["U"] + FRAMES + ["group_offset", "Y", "stream"],
                        ["W_in", "b", "W_out", "U", "Y"], None),
}
for _name, _head, _set in (("fnn", ["n_in", "n_hidden", "window", "n_out"], FNN_SET),
                           ("cnn", ["n_in", "c1", "c2", "n_out", "kernel"], CNN_SET),
                           ("lstm", ["n_in", "n_hidden", "n_out"], LSTM_SET)):
    ENTRY_POINTS[f"esn_{_name}_train"], ENTRY_POINTS[f"esn_{_name}_predict"] = _pair(_head, _set,
                                                                                    f"esn_{_name}_workspace_bytes")
# workspace query -> its parameter names
QUERIES = {"esn_fnn_workspace_bytes": ["n_in", "n_hidden", "window", "n_out", "n_groups", "T"],
           "esn_cnn_workspace_bytes": ["n_in", "c1", "c2", "n_out", "kernel", "n_groups", "n_frames", "T"],
           "esn_lstm_workspace_bytes": ["n_in", "n_hidden", "n_out", "n_groups", "n_frames", "T"]}
PTR, ODD, ODD4 = 64, 72, 68          # 16-byte aligned, only 8-byte aligned, only 4-byte aligned: none is ever valid
F64, F32, F16, BF16 = 0, 1, 2, 3
SIZES = dict(precision=F64, n_in=4, n_hidden=17, window=3, bias_col=1, n_wsets=2, n_out=3, e_cols=18, e_f32=0, c1=7, c2=19,
             kernel=3, n_isets=2, n_groups=2, n_frames=7, frames_per_group=5, T_in=19, T=23, transient=2, group_offset=1,
             epochs=10, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8)
OPTIONAL = SCALINGS + ["loss", "stream"]
CHANNEL_LIMITS = {"esn_elm": dict(n_hidden=1025), "esn_fnn": dict(n_hidden=1025), "esn_cnn": dict(c1=129, c2=129),
                  "esn_lstm": dict(n_hidden=129)}
# two faults at once: (label, changes); a row is recorded for every entry point that has all the changed arguments
PAIRS = [
    ("null U, n_out = 9", dict(U=None, n_out=9)),
    ("epochs = 0, n_hidden above the limit", dict(epochs=0, n_hidden=1025)),
    ("epochs = 0, c1 = 129", dict(epochs=0, c1=129)),
    ("precision 99, workspace one byte short", dict(precision=99, short=1)),
    ("n_out = 9, precision ESN_F32", dict(n_out=9, precision=F32)),
    ("n_isets = 0, lr = -1", dict(n_isets=0, lr=-1.0)),
    ("transient = T, null workspace", dict(transient=SIZES["T"], workspace=None)),
    ("frames_per_group = 0, n_in = 0", dict(frames_per_group=0, n_in=0)),
    ("precision ESN_F32, transient = -1", dict(precision=F32, transient=-1)),
    ("lr NaN, T_in > T", dict(lr="nan", T_in=SIZES["T"] + 1)),
    ("n_groups = 0, null workspace", dict(n_groups=0, workspace=None)),
    ("precision ESN_BF16, window = 17", dict(precision=BF16, window=17)),
]
# the grid of the workspace queries: refused shapes (which answer 0) among served ones
QUERY_GRID = [dict(), dict(n_groups=0), dict(n_frames=0), dict(n_groups=0, n_frames=0), dict(n_groups=-1),
              dict(n_frames=-1),
              dict(n_in=0), dict(n_in=64), dict(n_in=65), dict(n_hidden=0), dict(n_hidden=100), dict(n_hidden=128),
              dict(n_hidden=129), dict(c1=128, c2=128), dict(c1=129), dict(c2=0), dict(n_out=0), dict(n_out=8), dict(n_out=9),
              dict(kernel=2), dict(kernel=7), dict(kernel=9), dict(window=0), dict(window=16), dict(T=1), dict(T=4096),
              dict(T=4097), dict(T=0), dict(n_groups=4096, n_frames=65536, T=138)]


def open_library(path):
    from esn_ofdm_mimo_amd import _lib
    lib = C.CDLL(path)
    for name in ["esn_last_error", "esn_abi_version"] + list(ENTRY_POINTS) + list(QUERIES):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def query_args(query, v):
    """The arguments of a workspace query for the sizes in v (a training has no frames, a prediction no groups)."""
    return [v.get(p, 0) for p in QUERIES[query]]


def cases(lib):
    """[(entry point, case label, argument list)], None for a null pointer; `lib` answers the workspace queries."""
    out = []
    for name, (params, mandatory, query) in ENTRY_POINTS.items():
        family = name[:name.index("_", 4)]
        base = {p: SIZES.get(p, PTR) for p in params}
        base.update({p: None for p in OPTIONAL if p in params})

        def row(label, short=0, **change):
            if not set(change) <= set(params) or (short and "workspace_bytes" not in params):
                return
            v = dict(base, **change)
            if "workspace_bytes" in params:         # what the query says for the row's sizes (0 at a refused shape)
                v["workspace_bytes"] = getattr(lib, query)(*query_args(query, v)) - short
            out.append((name, label, [v[p] for p in params]))

        for p in mandatory:
            row(f"null {p}", **{p: None})
        row("n_in = 0", n_in=0)
        if family in ("esn_cnn", "esn_lstm"):
            row("n_in = 65", n_in=65)
            row("T = 4097", T=4097)
        else:
            row("T = 2^20 + 1", T=(1 << 20) + 1)
        for p, above in CHANNEL_LIMITS[family].items():
            row(f"{p} = {above}", **{p: above})
        for p, values in (("n_out", (0, 9)), ("kernel", (2, 9)), ("window", (0, 17)), ("transient", (-1, SIZES["T"])),
                          ("n_groups", (0,)), ("n_frames", (0,)), ("frames_per_group", (0,)), ("n_wsets", (0,)),
                          ("n_isets", (0,)), ("epochs", (0,)), ("lr", (-1.0, "nan")), ("beta1", (1.0,)), ("beta2", (-0.1,)),
                          ("eps", (0.0,)), ("bias_col", (2,)), ("e_cols", (17, 22))):
            for value in values:
                row(f"{p} = {value}", **{p: value})
        row("window * n_in = 257", window=1, n_in=257)
        row("T_in > T", T_in=SIZES["T"] + 1)
        for precision, label in ((F32, "ESN_F32"), (F16, "ESN_F16"), (BF16, "ESN_BF16"), (99, "99")):
            if not (precision == F16 and name in ("esn_elm_predict", "esn_fnn_predict")):
                row("precision " + label, precision=precision)
        row("null workspace", workspace=None)
        row("workspace one byte short", short=1)
        row("workspace at 68", workspace=ODD4)
        row("E at 72", E=ODD)
        if family in ("esn_elm", "esn_fnn"):
            row("Y at 72", Y=ODD)
        if name == "esn_fnn_train":
            row("n_hidden = 513", n_hidden=513)
            row("n_out n_hidden = 1025", n_out=5, n_hidden=205)
            row("ceil(n_hidden / 4) ceil(K / 8) = 513", n_hidden=108, window=8, n_in=19)
            row("LDS limit", n_hidden=100, window=8, T_in=20000, T=20000)
        for label, change in PAIRS:
            row(label, **change)
    return out


def queries(lib):
    """[(workspace query, argument list)] over QUERY_GRID, each shape once per query."""
    out = []
    for query in QUERIES:
        for change in QUERY_GRID:
            a = query_args(query, dict(SIZES, **change))
            if set(change) <= set(QUERIES[query]) and (query, a) not in out:
                out.append((query, a))
    return out


def answer(lib, name, args):
    rc = getattr(lib, name)(*[float("nan") if a == "nan" else a for a in args])
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
    sizes = [{"fn": q, "args": a, "bytes": getattr(lib, q)(*a)} for q, a in queries(lib)]
    with open(args.out, "w") as f:
        f.write('{"abi": %d, "commit": %s, "rows": [\n' % (lib.esn_abi_version(), json.dumps(args.commit)))
        f.write(",\n".join(json.dumps(r, sort_keys=True) for r in rows))          # one call per line
        f.write('\n], "queries": [\n')
        f.write(",\n".join(json.dumps(r, sort_keys=True) for r in sizes))
        f.write("\n]}\n")
    print(f"{args.out}: {len(rows)} rows and {len(sizes)} workspace sizes from {args.library}")


if __name__ == "__main__":
    main()
