"""CPU-only checks of the recurrence dispatch (csrc/esn_api.hip: plan_recur, the knob table): the size queries
answer what the recorded commit answered over a grid of shapes and knobs (tests/golden/dispatch_sizes.json, written
by tools/record_dispatch_sizes.py), esn_recur_path names the kernel include/esn_hip.h describes, sizes and paths
agree with each other, and every knob parses.  Needs the built library, no GPU."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the grid the golden file must cover, axis by axis
PRECISIONS = ["f64", "f32", "f16", "bf16"]
N_RES = [64, 128, 129, 256, 257, 300, 512, 513, 1024, 1025, 1500, 2048, 2049]
IO = [[2, 2], [3, 2], [4, 4], [16, 8], [16, 16]]
N_WSETS = [1, 3]
FRAMES = [[1, 1], [8, 1], [9, 4], [150, 75], [4096, 64]]
DEFAULTS = {"cluster": "1", "big_gemm": "1", "hcluster": "1", "f64_mfma": "1", "s16": "1", "skew": "1"}
MOVED = [["cluster", "0"], ["big_gemm", "0"], ["hcluster", "0"], ["f64_mfma", "0"], ["s16", "0"], ["skew", "0"]]
# keys of knobs that went with the kernels they selected: unknown like any other
RETIRED = ["rs", "big_pipe", "big_nt", "harvest_gemm"]
WORKSPACE_PATHS = {"cluster_f64", "big_predict", "big_harvest", "harvest_cluster"}


@pytest.fixture(scope="module")
def lib():
    from esn_ofdm_mimo_amd import build, _lib
    build.build_library(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "dispatch_sizes.json")) as f:
        return json.load(f)


class knobs_set:
    """`with knobs_set(lib, key=value, ...)`: the knobs moved, the defaults back afterwards"""

    def __init__(self, _lib, **kv):
        self._lib, self.kv = _lib, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self._lib.debug_set(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self._lib.debug_set(k, DEFAULTS[k])


def grid_shapes():
    for prec in PRECISIONS:
        for n_res in N_RES:
            for n_in, n_out in IO:
                for nw in N_WSETS:
                    yield prec, n_res, n_in, n_out, nw


def test_golden_covers_the_grid(golden):
    g = golden["grid"]
    assert (g["precisions"], g["n_res"], g["io"], g["n_wsets"], g["frames"]) == (PRECISIONS, N_RES, IO, N_WSETS, FRAMES)
    assert g["defaults"] == DEFAULTS and g["moved"] == MOVED
    keys = {"|".join(map(str, s)) for s in grid_shapes()}
    assert set(golden["shape"]) == keys and set(golden["sizes"]) == keys and len(keys) == 520
    assert all(len(v) == len(FRAMES) for v in golden["sizes"].values())
    assert set(golden["diffs"]) == {f"{k}={v}" for k, v in MOVED}
    assert len(golden["commit"]) == 40


def test_size_queries_answer_as_recorded(lib, golden):
    """All 18 200 combinations (520 shapes x 5 batches x default + 6 moved knobs), entry by entry."""
    from esn_ofdm_mimo_amd import _lib
    checked = 0
    for setting in [None] + MOVED:
        diffs = golden["diffs"][f"{setting[0]}={setting[1]}"] if setting else {}
        used = 0
        with knobs_set(_lib, **({setting[0]: setting[1]} if setting else {})):
            for shp in grid_shapes():
                prec, n_res, n_in, n_out, nw = shp
                key = "|".join(map(str, shp))
                p, sh = _lib.PRECISIONS[prec], _lib.Shape(n_res, n_in, n_out, 1, nw, 1.0)
                fixed = [lib.esn_tile_frames(p, C.byref(sh)), lib.esn_packed_weights_bytes(p, C.byref(sh)),
                         lib.esn_packed_readout_bytes(p, C.byref(sh))]
                for i, (nf, f) in enumerate(FRAMES):
                    got = fixed + [lib.esn_predict_workspace_bytes(p, C.byref(sh), nf, f),
                                   lib.esn_harvest_workspace_bytes(p, C.byref(sh), nf)]
                    want = diffs.get(f"{key}|{i}")
                    used += want is not None
                    if want is None:
                        want = golden["shape"][key] + golden["sizes"][key][i]
                    assert got == want, (setting, key, nf, f, got, want)
                    checked += 1
        assert used == len(diffs), setting
    assert checked == 520 * 5 * 7


# (harvest, precision, (n_res, n_in, n_out, n_wsets), n_sequences, F, have_workspace, knobs moved, path), each row
# written from the description of enum esn_path / esn_debug_set in include/esn_hip.h
PATH_TABLE = [
    # fp16/bf16 predict at 257..512 units: the 16x16x32 skewed kernel; "s16" = "0": the 32x32x16 one
    (0, "f16", (512, 16, 8, 1), 150, 75, 1, {}, "skew16"),
    (0, "bf16", (512, 16, 8, 1), 150, 75, 1, {}, "skew16"),
    (0, "f16", (512, 16, 8, 1), 150, 75, 0, {}, "skew16"),
    (0, "f16", (300, 16, 8, 1), 150, 75, 1, {}, "skew16"),
    (0, "f16", (512, 16, 8, 1), 150, 75, 1, {"s16": "0"}, "mfma"),
    (0, "bf16", (512, 16, 8, 1), 150, 75, 1, {"s16": "0"}, "mfma"),
    (0, "f16", (512, 16, 8, 1), 150, 75, 1, {"skew": "0"}, "mfma"),       # the skewed schedule is what skew16 runs
    (0, "f16", (512, 3, 2, 1), 150, 75, 1, {}, "mfma"),                   # n_in not 2/4/8/16
    (0, "f16", (512, 16, 16, 1), 150, 75, 1, {}, "mfma"),                 # n_out > 8
    (0, "f16", (256, 16, 8, 1), 150, 75, 1, {}, "mfma"),
    (0, "f16", (1024, 16, 8, 1), 150, 75, 1, {}, "mfma"),
    (0, "f32", (512, 16, 8, 1), 150, 75, 1, {}, "mfma"),
    # beyond 1024 units, fp16/bf16, one weight set: a GEMM launch per step when a workspace is lent
    (0, "f16", (2048, 16, 8, 1), 150, 75, 1, {}, "big_predict"),
    (0, "bf16", (1500, 4, 4, 1), 150, 75, 1, {}, "big_predict"),
    (0, "f16", (2048, 16, 8, 1), 150, 75, 0, {}, "mfma"),
    (0, "f16", (2048, 16, 8, 1), 150, 75, 1, {"big_gemm": "0"}, "mfma"),
    (0, "f16", (2048, 16, 8, 3), 150, 75, 1, {}, "mfma"),                 # the GEMM paths need one weight set
    (0, "f16", (2048, 16, 16, 1), 150, 75, 1, {}, "mfma"),                # ... and n_out <= 8
    # float64: matrix pipe for batches where its tiling fits (N_res <= 1024), else the vector ALU
    (0, "f64", (512, 16, 8, 1), 150, 75, 1, {}, "f64_mfma"),
    (0, "f64", (512, 16, 8, 1), 150, 75, 0, {}, "f64_mfma"),
    (0, "f64", (512, 16, 8, 1), 150, 75, 1, {"f64_mfma": "0"}, "f64_valu"),
    (0, "f64", (2048, 16, 8, 1), 150, 75, 1, {}, "f64_valu"),
    (0, "f64", (512, 16, 8, 1), 8, 1, 1, {}, "f64_valu"),                 # no more slots than one vector-ALU tile
    # ONE float64 sequence: the cluster kernel when a workspace is lent
    (0, "f64", (512, 16, 8, 1), 1, 1, 1, {}, "cluster_f64"),
    (0, "f64", (512, 16, 8, 1), 1, 1, 0, {}, "f64_valu"),
    (0, "f64", (512, 16, 8, 1), 1, 1, 1, {"cluster": "0"}, "f64_valu"),
    (1, "f64", (512, 16, 8, 1), 1, 1, 1, {}, "cluster_f64"),
    (1, "f64", (512, 16, 8, 1), 150, 1, 1, {}, "f64_mfma"),
    # harvest, fp16/bf16 at 257..512 units: the cluster kernel
    (1, "f16", (512, 16, 8, 1), 70, 1, 1, {}, "harvest_cluster"),
    (1, "bf16", (300, 16, 8, 1), 64, 1, 1, {}, "harvest_cluster"),
    (1, "f16", (512, 16, 8, 1), 70, 1, 0, {}, "mfma"),
    (1, "f16", (512, 16, 8, 1), 70, 1, 1, {"hcluster": "0"}, "mfma"),
    (1, "f16", (256, 16, 8, 1), 70, 1, 1, {}, "mfma"),
    (1, "f16", (2048, 16, 8, 1), 70, 1, 1, {}, "big_harvest"),
    (1, "f16", (2048, 16, 8, 1), 70, 1, 0, {}, "mfma"),
    (1, "f16", (2048, 16, 8, 1), 70, 1, 1, {"big_gemm": "0"}, "mfma"),
    (1, "f16", (2048, 16, 8, 3), 70, 1, 1, {}, "mfma"),
    (1, "f32", (512, 16, 8, 1), 70, 1, 1, {}, "mfma"),
]


@pytest.mark.parametrize("harvest,prec,shape,n,f,have_ws,moved,want", PATH_TABLE)
def test_recur_path_table(lib, harvest, prec, shape, n, f, have_ws, moved, want):
    from esn_ofdm_mimo_amd import _lib
    n_res, n_in, n_out, nw = shape
    sh = _lib.Shape(n_res, n_in, n_out, 1, nw, 1.0)
    with knobs_set(_lib, **moved):
        assert _lib.recur_path(harvest, prec, sh, n, f, have_ws) == want
        size = (lib.esn_harvest_workspace_bytes(_lib.PRECISIONS[prec], C.byref(sh), n) if harvest else
                lib.esn_predict_workspace_bytes(_lib.PRECISIONS[prec], C.byref(sh), n, f))
    if want in WORKSPACE_PATHS:
        assert size > 0            # a path that reads a workspace advertises one


def test_recur_path_errors(lib):
    from esn_ofdm_mimo_amd import _lib
    ok, bad = _lib.Shape(512, 16, 8, 1, 1, 1.0), _lib.Shape(0, 16, 8, 1, 1, 1.0)
    assert lib.esn_recur_path(0, _lib.F16, C.byref(bad), 1, 1, 1) == -1 and b"invalid shape" in lib.esn_last_error()
    assert lib.esn_recur_path(0, _lib.F32, C.byref(_lib.Shape(2048, 16, 8, 1, 1, 1.0)), 1, 1, 1) == -2
    assert lib.esn_recur_path(0, _lib.F16, C.byref(ok), 0, 1, 1) == -1 and b"invalid sizes" in lib.esn_last_error()
    assert lib.esn_recur_path(0, _lib.F16, C.byref(ok), 4, 0, 1) == -1
    assert lib.esn_recur_path(1, _lib.F16, C.byref(ok), 4, 0, 1) >= 0          # harvest ignores frames_per_group
    leaky = _lib.Shape(512, 16, 8, 1, 1, 0.5)
    assert lib.esn_recur_path(0, _lib.F16, C.byref(leaky), 4, 1, 1) == -2 and b"leak_rate" in lib.esn_last_error()
    # the size queries keep failing under their own names
    assert lib.esn_predict_workspace_bytes(_lib.F16, C.byref(leaky), 4, 1) == 0
    assert lib.esn_last_error().startswith(b"esn_predict_workspace_bytes: leak_rate")
    assert lib.esn_harvest_workspace_bytes(_lib.F16, C.byref(leaky), 4) == 0
    assert lib.esn_last_error().startswith(b"esn_harvest_workspace_bytes: leak_rate")


def test_sizes_and_paths_agree(lib):
    """Over the whole grid: a size query answers > 0 exactly when the call, lent a workspace, takes one of the four
    paths that read it, and a call without a workspace never takes one.  ONE exception, kept from before the plan
    existed: with big_gemm = "0" the sizes of big_predict / big_harvest are still advertised while the persistent
    kernel serves the call."""
    from esn_ofdm_mimo_amd import _lib

    def walk():
        out = {}
        for shp in grid_shapes():
            prec, n_res, n_in, n_out, nw = shp
            p, sh = _lib.PRECISIONS[prec], _lib.Shape(n_res, n_in, n_out, 1, nw, 1.0)
            served = lib.esn_tile_frames(p, C.byref(sh)) > 0
            for nf, f in FRAMES:
                for harvest in (0, 1):
                    size = (lib.esn_harvest_workspace_bytes(p, C.byref(sh), nf) if harvest else
                            lib.esn_predict_workspace_bytes(p, C.byref(sh), nf, f))
                    if not served:
                        assert size == 0 and lib.esn_recur_path(harvest, p, C.byref(sh), nf, f, 1) == -2, shp
                        continue
                    with_ws = _lib.recur_path(harvest, prec, sh, nf, f, True)
                    without = _lib.recur_path(harvest, prec, sh, nf, f, False)
                    assert without not in WORKSPACE_PATHS, (shp, nf, f, harvest, without)
                    out[shp, nf, f, harvest] = (size, with_ws, without)
        return out

    base = walk()
    assert len(base) > 4000
    for where, (size, with_ws, without) in base.items():
        assert (size > 0) == (with_ws in WORKSPACE_PATHS), (where, size, with_ws)
    for k, v in MOVED:
        with knobs_set(_lib, **{k: v}):
            moved = walk()
        for where, (size, with_ws, without) in moved.items():
            if k == "big_gemm" and base[where][1] in ("big_predict", "big_harvest"):
                # the exception: size as with big_gemm = "1", path as without a workspace
                assert size == base[where][0] > 0 and with_ws == without, (where, size, with_ws, without)
            else:
                assert (size > 0) == (with_ws in WORKSPACE_PATHS), (k, v, where, size, with_ws)


# every knob: key -> spellings esn_debug_set accepts (None = NULL: back to the default)
KNOB_SPELLINGS = {
    "skew": ["0", "1", None], "chol_dma": ["0", "1", None], "f64_mfma": ["0", "1", None],
    "big_gemm": ["0", "1", None], "cluster": ["0", "1", None], "s16": ["0", "1", None],
    "mfma_geom": ["8,2,4", "junk", None], "mfma_geom_f32": ["8,2,2", None],
    "chol_skip": ["3", "0", None], "gen_ko": ["5", "0", None],
    "hcluster": ["0", "4", "8", "1", None],
}


def test_every_knob_parses(lib):
    from esn_ofdm_mimo_amd import _lib
    enc = lambda v: None if v is None else v.encode()
    try:
        for key, values in KNOB_SPELLINGS.items():
            for v in values:
                assert lib.esn_debug_set(key.encode(), enc(v)) == 0, (key, v)
    finally:
        for key in KNOB_SPELLINGS:
            lib.esn_debug_set(key.encode(), None)
    assert lib.esn_debug_set(b"nope", b"1") == -1
    assert lib.esn_last_error() == b"esn_debug_set: unknown key 'nope'"
    assert lib.esn_debug_set(None, b"1") == -1 and lib.esn_last_error() == b"esn_debug_set: null key"
    for key in RETIRED:
        assert lib.esn_debug_set(key.encode(), b"1") == -1, key
        assert lib.esn_last_error() == b"esn_debug_set: unknown key '" + key.encode() + b"'"
    # the header documents every key of the table
    doc = open(os.path.join(ROOT, "include", "esn_hip.h")).read()
    for key in KNOB_SPELLINGS:
        assert f'"{key}"' in doc, key
        if key != "gen_ko":
            assert "ESN_" + key.upper() in doc, key
    # the parse rule seen through the plan: on unless "0" (hcluster's "4" / "8" once chose the members of a cluster)
    sh = _lib.Shape(512, 16, 8, 1, 1, 1.0)
    for v, want in (("2", "skew16"), ("0", "mfma"), (None, "skew16")):
        with knobs_set(_lib, s16=v):
            assert _lib.recur_path(False, "f16", sh, 150, 75) == want, v
    for v, want in (("2", 163904), ("1", 163904), ("4", 163904), ("8", 163904), (None, 163904), ("0", 0)):      # pairs: ceil(70 / 16) * 32768 + 64
        with knobs_set(_lib, hcluster=v):
            assert lib.esn_harvest_workspace_bytes(_lib.F16, C.byref(sh), 70) == want, v
