"""The 16x16x32 skewed predict kernel (esn_recur_skew16_impl.h) writes, at the bench's own launch shape cut down to 40
groups, exactly the bytes that the commit named in tests/golden/skew16_bench_shape_digests.json wrote.  The covering
sample of tests/test_gpu_skew16_sets.py stops at 11 groups and 24 steps; here 25 workgroups run 138 steps over groups of
75 frames that straddle workgroup boundaries, with and without an initial state (the prologue's two paths), in f16 and
bf16 with float64 and float32 I/O, and once with inputs that end before the steps do.  Cases and inputs are those of
tools/record_skew16_bench_digests.py."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_skew16_bench_digests",
                                               os.path.join(ROOT, "tools", "record_skew16_bench_digests.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

CASES = rec.cases()
with open(rec.GOLDEN) as _f:
    DOC = json.load(_f)


def test_cases_are_the_recorded_ones():
    """(no GPU) the golden file was recorded over the cases the tool builds today, and they are the bench's shape"""
    assert DOC["seed"] == rec.SEED and DOC["shape"] == rec.SHAPE and DOC["t_in_short"] == rec.T_IN_SHORT
    assert [d[0] for d in DOC["digests"]] == [c["id"] for c in CASES]
    assert len(DOC["commit"]) >= 7
    s = rec.SHAPE
    assert (s["n_res"], s["n_in"], s["n_out"], s["F"], s["T"], s["transient"], s["noise_mode"]) == (512, 16, 8, 75, 138, 10, "counter")
    f_pad = -(-s["F"] // 16) * 16
    assert s["G"] == 40 and f_pad - s["F"] == 5 and s["G"] * f_pad == 25 * 128 and 128 % f_pad != 0
    seen = {(c["precision"], c["io"], c["init"]) for c in CASES if c["t_in"] == s["T"]}
    assert seen == {(p, io, i) for p in ("f16", "bf16") for io in ("f64", "f32") for i in (False, True)}
    assert sum(c["t_in"] < s["T"] for c in CASES) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{i}-{c['id']}" for i, c in enumerate(CASES)])
def test_output_bytes_match_recorded_digest(i):
    c = CASES[i]
    name, want = DOC["digests"][i]
    assert name == c["id"]
    assert rec.digest(i, c) == want, f"{c['id']}: output bytes differ from commit {DOC['commit']}"
