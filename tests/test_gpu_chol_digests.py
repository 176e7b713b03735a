"""The Cholesky read-out solve (readout_chol_kernel, readout_chol_big_kernel) writes, over the smallest shapes at
which its diagonal-block factorisation can go wrong, exactly the W_out and status bytes that the commit named in
tests/golden/chol_parent_digests.json wrote: the DPP form of the factorisation -- and any later rewrite that is meant
to keep the results -- changes no output bit.  The sample and the inputs are those of tools/record_chol_digests.py
(one tile and ragged tiles, wide and tall, the residency tail, a rejected pivot by a duplicated row, a zero row and a
duplicated column, the ridge instances, the workspace kernel, the W_out passes that cols 528 and 60 never take, the
workspace kernel's ridge instance, exactly-zero pivot, idle substitution waves and full 512 rows; float64 and float32 E).  Every status is 0 except the
singular group of the rejected-pivot cases, which is 1."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_chol_digests", os.path.join(ROOT, "tools", "record_chol_digests.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

CASES = rec.cases()
with open(rec.GOLDEN) as _f:
    DOC = json.load(_f)


def test_sample_is_the_recorded_one():
    """(no GPU) the golden file was recorded over the cases the tool builds today"""
    assert DOC["seed"] == rec.SEED and DOC["transient"] == rec.TRANSIENT
    assert [d[0] for d in DOC["digests"]] == [c["id"] for c in CASES]
    assert len(DOC["commit"]) >= 7


def test_sample_covers_what_the_factorisation_can_get_wrong():
    """(no GPU) the shapes, both E types, the three ways to a rejected pivot, both ridge values, the workspace kernel"""
    key = {(c["kind"], c["rows"], c["cols"], c["n_out"], c["G"], c["e32"], c["drop"], c["ridge"]) for c in CASES}
    for e32 in (False, True):
        for n in (16, 17, 100, 127, 128):
            assert ("wide", n, 528, 8, 3, e32, None, None) in key
        assert ("wide", 40, 60, 3, 3, e32, None, None) in key
        for r, c in ((300, 100), (140, 37), (512, 128)):
            assert ("tall", r, c, 8, 3, e32, None, None) in key
        assert ("tail", 128, 528, 8, 5, e32, None, None) in key
        for drop, r, c in (("row", 128, 528), ("zero", 128, 528), ("col", 300, 100)):
            assert ("drop", r, c, 8, 5, e32, drop, None) in key
        for r, c in ((100, 528), (300, 100)):
            for lam in (0.0, 1e-3):
                assert ("ridge", r, c, 8, 3, e32, None, lam) in key
        for r, c in ((144, 528), (130, 200), (600, 144)):
            assert ("big", r, c, 8, 2, e32, None, None) in key
        for r, c, o in ((40, 61, 3), (20, 600, 8), (20, 800, 8)):
            assert ("wide", r, c, o, 3, e32, None, None) in key
        for r, c in ((144, 528), (600, 144)):
            for lam in (0.0, 1e-3):
                assert ("big-ridge", r, c, 8, 2, e32, None, lam) in key
        assert ("big-drop", 144, 528, 8, 5, e32, "zero", None) in key
        assert ("big-drop", 600, 144, 8, 5, e32, "zerocol", None) in key
        for r, c, o in ((130, 200, 3), (129, 528, 8), (512, 528, 8)):
            assert ("big", r, c, o, 2, e32, None, None) in key
    assert ("tail", 128, 528, 8, 513, True, None, None) in key


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{i:02d}-{c['id']}" for i, c in enumerate(CASES)])
def test_output_bytes_match_recorded_digest(i):
    c = CASES[i]
    name, want_w, want_s = DOC["digests"][i]
    assert name == c["id"]
    w, s, status = rec.digests(i, c)
    assert status == rec.expected_status(c), f"{c['id']}: status {status}"
    assert s == want_s, f"{c['id']}: status bytes differ from commit {DOC['commit']}"
    assert w == want_w, f"{c['id']}: W_out bytes differ from commit {DOC['commit']}"
