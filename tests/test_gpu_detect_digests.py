"""The detector tail writes, over the sample of tools/record_detect_digests.py, exactly the err, bits and X_hat bytes
that the commit named in tests/golden/detect_parent_digests.json wrote -- under detect_fixed "0" (the generic kernel:
moving its arithmetic into the shared helpers changed no bit) and under "1" (the fixed-shape instance is bitwise that
commit's kernel)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_detect_digests", os.path.join(ROOT, "tools", "record_detect_digests.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

CASES = rec.cases()
with open(rec.GOLDEN) as _f:
    DOC = json.load(_f)


def test_sample_is_the_recorded_one():
    """(no GPU) the golden file was recorded over the cases the tool builds today"""
    assert DOC["seed"] == rec.SEED and DOC["frames_per_workgroup"] == rec.K
    assert [d[0] for d in DOC["digests"]] == [c["id"] for c in CASES]
    assert len(DOC["commit"]) >= 7


@pytest.mark.gpu
@pytest.mark.parametrize("knob", ("1", "0"), ids=("fixed", "generic"))
@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{i:02d}-{c['id']}" for i, c in enumerate(CASES)])
def test_output_bytes_match_recorded_digest(i, knob):
    from esn_ofdm_mimo_amd import _lib
    c = CASES[i]
    name, *want = DOC["digests"][i]
    assert name == c["id"]
    try:
        _lib.debug_set("detect_fixed", knob)
        got = rec.digests(i, c)
    finally:
        _lib.debug_set("detect_fixed", "1")
    for what, g, w in zip(("err", "bits", "X_hat"), got, want):
        assert g == w, f"{c['id']}: {what} bytes differ from commit {DOC['commit']} under detect_fixed={knob}"
