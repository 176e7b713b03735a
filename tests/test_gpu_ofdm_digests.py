"""The OFDM kernels -- decide and re-modulate, the generic detector tail, the LS/MMSE baseline, the channel tracker, taps
to frequency, the frame generator and the LLRs -- write, over the sample of tools/record_ofdm_digests.py, exactly the
bytes that the commit named in tests/golden/ofdm_parent_digests.json wrote: moving their transform, grid and counter
arithmetic into csrc/esn_ofdm_math.h changed no bit of any output tensor."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_ofdm_digests", os.path.join(ROOT, "tools", "record_ofdm_digests.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

CASES = rec.cases()
with open(rec.GOLDEN) as _f:
    DOC = json.load(_f)


def test_sample_is_the_recorded_one():
    """(no GPU) the golden file was recorded over the cases the tool builds today"""
    assert DOC["seed"] == rec.SEED
    assert [d[0] for d in DOC["digests"]] == [c["id"] for c in CASES]
    assert all(len(h) == 64 for _, d in DOC["digests"] for h in d.values())
    assert len(DOC["commit"]) >= 7


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{i:03d}-{c['id']}" for i, c in enumerate(CASES)])
def test_output_bytes_match_recorded_digest(i):
    c = CASES[i]
    name, want = DOC["digests"][i]
    assert name == c["id"]
    got = rec.digests(i, c)
    assert sorted(got) == sorted(want)
    for what in want:
        assert got[what] == want[what], f"{c['id']}: {what} bytes differ from commit {DOC['commit']}"
