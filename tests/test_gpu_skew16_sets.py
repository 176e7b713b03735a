"""The 16x16x32 skewed predict kernel (esn_recur_skew16_impl.h) writes, over a covering sample of its shapes, exactly
the bytes that the commit named in tests/golden/skew16_parent_digests.json wrote: the per-wave-set bodies of the
step loop -- and any later rewrite that is meant to keep the results -- change no output bit.  The sample and the
inputs are those of tools/record_skew16_digests.py (f16 / bf16, three noise modes, float64 / float32 I/O, n_in, n_out,
N_res, frames per group, groups, weight sets, transient, initial state, ragged last group, steps past the inputs)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_skew16_digests", os.path.join(ROOT, "tools", "record_skew16_digests.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

CASES = rec.cases()
with open(rec.GOLDEN) as _f:
    DOC = json.load(_f)


def test_sample_is_the_recorded_one():
    """(no GPU) the golden file was recorded over the grid the tool builds today"""
    assert DOC["seed"] == rec.SEED
    assert DOC["axes"] == {k: list(v) for k, v in rec.AXES.items()}
    assert [d[0] for d in DOC["digests"]] == [c["id"] for c in CASES]
    assert len(DOC["commit"]) >= 7


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{i:02d}-{c['id']}" for i, c in enumerate(CASES)])
def test_output_bytes_match_recorded_digest(i):
    c = CASES[i]
    name, want = DOC["digests"][i]
    assert name == c["id"]
    assert rec.digest(i, c) == want, f"{c['id']}: output bytes differ from commit {DOC['commit']}"
