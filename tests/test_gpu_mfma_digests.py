"""The MFMA recurrence kernel (esn::recur_mfma_kernel: skewed 32x32x16 predict schedule, in-step predict schedule, in-step
harvest) writes, over a covering sample of its shapes, exactly the bytes that the commit named in
tests/golden/mfma_parent_digests.json wrote: a clean-up or rewrite of the kernel that is meant to keep the results
changes no output bit.  The sample and the inputs are those of
tools/record_mfma_digests.py (predict Y / harvest E, f32 / f16 / bf16, three noise modes, float64 / float32 output, one
N_res per row of the tiling table, both schedules, n_in, n_out, frames per group, groups, weight sets, transient, initial
state, ragged last group, steps past the inputs, input gain)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_mfma_digests", os.path.join(ROOT, "tools", "record_mfma_digests.py"))
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


def test_every_case_reaches_the_kernel():
    """(no GPU) under its knobs every case dispatches to this kernel, with and without a workspace lent; and the sample
    holds both schedules of a skew-eligible half-precision predict"""
    for c in CASES:
        assert rec.paths(c) == ("mfma", "mfma"), c["id"]
    assert {c["schedule"] for c in CASES if rec.skew_eligible(c)} == set(rec.AXES["schedule"])


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{i:03d}-{c['id']}" for i, c in enumerate(CASES)])
def test_output_bytes_match_recorded_digest(i):
    c = CASES[i]
    name, want = DOC["digests"][i]
    assert name == c["id"]
    assert rec.digest(i, c) == want, f"{c['id']}: output bytes differ from commit {DOC['commit']}"
