"""The solve of the running normal equations (gram_solve_kernel) writes, over the sample of
tools/record_gram_solve_digests.py, exactly the W_out and status bytes that the commit named in
tests/golden/gram_solve_parent_digests.json wrote: moving its factorisation and substitutions into code shared with
readout_chol_big_kernel -- and any later rewrite that is meant to keep the results -- changes no output bit.  The state
is built on the host (the accumulate kernel is not in the digest); the sample holds a ragged tile, one exact tile, one
column past a tile, more right-hand sides than waves, the ninth row slot of a lane, the limit (cols 544, 16 outputs), a
pivot that is exactly zero at lambda 0 and invalid lambdas."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_gram_solve_digests",
                                               os.path.join(ROOT, "tools", "record_gram_solve_digests.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

CASES = rec.cases()
with open(rec.GOLDEN) as _f:
    DOC = json.load(_f)


def test_sample_is_the_recorded_one():
    """(no GPU) the golden file was recorded over the cases the tool builds today"""
    assert DOC["seed"] == rec.SEED
    assert [d[0] for d in DOC["digests"]] == [c["id"] for c in CASES]
    assert len(DOC["commit"]) >= 7


def test_sample_covers_what_the_solve_can_get_wrong():
    """(no GPU) the shapes, the flagged entries and a lambda per group and candidate"""
    key = [(c["cols"], c["n_out"], c["L"], c["special"]) for c in CASES]
    assert key == [(5, 1, 1, None), (16, 2, 2, None), (17, 4, 2, None), (132, 9, 3, None), (528, 8, 2, None),
                   (544, 16, 1, None), (132, 8, 2, "zero_pivot"), (17, 4, 3, "bad_lambda")]
    assert rec.G == 3
    assert rec.expected_status(CASES[6]) == [[0, 0], [1, 0], [0, 0]]
    assert rec.expected_status(CASES[7]) == [[0, 2, 2]] * 3
    Gm, Cm, lam = rec.arrays(3, CASES[3])
    assert Gm.shape == (3, 132, 132) and Cm.shape == (3, 9, 132) and lam.shape == (3, 3)
    assert sorted(lam[0]) == [132 * s for s in rec.LAMBDA_SCALES] and len({tuple(r) for r in lam}) == 3
    assert (Gm == Gm.transpose(0, 2, 1)).all()                  # symmetric bit for bit, as the accumulate kernel leaves it
    Gz = rec.arrays(6, CASES[6])[0]
    assert not Gz[1, 7].any() and not Gz[1, :, 7].any() and Gz[0, 7, 7] > 0


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
