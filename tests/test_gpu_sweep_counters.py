"""The Monte-Carlo harness computes what the commit named in tests/golden/sweep_parent_counters.json computed: for one
small sweep per constructor arm and per branch of a chunk, and for the two coded comparison points, every counter,
fits_repaired, the bytes of W_out and the per-candidate, per-symbol and cache-hit counts are equal entry for entry, and
so are the per-block counters of the seven uncoded comparison points over one full and one short chunk
(cases and recorder: tools/record_sweep_counters.py).  Each sweep and each point runs once."""
import functools
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_sweep_counters",
                                               os.path.join(ROOT, "tools", "record_sweep_counters.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

NAMES = list(rec.CASES) + [rec.POINTS_CASE] + list(rec.POINT_CASES)


@functools.lru_cache(maxsize=None)
def golden():
    with open(rec.GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def record(name):
    return rec.record(name)


def test_the_golden_file_names_its_commit_and_every_case():
    doc = golden()
    assert len(doc["commit"]) >= 7 and doc["seed"] == rec.SEED
    assert sorted(doc["cases"]) == sorted(NAMES) and sorted(doc["host_draw_sha256"]) == sorted(rec.HOST_DRAWN)


@pytest.mark.parametrize("name", NAMES)
def test_case_gives_the_recorded_entries(name):
    doc = golden()
    if name in rec.HOST_DRAWN:
        assert rec.host_draw_digest(name) == doc["host_draw_sha256"][name], \
            "host draw differs from the recording machine: re-record on the parent"
    got, want = record(name), doc["cases"][name]
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], f"{name}: {key} differs from commit {doc['commit']}"


def test_fresh_radius_cache_serves_the_second_point_and_changes_nothing():
    cached, plain, split = record("fresh_cache"), record("fresh_no_cache"), record("fresh_f16x2")
    assert cached["fresh_radius_hits"] == rec.BLOCKS and plain["fresh_radius_hits"] == 0
    assert cached["counters"] == plain["counters"] and cached["w_out_sha256"] == plain["w_out_sha256"]
    assert split["fresh_radius_hits"] == rec.BLOCKS
