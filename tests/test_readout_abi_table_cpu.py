"""The argument checks of the eight read-out solve entry points (QR, Cholesky, leave-one-out; pinv and ridge; float64
and float32 E) answer every refused call of tests/golden/readout_abi_errors.json with the return code and the
esn_last_error() text, byte for byte, that the commit named there gave: the entry points share one validator, and each
keeps its own answers.  Every row is refused before any launcher or device call (tools/record_readout_abi_errors.py
says which candidate rows were left out for that reason), so no GPU is needed and none is touched."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_readout_abi_errors",
                                               os.path.join(ROOT, "tools", "record_readout_abi_errors.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(rec.GOLDEN) as _f:
    DOC = json.load(_f)
ROWS = DOC["rows"]


@pytest.fixture(scope="module")
def lib():
    from esn_ofdm_mimo_amd import _lib
    return _lib.load()


def test_table_is_the_one_the_tool_builds(lib):
    """the recorded calls are today's sample (the workspace sizes in them are what today's queries say)"""
    assert DOC["abi"] == lib.esn_abi_version() == 10 and len(DOC["commit"]) >= 7
    assert [(r["fn"], r["case"], r["args"]) for r in ROWS] == [(n, c, a) for n, c, a in rec.cases(lib)]


def test_table_covers_every_entry_point_and_stage():
    by_fn = {}
    for r in ROWS:
        by_fn.setdefault(r["fn"], []).append(r)
    assert sorted(by_fn) == sorted(rec.ENTRY_POINTS)
    for name, rows in by_fn.items():
        labels = {r["case"] for r in rows}
        assert {f"null {p}" for p in rec.ENTRY_POINTS[name][1]} <= labels
        assert {"n_groups = 0", "transient = T", "cols = 0", "n_out = 0", "Gram 129, null workspace"} <= labels
        text = " | ".join(r["error"] for r in rows)
        assert "null pointer" in text and "invalid sizes" in text
        if "solve_batch" not in name and "solve_ridge_batch" not in name:       # Cholesky and leave-one-out
            assert {r["rc"] for r in rows} == {-1, -2}
            assert "workspace holds" in text and "aligned" in text
    assert all(r["rc"] in (-1, -2) and r["error"].startswith(r["fn"] + ": ") for r in ROWS)


@pytest.mark.parametrize("i", range(len(ROWS)), ids=[f"{r['fn'][4:]}-{r['case']}".replace(" ", "_") for r in ROWS])
def test_refused_call_answers_as_recorded(lib, i):
    r = ROWS[i]
    rc, text = rec.answer(lib, r["fn"], r["args"])
    assert (rc, text.encode()) == (r["rc"], r["error"].encode()), f"differs from commit {DOC['commit']}"
