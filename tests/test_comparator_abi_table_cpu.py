"""The argument checks of the eight comparator entry points (esn_elm_features, esn_elm_predict and the train / predict
pairs of the FNN, the CNN and the LSTM) answer every refused call of tests/golden/comparator_abi_errors.json with the
return code and the esn_last_error() text, byte for byte, that the commit named there gave, and the three workspace
queries answer its grid of shapes with the same sizes: the trained entry points share their optimiser, workspace and
sequence-model checks, and each keeps its own answers and the order of its checks.  Every row is refused before any
launcher or device call (tools/record_comparator_abi_errors.py says which candidate rows were left out for that reason),
so no GPU is needed and none is touched."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_comparator_abi_errors",
                                               os.path.join(ROOT, "tools", "record_comparator_abi_errors.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(rec.GOLDEN) as _f:
    DOC = json.load(_f)
ROWS, SIZES = DOC["rows"], DOC["queries"]


@pytest.fixture(scope="module")
def lib():
    from esn_ofdm_mimo_amd import _lib
    return _lib.load()


def test_table_is_the_one_the_tool_builds(lib):
    """the recorded calls are today's sample (the workspace sizes in them are what today's queries say)"""
    assert DOC["abi"] == lib.esn_abi_version() == 10 and len(DOC["commit"]) >= 7
    assert [(r["fn"], r["case"], r["args"]) for r in ROWS] == [(n, c, a) for n, c, a in rec.cases(lib)]
    assert [(r["fn"], r["args"]) for r in SIZES] == rec.queries(lib)


def test_table_covers_every_entry_point_and_stage():
    by_fn = {}
    for r in ROWS:
        by_fn.setdefault(r["fn"], []).append(r)
    assert sorted(by_fn) == sorted(rec.ENTRY_POINTS)
    for name, rows in by_fn.items():
        params, mandatory, query = rec.ENTRY_POINTS[name]
        labels = {r["case"] for r in rows}
        assert {f"null {p}" for p in mandatory} <= labels
        assert {"n_in = 0", "T_in > T", "precision ESN_F32", "precision ESN_BF16", "precision 99"} <= labels
        assert {r["rc"] for r in rows} == {-1, -2}
        assert sum(r["case"] in dict(rec.PAIRS) for r in rows) >= (1 if name == "esn_elm_features" else 3)   # two faults
        if query:
            assert {"null workspace", "workspace one byte short", "workspace at 68"} <= labels
            assert sum(query in r["error"] for r in rows) >= 3
        if name.endswith("_train"):
            assert {"n_isets = 0", "epochs = 0", "lr = -1.0", "lr = nan", "beta1 = 1.0", "beta2 = -0.1",
                    "eps = 0.0"} <= labels
    assert sum(len({r["fn"] for r in ROWS if r["case"] == label}) > 0 for label, _ in rec.PAIRS) >= 6
    assert all(r["rc"] in (-1, -2) and r["error"].startswith(r["fn"] + ": ") for r in ROWS)
    for query in rec.QUERIES:
        sizes = [r["bytes"] for r in SIZES if r["fn"] == query]
        assert 0 in sizes and max(sizes) > 0


@pytest.mark.parametrize("i", range(len(ROWS)), ids=[f"{r['fn'][4:]}-{r['case']}".replace(" ", "_") for r in ROWS])
def test_refused_call_answers_as_recorded(lib, i):
    r = ROWS[i]
    rc, text = rec.answer(lib, r["fn"], r["args"])
    assert (rc, text.encode()) == (r["rc"], r["error"].encode()), f"differs from commit {DOC['commit']}"


def test_workspace_queries_answer_as_recorded(lib):
    got = [getattr(lib, r["fn"])(*r["args"]) for r in SIZES]
    assert got == [r["bytes"] for r in SIZES], f"differs from commit {DOC['commit']}"
