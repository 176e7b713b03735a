"""The seven *_point functions and the constructor of DetectorSweep answer every refused call of
tests/golden/point_refusals.json with the exception class and the message, byte for byte, that the commit named there
gave: the points share their block-range, read-out and chunk helpers and the constructor checks its options in one
function, and each keeps its own answers and the order of its checks (cases and recorder:
tools/record_point_refusals.py).  Every row is refused from the arguments alone, so no GPU is needed and none is
touched -- nor for the three options the constructor used to check only after it had opened the device.  And the one QR
retry of the points (points._retry_with_qr) on stub bodies."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_point_refusals",
                                               os.path.join(ROOT, "tools", "record_point_refusals.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(rec.GOLDEN) as _f:
    DOC = json.load(_f)
ROWS = DOC["rows"]


def test_table_is_the_one_the_tool_builds():
    assert len(DOC["commit"]) >= 7
    assert [[r["fn"], r["link"], r["kw"]] for r in ROWS] == rec.cases()


def test_table_covers_every_function_and_the_order_of_its_checks():
    by_fn = {}
    for r in ROWS:
        by_fn.setdefault(r["fn"], []).append(r)
    assert sorted(by_fn) == sorted(rec.POINTS + (rec.SWEEP,))
    for fn, rows in by_fn.items():
        assert {r["class"] for r in rows} == {"ValueError"}
        assert sum(len(r["kw"]) + len(r["link"] or {}) >= 2 for r in rows) >= 3, fn       # two faults at once
        if fn != rec.SWEEP:
            texts = " ".join(r["error"] for r in rows)
            assert all(word in texts for word in ("n_blocks = 0", "first_block = -1", "chunk_blocks", "frames_per_block"))
    assert len({r["error"] for r in by_fn[rec.SWEEP]}) >= 20


@pytest.mark.parametrize("i", range(len(ROWS)), ids=[f"{i}-{r['fn']}" for i, r in enumerate(ROWS)])
def test_refused_call_answers_as_recorded(i):
    r = ROWS[i]
    cls, text = rec.answer(r["fn"], r["link"], r["kw"])
    assert (cls, (text or "").encode()) == (r["class"], r["error"].encode()), f"differs from commit {DOC['commit']}"


@pytest.mark.parametrize("kw, word", [(dict(ridge=1.0, ridge_grid=[1.0]), "give ridge or ridge_grid, not both"),
                                      (dict(radius="x"), "radius must be 'host' or 'device'"),
                                      (dict(radius_precision="x"), "radius_precision must be one of")])
def test_constructor_refuses_these_without_a_device(kw, word):
    from esn_ofdm_mimo_amd.link import LinkParams
    from esn_ofdm_mimo_amd.sweep import DetectorSweep
    with pytest.raises(ValueError, match=word):
        DetectorSweep(LinkParams(**rec.SMALL), **kw)


def _body(flags, calls):
    def body(method):
        calls.append(method)
        return "result of " + method, flags[method]
    return body


def test_a_flagged_point_is_redone_once_with_qr():
    from esn_ofdm_mimo_amd.points import _retry_with_qr
    calls = []
    assert _retry_with_qr(_body({"auto": np.array(1), "qr": np.array(0)}, calls), "auto") == "result of qr"
    assert calls == ["auto", "qr"]
    calls = []
    assert _retry_with_qr(_body({"chol": 3, "qr": 1}, calls), "chol") == "result of qr"       # (no third pass)
    assert calls == ["chol", "qr"]


def test_an_unflagged_point_and_a_qr_point_run_once():
    from esn_ofdm_mimo_amd.points import _retry_with_qr
    calls = []
    assert _retry_with_qr(_body({"auto": np.array(0)}, calls), "auto") == "result of auto"
    assert calls == ["auto"]
    calls = []
    assert _retry_with_qr(_body({"qr": 1}, calls), "qr") == "result of qr"
    assert calls == ["qr"]
