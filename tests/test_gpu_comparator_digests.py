"""The Adam-trained comparator banks and the four comparator point functions give, bit for bit, what the commit named in
tests/golden/comparator_digests.json gave (tools/record_comparator_digests.py recorded it there and says at which shapes):
every trained array and the loss of FnnBank, CnnBank and LstmBank (the LSTM at both of its kernel instances), a ragged
prediction from them (the FNN's also at "f16"), and the errors and bits of elm_point, fnn_point, cnn_point and lstm_point
over chunks with a remainder, with shared and with per-block initial sets.  The banks share one base and the points one
helper; neither may move a bit."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_comparator_digests",
                                               os.path.join(ROOT, "tools", "record_comparator_digests.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(rec.GOLDEN) as _f:
    DOC = json.load(_f)


def test_the_golden_file_is_the_one_the_tool_writes():
    assert DOC["seed"] == rec.SEED and len(DOC["commit"]) >= 7
    assert sorted(DOC["banks"]) == sorted(rec.BANKS) and sorted(DOC["points"]) == sorted(rec.POINTS)
    for name, row in rec.BANKS.items():
        assert sorted(DOC["banks"][name]) == sorted(list(row[3]) + ["loss"] + ["predict_" + p for p in row[4]])
    for name in rec.POINTS:
        assert len(DOC["points"][name]) == 4
    digests = [d for part in ("banks", "points") for v in DOC[part].values() for d in v.values()]
    assert all(len(d) == 64 for d in digests)


@pytest.mark.parametrize("name", list(rec.BANKS))
def test_bank_trains_and_predicts_the_recorded_bytes(name):
    got = rec.bank_digests(name)
    assert got == DOC["banks"][name], f"differs from commit {DOC['commit']}"


@pytest.mark.parametrize("name", list(rec.POINTS))
def test_point_counts_the_recorded_bytes(name):
    got = rec.point_digests(name)
    assert got == DOC["points"][name], f"differs from commit {DOC['commit']}"
