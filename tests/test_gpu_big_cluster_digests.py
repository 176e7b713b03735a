"""The launch-per-step GEMM kernels beyond 1024 units (esn_big_predict.hip, esn_big_harvest.hip) and the harvest cluster
kernel (esn_harvest_cluster.hip) write, at the shapes of tools/record_big_cluster_digests.py, exactly the bytes that the
commit named in tests/golden/big_cluster_parent_digests.json wrote: a clean-up of these kernels that is meant to keep the
results changes no output bit.  (tests/test_gpu_big.py and tests/test_gpu_harvest_cluster.py compare them with the
persistent kernels within rounding; this pins the bits.)"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_big_cluster_digests",
                                               os.path.join(ROOT, "tools", "record_big_cluster_digests.py"))
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


def test_every_case_reaches_its_kernel():
    """(no GPU) every case dispatches to the kernel it names, and the three kernels all occur"""
    for c in CASES:
        assert rec.path(c) == c["path"], c["id"]
    assert {c["path"] for c in CASES} == {"big_predict", "big_harvest", "harvest_cluster"}


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["id"] for c in CASES])
def test_output_bytes_match_recorded_digest(i):
    c = CASES[i]
    name, want = DOC["digests"][i]
    assert name == c["id"]
    assert rec.digest(i, c) == want, f"{c['id']}: output bytes differ from commit {DOC['commit']}"
