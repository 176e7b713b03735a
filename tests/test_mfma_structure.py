"""(no GPU) Every instance of the MFMA recurrence kernel (esn::recur_mfma_kernel), read off the gfx950 assembly of
esn_recur_mfma_{f32,f16,bf16}.hip compiled with the product flags the way tools/mfma_isa.py does, against the table
that tool recorded from the commit named in tests/golden/mfma_parent_regs.json:

  * the set of mangled instance names is the recorded one (the kernel keeps its name and its template parameter list:
    bench.py's kernel label, tools/pmc_common.py and the kernel-stats files under profiles/ go by them);
  * per instance, spilled VGPRs, spilled SGPRs and private-segment bytes are not above the recorded ones;
  * no s_swappc: every lambda of the schedules is inlined (an outlined one sends the accumulators through scratch).

VGPR counts are printed, not asserted (occupancy is set by __launch_bounds__ and the LDS image here).
Skipped where hipcc is absent."""
import importlib.util
import json
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("mfma_isa", os.path.join(ROOT, "tools", "mfma_isa.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
with open(isa.GOLDEN) as _f:
    DOC = json.load(_f)
PARENT = {n: dict(zip(DOC["keys"], v)) for n, v in DOC["instances"].items()}


@pytest.fixture(scope="module")
def instances(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not found")
    return isa.table(isa.compile_asm(str(tmp_path_factory.mktemp("mfma_isa"))))


def test_instance_names_are_the_recorded_ones(instances):
    assert sorted(instances) == sorted(PARENT)


def test_no_instance_spills_more_or_calls(instances):
    worse = []
    for name in sorted(PARENT):
        now, was = instances[name], PARENT[name]
        print(isa.short(name), "VGPRs", now["vgpr_count"], "(recorded", was["vgpr_count"], ")")
        for k in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            if now[k] > was[k]:
                worse.append((isa.short(name), k, now[k], was[k]))
        if now["swappc"] != 0:
            worse.append((isa.short(name), "swappc", now["swappc"], 0))
    assert not worse, worse
