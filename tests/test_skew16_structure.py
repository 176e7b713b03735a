"""(no GPU) What surrounds the recurrence slots of the 16x16x32 skewed predict kernel (esn_recur_skew16_impl.h), read
off the gfx950 assembly of all twelve instances, compiled with the product flags the way tools/skew16_isa.py does:

  * no s_cbranch_execnz between the first and the last s_barrier of either step loop: that branch is the latch of a
    readfirstlane loop around a buffer operation whose descriptor the compiler keeps in VGPRs (set B's four input
    LDS-DMA launches had one each) or of a per-lane branch (the tensor noise had 128);
  * at most one loop with a ds_write_b16 in front of the step loops (the inputs of step 0): the state image is zeroed
    and filled in 16-byte stores;
  * spilled VGPRs not above those of the kernel before the prologue was rewritten, per instance (the lower block of
    profiles/r07_skew16_isa.txt), and no scratch instruction inside a GEMM trip loop (there was none).

Skipped where hipcc is absent."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("skew16_isa", os.path.join(ROOT, "tools", "skew16_isa.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# (precision, noise mode, float32 I/O) -> spilled VGPRs / scratch instructions inside the trip loops of the parent
PARENT = {
    ("9TraitsF16", 0, 1): (8, 0), ("9TraitsF16", 1, 1): (2, 0), ("9TraitsF16", 2, 1): (4, 0),
    ("9TraitsF16", 0, 0): (8, 0), ("9TraitsF16", 1, 0): (2, 0), ("9TraitsF16", 2, 0): (4, 0),
    ("10TraitsBF16", 0, 1): (0, 0), ("10TraitsBF16", 1, 1): (13, 0), ("10TraitsBF16", 2, 1): (7, 0),
    ("10TraitsBF16", 0, 0): (0, 0), ("10TraitsBF16", 1, 0): (2, 0), ("10TraitsBF16", 2, 0): (6, 0),
}


def _name(key):
    tr, noise, io32 = key
    return f"_ZN3esn19recur_skew16_kernelINS_{tr}ELi{noise}ELb{io32}EEEvNS_11RecurParamsE"


@pytest.fixture(scope="module")
def instances(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("skew16_isa") / "esn_recur_skew16.s")
    isa.compile_asm(out)
    with open(out) as f:
        return isa.functions(f.read().splitlines())


def test_all_twelve_instances_are_there(instances):
    assert sorted(instances) == sorted(_name(k) for k in PARENT)


@pytest.mark.parametrize("key", sorted(PARENT), ids=lambda k: f"{k[0][-4:].lstrip('s')}-noise{k[1]}-io32_{k[2]}")
def test_structure_around_the_slots(instances, key):
    body, meta = instances[_name(key)]
    st = isa.structure(body, meta)
    print(key, st)
    spilled, trip_scratch = PARENT[key]
    assert st["step_loops"] == 2                                   # one body per wave set
    assert st["execnz_in_steps"] == 0
    assert st["b16_loops_before"] <= 1
    assert st["spilled_vgprs"] <= spilled
    assert st["trip_scratch"] <= trip_scratch
