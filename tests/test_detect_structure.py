"""(no GPU) What the speed of the fixed-shape detector tail (detect_count_fixed_kernel in esn_detect.hip) rests on, read
off the gfx950 assembly of both instances (float64 and float32 Y), compiled with the product flags the way
tools/detect_isa.py does:

  * no scratch: the rows and tx words of the next frame are held in registers;
  * no v_mul_hi_u32 (an integer division by a run-time value) and no s_barrier inside the frame loop;
  * at most 716 vector instructions per frame (the static count of the frame loop over the frames it takes per trip;
    one wave executes it).  The budget: the kernel must read 1.573 GB per bench launch (Y 153 600 x 128 x 8 x 8 B,
    tx_bits 153 600 x 128 x 16 B), 0.262 ms at 6.0 TB/s; at the 4.08 cycles per vector instruction the generic kernel
    was measured at and 1.9 to 2.1 GHz on 1024 SIMDs, vector issue stays below that time with at most about 125 M
    vector instructions per launch; the design budget is 110 M, which is 716 per frame (the generic kernel: 1 856);
  * VGPRs and LDS allow three waves per SIMD (twelve one-wave workgroups per CU), the occupancy the instance is
    designed for: at most 168 VGPRs, and 12 x LDS bytes within the 160 KiB of a CU.

Skipped where hipcc is absent."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("detect_isa", os.path.join(ROOT, "tools", "detect_isa.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
VALU_PER_FRAME_BUDGET = 716
WAVES_PER_SIMD = 3
INSTANCES = [False, True]


@pytest.fixture(scope="module")
def instances(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("detect_isa") / "esn_detect.s")
    isa.compile_asm(out)
    with open(out) as f:
        return isa.functions(f.read().splitlines())


def test_both_instances_are_there(instances):
    assert sorted(instances) == sorted(isa.instance_name(io32) for io32 in INSTANCES)


@pytest.mark.parametrize("io32", INSTANCES, ids=("f64", "f32"))
def test_no_scratch_and_designed_occupancy(instances, io32):
    _, meta = instances[isa.instance_name(io32)]
    print(io32, meta)
    assert meta["private_segment_fixed_size"] == 0
    assert meta["vgpr_spill_count"] == 0
    assert meta["vgpr_count"] <= 512 // WAVES_PER_SIMD // 8 * 8                 # 168: three waves per SIMD
    assert 4 * WAVES_PER_SIMD * meta["group_segment_fixed_size"] <= 160 * 1024  # one-wave workgroups


@pytest.mark.parametrize("io32", INSTANCES, ids=("f64", "f32"))
def test_frame_loop_within_the_instruction_budget(instances, io32):
    body, _ = instances[isa.instance_name(io32)]
    st = isa.loop_stats(body, io32)
    print(io32, st)
    assert st["v_mul_hi_u32"] == 0
    assert st["s_barrier"] == 0
    assert st["valu_per_frame"] <= VALU_PER_FRAME_BUDGET
    assert st["valu_f64"] / st["frames_per_trip"] >= 280       # the loop found is the frame loop: 28 butterflies x 10 per lane
