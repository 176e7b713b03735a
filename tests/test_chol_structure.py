"""(no GPU) What the residency and the diagonal-block factorisation of the LDS Cholesky read-out kernel
(readout_chol_kernel in esn_solve_chol.hip) rest on, read off the gfx950 assembly of all eight instances, compiled with the
product flags the way tools/chol_isa.py does:

  * no scratch and at most 128 VGPRs in any instance: two workgroups of 512 threads per CU (four waves per SIMD);
  * readout_chol_big_kernel uses no more scratch than it did (none);
  * in the headline instance (float32 E, wide, no ridge) the stretch between the two barriers that bracket the
    diagonal-block factorisation holds fewer v_readlane_b32 + v_writelane_b32 than it did when every L[k][j] travelled
    lane -> SGPR pair -> operand and the broadcasts were spilled for the inversion (PARENT_LANE_TRAFFIC, counted with
    the same tool on the commit before the DPP form); the pivot is a DPP row broadcast too, so there is none now.

Skipped where hipcc is absent."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("chol_isa", os.path.join(ROOT, "tools", "chol_isa.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INSTANCES = [(te, wide, rg) for te in "fd" for wide in (1, 0) for rg in (1, 0)]
PARENT_LANE_TRAFFIC = 1010           # 711 v_readlane_b32 + 299 v_writelane_b32 of 2804 instructions
PARENT_BIG_SCRATCH = 0


def _name(key):
    te, wide, rg = key
    return f"_ZN3esn19readout_chol_kernelI{te}Lb{wide}ELb{rg}EEEvNS_11SolveParamsE"


@pytest.fixture(scope="module")
def instances(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("chol_isa") / "esn_solve_chol.s")
    isa.compile_asm(out)
    with open(out) as f:
        return isa.functions(f.read().splitlines())


def test_all_instances_are_there(instances):
    small = sorted(n for n in instances if "big" not in n)
    assert small == sorted(_name(k) for k in INSTANCES)
    assert len([n for n in instances if "big" in n]) == 2


@pytest.mark.parametrize("key", INSTANCES, ids=lambda k: f"{'f32' if k[0] == 'f' else 'f64'}-{'wide' if k[1] else 'tall'}-ridge{k[2]}")
def test_no_scratch_and_128_vgprs(instances, key):
    _, meta = instances[_name(key)]
    print(key, meta)
    assert meta["private_segment_fixed_size"] == 0
    assert meta["vgpr_spill_count"] == 0
    assert meta["vgpr_count"] <= 128


def test_big_kernel_scratch_not_above_parent(instances):
    for name, (_, meta) in instances.items():
        if "big" in name:
            assert meta["private_segment_fixed_size"] <= PARENT_BIG_SCRATCH, name


def test_diagonal_block_lane_traffic_below_parent(instances):
    body, _ = instances[isa.HEADLINE]
    mix = isa.diag_stretch(body)
    n = isa.lane_traffic(mix)
    print(sum(mix.values()), "instructions,", n, "v_readlane + v_writelane;", mix.most_common(8))
    assert mix["v_rsq_f64_e32"] == 16                      # the stretch is the factorisation of one tile
    assert n < PARENT_LANE_TRAFFIC
