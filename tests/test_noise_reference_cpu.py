"""The numpy model of the counter state-noise stream (tests/noise_ref.py) against its source, and the conditions
under which tests/test_gpu_noise_parity.py may call a kernel's noise right.  No GPU.

  * model equals source: a host program compiled from csrc/esn_common.h itself prints noise_key / noise_uniform on a
    grid; the model must give every value exactly;
  * the model's stream is uniform, distinct per (frame, step) and uncorrelated between rows;
  * power: for every case of the shared table that is compared with the oracle, four wrong streams (step + 1,
    frame + 1, rows 0..31 exchanged with 32..63, no noise) each move the compared quantity by at least twice the
    tolerance of the comparison -- a kernel with one of those errors cannot pass;
  * the bound of "counter mode equals tensor mode fed the model's uniforms" is at most half of what exchanging ONE
    quad of rows (0..3 with 4..7) does;
  * every case names the kernel the dispatch picks, and the table covers every path but the experimental "rs".
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_ref as nr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEEDS = [0, 1, 0xDEADBEEF, (7 << 32) + 12345, 2 ** 64 - 1]
FRAMES = [0, 1, 2, 1000003, 2 ** 32 - 2, 2 ** 32 - 1]
STEPS = [0, 1, 11, 521]
ROWS = list(range(8)) + [255, 511, 2047]

PROBE_SRC = r'''
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#undef __device__
#define __device__ __attribute__((device)) __attribute__((host))
#if !defined(__HIP_DEVICE_COMPILE__)
static inline unsigned int __umul24(unsigned int a, unsigned int b) { return (a & 0xffffffu) * (b & 0xffffffu); }
#endif
#include "esn_common.h"
/* argv: n_seeds seeds.. n_frames frames.. n_steps steps.. n_rows rows..; one line per (seed, frame, step) */
int main(int argc, char** argv) {
    int a = 1;
    unsigned long long v[4][64];
    int n[4];
    for (int k = 0; k < 4; ++k) {
        n[k] = atoi(argv[a++]);
        for (int i = 0; i < n[k]; ++i) v[k][i] = strtoull(argv[a++], 0, 10);
    }
    for (int i = 0; i < n[0]; ++i)
        for (int j = 0; j < n[1]; ++j)
            for (int s = 0; s < n[2]; ++s) {
                const uint32_t key = esn::noise_key((uint64_t)v[0][i], (uint32_t)v[1][j], (uint32_t)v[2][s]);
                printf("%u", key);
                for (int r = 0; r < n[3]; ++r) printf(" %.17g", (double)esn::noise_uniform(key, (uint32_t)v[3][r]));
                printf("\n");
            }
    return 0;
}
'''


def test_model_equals_the_header(tmp_path):
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("hipcc not found: the header cannot be compiled for the host")
    src, exe = tmp_path / "noise_probe.hip", tmp_path / "noise_probe"
    src.write_text(PROBE_SRC)
    r = subprocess.run([hipcc, "--offload-host-only", "-O1", "-I", os.path.join(ROOT, "esn_ofdm_mimo_amd", "csrc"),
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    args = []
    for axis in (SEEDS, FRAMES, STEPS, ROWS):
        args += [str(len(axis))] + [str(x) for x in axis]
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(SEEDS) * len(FRAMES) * len(STEPS)
    it = iter(lines)
    checked = 0
    for seed in SEEDS:
        for frame in FRAMES:
            for step in STEPS:
                f = next(it).split()
                key = int(nr.noise_key(seed, frame, step))
                assert int(f[0]) == key, (seed, frame, step)
                got = np.array([float(x) for x in f[1:]])
                want = nr.noise_uniform(key, np.array(ROWS))
                assert np.array_equal(got, want), (seed, frame, step, got, want)
                checked += len(ROWS)
    assert checked == 5 * 6 * 4 * 11
    # the array form the GPU tests use is the same function (frames wrap mod 2^32)
    u = nr.counter_uniforms(SEEDS[3], 2 ** 32 - 2, 4, 12, 2048)
    for j, frame in enumerate([2 ** 32 - 2, 2 ** 32 - 1, 0, 1]):
        assert np.array_equal(u[j, 11, ROWS], nr.noise_uniform(nr.noise_key(SEEDS[3], frame, 11), np.array(ROWS)))
    assert np.array_equal(u, nr.counter_uniforms(SEEDS[3], 2 ** 33 - 2, 4, 12, 2048))


def test_model_statistics():
    """seed 5, 300 frames x 40 steps x 512 rows.  Measured: chi2/255 0.93, mean 0.5002, 12 000 distinct columns, largest
    |correlation| between two rows 0.060 (12 000 samples: sigma 0.009, expected maximum of 131 000 pairs ~0.045)."""
    b = nr.counter_bytes(5, 0, 300, 40, 512).reshape(12000, 512)
    hist = np.bincount(b.ravel(), minlength=256).astype(np.float64)
    expect = b.size / 256.0
    chi2 = float(np.sum((hist - expect) ** 2 / expect)) / 255.0
    mean = float(((b.astype(np.float64) + 0.5) / 256.0).mean())
    distinct = len({row.tobytes() for row in b})
    c = np.corrcoef(b.astype(np.float64).T)
    cmax = float(np.max(np.abs(c - np.eye(512))))
    print(f"chi2/255 {chi2:.3f}  mean {mean:.5f}  distinct columns {distinct}  max |corr| {cmax:.4f}")
    assert 0.7 <= chi2 <= 1.3
    assert abs(mean - 0.5) < 1e-3
    assert distinct == 12000
    assert cmax < 0.08


def test_replay_rng_feeds_the_oracle_row_by_row():
    c = nr.BY_ID["h-f64-valu-71"]
    d = nr.case_data(c.id)
    rng = nr.ReplayRng(d["nz"][0])
    assert np.array_equal(rng.rand(c.n_res), d["nz"][0][0]) and np.array_equal(rng.rand(c.n_res), d["nz"][0][1])
    # with zero weights and noise 1 the oracle's states ARE the draws (the read-back test of the GPU module)
    from oracle import esn_oracle as eo
    z = np.zeros
    o = eo.OracleESN(c.n_in, c.n_out, c.n_res, noise=1.0, weights=(z((c.n_res, c.n_res)), z((c.n_res, c.n_in)),
                                                                     z((c.n_res, c.n_out))))
    o.rng = nr.ReplayRng(d["nz"][0])
    o.fit(d["u"][0], d["d"][0], 0)
    assert np.array_equal(o._ext_states[1:, :c.n_res] + 0.5, d["nz"][0]) and not o._ext_states[0, :c.n_res].any()


ORACLE_CASES = [c for c in nr.CASES if c.tol is not None]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: c.id)
def test_wrong_streams_move_the_result_by_twice_the_tolerance(case):
    d = nr.case_data(case.id)
    for i in nr.frames_compared(case):
        right = nr.oracle_run(case, d, i, d["nz"][i])
        for name, draws in nr.wrong_streams(d["nz"], i).items():
            moved = nr.rel_err(nr.oracle_run(case, d, i, draws), right)
            print(f"{case.id} sequence {i} {name}: {moved:.3e} (tolerance {case.tol:g})")
            assert moved >= 2 * case.tol, (case.id, i, name, moved)


@pytest.mark.parametrize("case", [c for c in nr.CASES if c.precision != "f64"], ids=lambda c: c.id)
def test_counter_vs_tensor_bound_is_below_one_quad_exchange(case):
    bound = nr.COUNTER_VS_TENSOR[case.precision]
    d = nr.case_data(case.id)
    for i in nr.frames_compared(case):
        right = nr.oracle_run(case, d, i, d["nz"][i])
        moved = nr.rel_err(nr.oracle_run(case, d, i, nr.exchange_rows(d["nz"][i], 0, 4, 4)), right)
        print(f"{case.id} sequence {i} rows 0..3 <-> 4..7: {moved:.3e} (bound {bound:g})")
        assert bound <= 0.5 * moved, (case.id, i, moved)


def test_table_names_the_dispatched_kernel_and_covers_every_path():
    from esn_ofdm_mimo_amd import build, _lib
    build.build_library(verbose=False)
    for c in nr.CASES:
        shape = _lib.Shape(c.n_res, c.n_in, c.n_out, 1, 1, 1.0)
        try:
            for k, v in c.knobs.items():
                _lib.debug_set(k, v)
            got = _lib.recur_path(c.kind == "harvest", c.precision, shape, nr.n_seq(c), c.F)
        finally:
            for k in c.knobs:
                _lib.debug_set(k, None)
        assert got == c.path, (c.id, got)
    assert {c.path for c in nr.CASES} == set(_lib.PATHS)
    for path in _lib.PATHS:
        kinds = {c.kind for c in nr.CASES if c.path == path}
        assert kinds, path
    # the ragged last group and the seed's high half are what the table promises
    assert all(c.last < c.F for c in nr.CASES if c.kind == "predict" and c.path != "cluster_f64")
    assert nr.SEED >> 32 and nr.GROUP_OFFSET
