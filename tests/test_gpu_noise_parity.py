"""State noise of every recurrence kernel against the host model of the stream (tests/noise_ref.py) and the float64
oracle run with the same draws.  Cases, tolerances and amplitudes are the shared table of noise_ref.py;
tests/test_noise_reference_cpu.py proves on the CPU that at those a kernel with a wrong step, frame or row, or with no
noise at all, cannot pass.  Every launch asserts its dispatch path.

  (a) read-back: zero weights, noise 1, counter mode, harvest: E[g, s + 1, r] + 0.5 IS the model's uniform, exactly.
      float64 paths: tanh(0) + 1.0 (u - 0.5) in double.  float32 matrix-pipe harvest: fmaf(byte, 1/256, 0 + (0.5/256
      - 0.5)) -- every operand and the result are multiples of 2^-9 below 1: exact.  Not run for fp16 / bf16: their
      packed-half tail rounds tanh - c1 to the noise grid itself, an exact tie at zero pre-activation.
  (b) tensor mode (RandomState uniforms) against the oracle replaying the same rows: outputs of the first, last-of-
      group, first-of-next-group and last (ragged) frame; states of the first, middle and last pilot.
  (c) counter mode equals tensor mode fed counter_uniforms(...), same kernel, weights and launch.  float64 paths:
      bitwise (both modes evaluate p.noise * (u - 0.5) on the same double u).  Other precisions differ in how the
      addition rounds (counter: one fma of the byte, in packed half on the fp16 kernels; tensor: float u - 0.5, a
      multiply and an add).  Largest relative difference, max |a - b| / max |b|, measured on the MI355X:

          case                      noise   difference
          p-f32-48                  0.1     5.844e-08
          h-f32-48                  0.1     1.996e-07
          p-f32-300                 0.1     1.403e-07
          h-f32-300                 0.1     3.412e-07
          p-f32-600                 0.1     1.604e-07
          h-f32-600                 0.1     4.411e-07
          p-f16-100                 0.5     0
          h-f16-100                 0.1     4.655e-04
          p-f16-1024-skew           0.5     8.761e-04
          p-f16-1024-instep         0.5     0
          h-f16-1024                0.1     9.320e-04
          p-f16-1100-persistent     0.5     0
          h-f16-1100-persistent     0.1     9.337e-04
          p-bf16-100                0.5     0
          h-bf16-100                0.1     0
          p-f16-300-skew16          0.5     5.641e-04
          p-f16-512-skew16          0.5     9.515e-04
          p-f16-512-skew32          0.5     6.509e-04
          p-f16-1100-big            0.5     0
          h-f16-1100-big            0.1     9.320e-04
          h-f16-512-hcluster17      0.1     9.320e-04
          h-f16-300-hcluster17      0.1     4.664e-04
          h-f16-512-hcluster1       0.1     2.940e-05
          h-f16-300-persistent      0.1     9.328e-04
          (the eight float64 cases: 0, asserted bitwise)

      The bounds (noise_ref.COUNTER_VS_TENSOR) are twice the largest of a precision: f32 8.9e-7, f16 1.91e-3 (the
      differences are single fp16 ulps of states above 1), bf16 0, i.e. bitwise at these shapes.  The difference is
      deterministic, the margin is for other shapes.  (Zeros at noise 0.5 outside the packed-half tail: noise / 256
      is then a power of two, so both forms add an exact term; bf16 keeps 8 bits, which a float32 rounding difference
      rarely crosses.)  With (b) this ties counter mode to the oracle on every kernel.
  (d) frame identity: a predict of B frames at group_offset k equals, bitwise, the same frames launched as the first 2 F
      at k and the rest at k + 2 (float64; fp16 on the 32x32x16 skewed kernel); a float64 predict and harvest whose
      frame index crosses 2^32 draw the model's mod-2^32 frames.  The 16x16x32 kernel sums its read-out in an order that
      depends on the column tile a group lands in inside the 128-slot workgroup tile -- moving a group to another
      column tile changes its outputs by one float32 ulp (6e-8 at |y| up to 0.4) with the noise on or off -- so its batch is
      cut at the tile boundary (8 groups at k, the ninth at k + 8), which keeps every group's column tile.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_ref as nr  # noqa: E402

pytestmark = pytest.mark.gpu

ids = lambda c: c.id  # noqa: E731


class Knobs:
    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        from esn_ofdm_mimo_amd import _lib
        for k, v in self.kv.items():
            _lib.debug_set(k, v)

    def __exit__(self, *exc):
        from esn_ofdm_mimo_amd import _lib
        for k in self.kv:
            _lib.debug_set(k, None)


_banks = {}


def bank_for(c, zero=False):
    """One bank per (precision-independent) weight shape; the scalings / read-outs of the case are set per launch."""
    from esn_ofdm_mimo_amd import batched
    key = (c.n_res, c.n_in, c.n_out, zero)
    if key not in _banks:
        w, w_in, w_fb = nr.weights(c.n_res, c.n_in, c.n_out)
        if zero:
            w, w_in, w_fb = np.zeros_like(w), np.zeros_like(w_in), np.zeros_like(w_fb)
        _banks[key] = batched.ReservoirBank(c.n_in, c.n_out, c.n_res, w, w_in, w_fb)
    return _banks[key]


def launch(c, noise_mode, noise_u=None, group_offset=nr.GROUP_OFFSET, groups=None, noise=None, zero=False, seed=nr.SEED):
    """The case's launch (or its groups [lo, hi)) -> numpy: outputs [B, T - transient, n_out] / states [G, T, n_res]."""
    from esn_ofdm_mimo_amd import _lib
    d = nr.case_data(c.id)
    lo, hi = groups or (0, c.groups)
    f0, f1 = lo * c.F, min(hi * c.F, nr.n_seq(c))
    bank = bank_for(c, zero)
    bank.noise = c.noise if noise is None else noise
    bank.set_scaling(d["in_scale"][lo:hi], d["in_shift"][lo:hi], d["t_scale"][lo:hi], d["t_shift"][lo:hi])
    with Knobs(c.knobs):
        assert _lib.recur_path(c.kind == "harvest", c.precision, bank.shape, f1 - f0, c.F) == c.path, c.id
        if c.kind == "predict":
            bank.set_readout(d["W_out"][lo:hi])
            out = bank.predict(d["u"][f0:f1], c.F, transient=nr.TRANSIENT, precision=c.precision, x0=d["x0"][lo:hi],
                               y0=d["y0"][lo:hi], noise_mode=noise_mode, noise_u=noise_u, seed=seed,
                               group_offset=group_offset)
        else:
            out = bank.harvest(d["u"][f0:f1], d["d"][f0:f1], precision=c.precision, noise_mode=noise_mode,
                               noise_u=noise_u, seed=seed, group_offset=group_offset)[..., :c.n_res]
        out = out.cpu().numpy()
    bank.raise_if_cluster_timed_out()
    bank.raise_if_harvest_timed_out()
    return out


def model_uniforms(c, group_offset=nr.GROUP_OFFSET, seed=nr.SEED):
    return nr.counter_uniforms(seed, group_offset * c.F, nr.n_seq(c), nr.n_steps(c), c.n_res)


# ---- (a) ---------------------------------------------------------------------------------------------------------
def check_read_back(case, group_offset):
    assert case.kind == "harvest" and case.precision in ("f64", "f32")
    E = launch(case, "counter", group_offset=group_offset, noise=1.0, zero=True)
    want = model_uniforms(case, group_offset)
    assert not E[:, 0].any()                                   # row 0 is never fed
    got = E[:, 1:] + 0.5
    bad = np.argwhere(got != want)
    assert bad.size == 0, (case.id, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("case", [c for c in nr.CASES if c.readback], ids=ids)
def test_states_read_back_the_stream(case):
    check_read_back(case, nr.GROUP_OFFSET)


def test_harvest_frame_index_wraps_at_2_to_32():
    check_read_back(nr.BY_ID["h-f64-valu-71"], 2 ** 32 - 2)       # pilots 2^32 - 2, 2^32 - 1, 0, 1, 2


# ---- (b) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in nr.CASES if c.tol is not None], ids=ids)
def test_tensor_mode_matches_the_oracle_with_the_same_draws(case):
    d = nr.case_data(case.id)
    nz = d["nz"][:nr.n_seq(case)]
    got = launch(case, "tensor", noise_u=nz)
    worst = 0.0
    for i in nr.frames_compared(case):
        err = nr.rel_err(got[i], nr.oracle_run(case, d, i, nz[i]))
        print(f"NOISE_B {case.id} sequence {i}: {err:.3e} (tolerance {case.tol:g})")
        worst = max(worst, err)
    assert worst < case.tol, (case.id, worst)


# ---- (c) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", nr.CASES, ids=ids)
def test_counter_mode_equals_tensor_mode_fed_the_model(case):
    counter = launch(case, "counter")
    tensor = launch(case, "tensor", noise_u=model_uniforms(case))
    assert np.isfinite(counter).all() and np.abs(counter).max() > 0
    diff = nr.rel_err(counter, tensor)
    bound = nr.COUNTER_VS_TENSOR[case.precision]
    print(f"NOISE_C {case.id} {case.precision} noise {case.noise:g}: {diff:.3e} (bound {bound})")
    if case.precision == "f64":
        assert np.array_equal(counter, tensor), (case.id, diff)
    else:
        assert diff <= bound, (case.id, diff)
    # the stream enters at all: another seed gives other states
    assert not np.array_equal(counter, launch(case, "counter", seed=nr.SEED + (1 << 32)))


# ---- (d) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id,cut", [("p-f64-valu-71-tiles", 2), ("p-f16-512-skew32", 2), ("p-f16-512-skew16", 8)])
def test_a_frame_draws_the_same_noise_in_whichever_launch(case_id, cut):
    case, k = nr.BY_ID[case_id], nr.GROUP_OFFSET
    whole = launch(case, "counter", group_offset=k)
    head = launch(case, "counter", group_offset=k, groups=(0, cut))
    tail = launch(case, "counter", group_offset=k + cut, groups=(cut, case.groups))
    assert head.shape[0] == cut * case.F and head.shape[0] + tail.shape[0] == whole.shape[0]
    assert np.array_equal(np.concatenate([head, tail]), whole)
    # ... and a frame launched under another global index does not
    assert not np.array_equal(launch(case, "counter", group_offset=k + 1, groups=(0, cut)), head)


def test_predict_frame_index_wraps_at_2_to_32():
    case = nr.BY_ID["p-f64-valu-71"]                 # F = 3: group_offset F crosses 2^32 inside the batch
    k = (2 ** 32 + 2) // 3 - 1
    assert k * case.F < 2 ** 32 < k * case.F + nr.n_seq(case)
    counter = launch(case, "counter", group_offset=k)
    tensor = launch(case, "tensor", noise_u=model_uniforms(case, k))
    assert np.array_equal(counter, tensor)
