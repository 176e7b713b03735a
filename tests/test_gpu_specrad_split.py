"""The split-operand spectral radius on the device (csrc/esn_specrad_split.hip): against the float64
restatement (tests/specrad_ref.py) at the same K and against np.linalg.eigvals, its padding, batch invariance and
flagging, and the plumbing through reservoirs.generate and DetectorSweep (radius_precision, the radius cache).

Bounds: kernel vs restatement at the same K 1e-6 relative -- 5 x the 2.0e-7 the NumPy emulation of the method measured
(2.1e-7 in tests/specrad_split_ref.py's variant; the two fp16 pieces carry 22 bits), the margin for the matrix pipe's
own summation order;
kernel vs eigvals at K = 24 1e-6 relative, the bound the float64 kernel is held to.  The matrices are not symmetric:
a swapped operand (A A^T) or a missing cross term fails the first test."""
import numpy as np
import pytest

import specrad_ref as sr

pytestmark = pytest.mark.gpu

CASES = sr.cases()
SPLIT = "f16x2"


@pytest.fixture(scope="module")
def res():
    from esn_ofdm_mimo_amd import reservoirs
    return reservoirs


@pytest.fixture(scope="module")
def mats():
    """The CPU test's matrices with their eigvals radius and their restated radius at K = 24 and 16, computed once."""
    out = {}
    for c in CASES:
        w = sr.reference_matrix(*c)
        w.setflags(write=False)
        out[c] = (w, float(np.max(np.abs(np.linalg.eigvals(w)))), sr.specrad(w, 24)[0], sr.specrad(w, 16)[0])
    return out


def _groups():
    keys = {}
    for c in CASES:
        keys.setdefault(c[:2], []).append(c)
    return keys


def _split(res, w, k=24):
    r, s = res.spectral_radius(w, n_squarings=k, return_status=True, precision=SPLIT)
    return r.cpu().numpy(), s.cpu().numpy()


# ---- 1. accuracy ---------------------------------------------------------------------------------------------------
def test_split_radius_matches_restatement_and_eigvals(res, mats):
    worst = {24: 0.0, 16: 0.0, "eig": 0.0}
    for (n, sp), cs in _groups().items():
        stack = np.stack([mats[c][0] for c in cs])
        for k, col in ((24, 2), (16, 3)):
            got5, st5 = _split(res, stack, k)               # S = 5 (1 at n = 512)
            assert not st5.any(), (n, sp, k)
            for i in range(len(cs)):                        # S = 1: every matrix alone, the same bits and status 0
                got1, st1 = _split(res, stack[i], k)
                assert int(st1) == 0 and float(got1) == got5[i], (n, sp, k, i)
            for c, g in zip(cs, got5):
                rel = abs(g - mats[c][col]) / mats[c][col]
                worst[k] = max(worst[k], rel)
                if k == 24:
                    worst["eig"] = max(worst["eig"], abs(g - mats[c][1]) / mats[c][1])
    print(f"split kernel vs restatement: worst relative {worst[24]:.2e} (K = 24), {worst[16]:.2e} (K = 16); "
          f"split kernel vs eigvals (K = 24): {worst['eig']:.2e}; {len(CASES)} matrices")
    assert worst[24] <= 1e-6 and worst[16] <= 1e-6
    assert worst["eig"] <= 1e-6


# ---- 2. ragged padding ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, k", [(5, 24), (33, 24), (65, 24), (130, 24), (577, 16)])
def test_split_radius_with_a_ragged_edge(res, n, k):
    w = sr.reference_matrix(n, 0.1, 7000 + n)
    assert sr.has_cycle(w)
    want = sr.specrad(w, k)[0]
    got, st = _split(res, w, k)
    rel = abs(float(got) - want) / want
    print(f"n = {n}, K = {k}: relative {rel:.2e}")
    assert int(st) == 0 and rel <= 1e-6, (n, k, rel)


# ---- 3. batch invariance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 130, 300])
def test_split_radius_is_bitwise_the_same_alone_and_in_a_batch(res, mats, n):
    cs = _groups()[(n, 0.1)]
    stack = np.stack([mats[c][0] for c in cs])
    batch, _ = _split(res, stack)
    assert batch.shape == (5,) and len(set(batch.tolist())) == 5
    for i in (0, 3):
        assert float(_split(res, stack[i])[0]) == batch[i], (n, i)


def test_split_radius_at_512_is_bitwise_the_same_alone_and_in_a_batch_of_two(res):
    stack = np.stack([sr.reference_matrix(512, 0.1, 9100 + i) for i in range(2)])
    batch, st = _split(res, stack, 16)
    assert not st.any() and batch[0] != batch[1]
    assert float(_split(res, stack[1], 16)[0]) == batch[1]
    assert float(_split(res, stack[0], 16)[0]) == batch[0]


# ---- 4. flagging ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 130])
def test_zero_and_nilpotent_matrices_are_flagged_and_leave_their_neighbours_alone(res, mats, n):
    cs = _groups()[(n, 0.1)]
    a, b = mats[cs[0]][0], mats[cs[1]][0]
    tri = np.triu(np.ones((n, n)), 1)
    r4, s4 = _split(res, np.stack([a, np.zeros_like(a), b, tri]))
    r2, s2 = _split(res, np.stack([a, b]))
    assert s4.tolist() == [0, 1, 0, 1] and s2.tolist() == [0, 0]
    assert r4[1] == 0.0 and r4[3] == 0.0 and r4[0] == r2[0] and r4[2] == r2[1]


# ---- 5. generate ---------------------------------------------------------------------------------------------------
def test_generate_with_the_split_radius_and_with_a_known_radius(res):
    args = (4, 2, 130, 0.9, 0.1, 77)
    W, W_in, W_fb, radius, status = res.generate(*args, first_set=3, n_sets=5)
    Ws, Ws_in, Ws_fb, rs, ss = res.generate(*args, first_set=3, n_sets=5, radius_precision=SPLIT)
    w, ws = W.cpu().numpy(), Ws.cpu().numpy()
    assert not status.cpu().numpy().any() and not ss.cpu().numpy().any()
    assert np.abs(ws - w).max() <= 2e-6 * np.abs(w).max()
    assert not np.array_equal(rs.cpu().numpy(), radius.cpu().numpy())        # (it was measured on the other pipe)
    assert np.array_equal(Ws_in.cpu().numpy(), W_in.cpu().numpy()) and np.array_equal(Ws_fb.cpu().numpy(), W_fb.cpu().numpy())
    Wk, Wk_in, Wk_fb, rk, sk = res.generate(*args, first_set=3, n_sets=5, radius=radius)
    assert np.array_equal(Wk.cpu().numpy(), w) and np.array_equal(rk.cpu().numpy(), radius.cpu().numpy())
    assert not sk.cpu().numpy().any()
    assert np.array_equal(Wk_in.cpu().numpy(), W_in.cpu().numpy()) and np.array_equal(Wk_fb.cpu().numpy(), W_fb.cpu().numpy())
    with pytest.raises(ValueError):
        res.generate(*args, first_set=3, n_sets=5, radius=radius[:4])
    # a flagged radius handed back (0, status 1) leaves its set unscaled, as the measuring path does
    import torch
    r0 = radius.clone()
    r0[2] = 0.0
    for st in (None, torch.tensor([0, 0, 1, 0, 0], dtype=torch.int32, device=radius.device)):
        Wf, _, _, _, sf = res.generate(*args, first_set=3, n_sets=5, radius=r0, radius_status=st, check_status=False)
        assert sf.cpu().tolist() == [0, 0, 1, 0, 0]
        wf = Wf.cpu().numpy()
        assert np.array_equal(wf[[0, 1, 3, 4]], w[[0, 1, 3, 4]]) and np.isfinite(wf[2]).all()


def test_bank_generate_passes_the_radius_precision_on(res):
    from esn_ofdm_mimo_amd.batched import ReservoirBank
    bank = ReservoirBank.generate(4, 2, 100, 0.9, 0.1, seed=21, first_set=0, n_sets=3, radius_precision=SPLIT,
                                  n_squarings=16)
    want = res.generate(4, 2, 100, 0.9, 0.1, 21, first_set=0, n_sets=3, radius_precision=SPLIT, n_squarings=16)
    assert np.array_equal(bank.weights[0].cpu().numpy(), want[0].cpu().numpy())
    assert np.array_equal(bank.generated_radius.cpu().numpy(), want[3].cpu().numpy())


# ---- 6. sweep ------------------------------------------------------------------------------------------------------
def test_split_fresh_sweep_chunking_and_the_radius_cache(res):
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    kw = dict(n_reservoir=100, reservoirs="fresh", radius_precision=SPLIT, radius_squarings=16)
    sw = DetectorSweep(LinkParams(), **kw)
    ber_c, cnt_c = sw.run([6, 21], 7, frames_per_block=2, chunk_blocks=3)
    assert sw.fresh_radius_hits == 7
    ber_u, cnt_u = sw.run([6, 21], 7, frames_per_block=2, chunk_blocks=7)
    assert sw.fresh_radius_hits == 7
    assert np.array_equal(cnt_c, cnt_u)
    assert cnt_u[:, 1].min() > 0 and ber_u[1] < ber_u[0]
    plain = DetectorSweep(LinkParams(), fresh_radius_cache=False, **kw)
    _, cnt_p = plain.run([6, 21], 7, frames_per_block=2, chunk_blocks=3)
    assert plain.fresh_radius_hits == 0
    assert np.array_equal(cnt_p, cnt_c)
    # the bank holds the split path's weights, block b in slot b
    want = res.generate(sw.n_in, sw.n_out, 100, 0.9, 0.1, sw.reservoir_seed, first_set=5, n_sets=1,
                        radius_precision=SPLIT, n_squarings=16)
    assert np.array_equal(sw.bank.weights[0][5].cpu().numpy(), want[0][0].cpu().numpy())


def test_default_fresh_sweep_keeps_the_float64_radius(res):
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    sw = DetectorSweep(LinkParams(), n_reservoir=100, reservoirs="fresh")
    assert sw.radius_precision == "f64" and sw.radius_squarings == 24 and sw.FRESH_BYTES_PER_BLOCK_N2 == 40
    sw.run([6, 21], 7, frames_per_block=2, chunk_blocks=7)
    assert sw.fresh_radius_hits == 7
    want = res.generate(sw.n_in, sw.n_out, 100, 0.9, 0.1, sw.reservoir_seed, first_set=5, n_sets=1)
    for got, w in zip(sw.bank.weights, want[:3]):
        assert np.array_equal(got[5].cpu().numpy(), w[0].cpu().numpy())
    with pytest.raises(ValueError, match="radius_precision"):
        DetectorSweep(LinkParams(), n_reservoir=100, reservoirs="fresh", radius_precision="f16")
