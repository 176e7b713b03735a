"""Reservoirs drawn on the device: the spectral-radius kernel against its NumPy restatement
(tests/specrad_ref.py) and against np.linalg.eigvals, the generator against NumPy on supplied uniforms and its own
Philox streams, and the plumbing through ReservoirBank and DetectorSweep(reservoirs="fresh" / radius="device").

Bounds: kernel vs restatement 1e-12 relative (summation order only: a NumPy proxy that summed the product in another
order moved by 7e-16, and the 2^(K-1) divisor suppresses late round-off); kernel vs eigvals 1e-6 relative (16 x the worst
6.3e-8 of the method itself at K = 24)."""
import numpy as np
import pytest

import specrad_ref as sr

pytestmark = pytest.mark.gpu

CASES = sr.cases()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


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
    """The cases of one (n, sparsity): batches of 5 (one for n = 512)."""
    keys = {}
    for c in CASES:
        keys.setdefault(c[:2], []).append(c)
    return keys


# ---- 1. radius: kernel vs restatement vs eigvals ---------------------------------------------------------------------
def test_radius_matches_restatement_and_eigvals(res, mats):
    worst = {24: 0.0, 16: 0.0, "eig": 0.0}
    for (n, sp), cs in _groups().items():
        stack = np.stack([mats[c][0] for c in cs])
        for k, col in ((24, 2), (16, 3)):
            got5, st5 = res.spectral_radius(stack, n_squarings=k, return_status=True)     # S = 5 (1 at n = 512)
            got1, st1 = res.spectral_radius(stack[0], n_squarings=k, return_status=True)  # S = 1
            got5, got1 = got5.cpu().numpy(), float(got1.cpu())
            assert not st5.cpu().numpy().any() and int(st1.cpu()) == 0
            assert got1 == got5[0], (n, sp, k)
            for c, g in zip(cs, got5):
                want = mats[c][col]
                rel = abs(g - want) / want
                worst[k] = max(worst[k], rel)
                assert rel <= 1e-12, (c, k, rel)
                if k == 24:
                    rel_e = abs(g - mats[c][1]) / mats[c][1]
                    worst["eig"] = max(worst["eig"], rel_e)
                    assert rel_e <= 1e-6, (c, rel_e)
    print(f"kernel vs restatement: worst relative {worst[24]:.2e} (K = 24), {worst[16]:.2e} (K = 16); "
          f"kernel vs eigvals (K = 24): {worst['eig']:.2e}; {len(CASES)} matrices")


# ---- 2. batch invariance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 16, 33, 100, 130, 300])
def test_radius_is_bitwise_the_same_alone_and_in_a_batch(res, mats, n):
    cs = _groups()[(n, 0.1)]
    stack = np.stack([mats[c][0] for c in cs])
    batch = res.spectral_radius(stack).cpu().numpy()
    alone = float(res.spectral_radius(stack[3]).cpu())
    assert batch.shape == (5,) and alone == batch[3]


def _big(n, count, seed):
    """`count` reference-distribution matrices of a size beyond the eigvals-checked set (no eigvals taken)."""
    return np.stack([sr.reference_matrix(n, 0.1, seed + i) for i in range(count)])


def test_radius_at_512_is_bitwise_the_same_alone_and_in_a_batch_of_five(res):
    """64 workgroup tiles per matrix and blockIdx.y > 0: the stride between the matrices' workspaces and the sum of 64
    tile partials; also against the restatement (1e-12) for two of the five."""
    stack = _big(512, 5, 9100)
    batch, status = res.spectral_radius(stack, return_status=True)
    batch = batch.cpu().numpy()
    assert not status.cpu().numpy().any()
    for i in (0, 3, 4):
        assert float(res.spectral_radius(stack[i]).cpu()) == batch[i], i
    assert len(set(batch.tolist())) == 5
    for i in (1, 3):
        want = sr.specrad(stack[i], 24)[0]
        assert abs(batch[i] - want) <= 1e-12 * want, (i, batch[i], want)


def test_radius_beyond_512_with_a_ragged_edge(res):
    """n = 600 (padded to 640: 100 tiles, more partials than one pass of the first 64 lanes) in a batch of 2."""
    stack = _big(600, 2, 9200)
    batch = res.spectral_radius(stack).cpu().numpy()
    assert float(res.spectral_radius(stack[1]).cpu()) == batch[1]
    for i in range(2):
        want = sr.specrad(stack[i], 24)[0]
        assert abs(batch[i] - want) <= 1e-12 * want, (i, batch[i], want)


# ---- 3. status -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 130, 512])
def test_zero_matrix_is_flagged_and_leaves_its_neighbours_alone(res, mats, torch, n):
    if n == 512:
        a, b = _big(512, 2, 9100)
    else:
        cs = _groups()[(n, 0.1)]
        a, b = mats[cs[0]][0], mats[cs[1]][0]
    r3, s3 = res.spectral_radius(np.stack([a, np.zeros_like(a), b]), return_status=True)
    r2, s2 = res.spectral_radius(np.stack([a, b]), return_status=True)
    r3, s3, r2, s2 = (t.cpu().numpy() for t in (r3, s3, r2, s2))
    assert s3.tolist() == [0, 1, 0] and s2.tolist() == [0, 0]
    assert r3[1] == 0.0 and r3[0] == r2[0] and r3[2] == r2[1]
    # a nilpotent matrix (strictly upper triangular) is flagged too
    r, s = res.spectral_radius(np.triu(np.ones((n, n)), 1), return_status=True)
    assert int(s.cpu()) == 1 and float(r.cpu()) == 0.0


def test_generate_raises_on_a_flagged_set(res):
    from esn_ofdm_mimo_amd._lib import EsnHipError
    with pytest.raises(EsnHipError, match=r"weight set\(s\) \[4, 5\]"):
        res.generate(4, 2, 33, 0.9, 1.0, 3, first_set=4, n_sets=2)        # sparsity 1: every entry masked, W = 0
    W, _, _, radius, status = res.generate(4, 2, 33, 0.9, 1.0, 3, first_set=4, n_sets=2, check_status=False)
    assert status.cpu().tolist() == [1, 1] and radius.cpu().tolist() == [0.0, 0.0] and not W.cpu().numpy().any()


# ---- 4. supplied uniforms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, n_in, n_out", [(33, 4, 2), (130, 16, 8)])
@pytest.mark.parametrize("sparsity", [0.1, 0.0])
def test_supplied_uniforms_give_numpy_bits_and_the_host_scale(res, n, n_in, n_out, sparsity):
    from esn_ofdm_mimo_amd.montecarlo import draw_reservoir
    seed, rho = 1234 + n, 0.9
    rs = np.random.RandomState(seed)
    u_w, u_m, u_in, u_fb = rs.rand(n, n), rs.rand(n, n), rs.rand(n, n_in), rs.rand(n, n_out)
    u = np.concatenate([x.ravel() for x in (u_w, u_m, u_in, u_fb)])[None]
    want_w = u_w - 0.5
    want_w[u_m < sparsity] = 0
    # unscaled: rho / radius == 1 cannot be asked for, so read W before the scale through the library calls
    import torch
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    W = torch.empty((1, n, n), dtype=torch.float64, device=dev)
    W_in = torch.empty((1, n, n_in), dtype=torch.float64, device=dev)
    W_fb = torch.empty((1, n, n_out), dtype=torch.float64, device=dev)
    ud = torch.as_tensor(u, device=dev)
    _lib.check(lib.esn_gen_reservoirs(n, n_in, n_out, sparsity, 0, 0, 1, ud.data_ptr(), W.data_ptr(), W_in.data_ptr(),
                                      W_fb.data_ptr(), _lib.stream_handle()), "esn_gen_reservoirs")
    assert np.array_equal(W[0].cpu().numpy(), want_w)
    assert np.array_equal(W_in[0].cpu().numpy(), u_in * 2 - 1)
    assert np.array_equal(W_fb[0].cpu().numpy(), u_fb * 2 - 1)
    # scaled: against the host path on the same seed
    Ws, Wi, Wf, radius, status = res.generate(n_in, n_out, n, rho, sparsity, 0, uniforms=u)
    hw, hin, hfb = draw_reservoir(n_in, n_out, n, rho, sparsity, seed)
    got = Ws[0].cpu().numpy()
    assert np.abs(got - hw).max() <= 1e-6 * np.abs(hw).max()
    assert np.array_equal(Wi[0].cpu().numpy(), hin) and np.array_equal(Wf[0].cpu().numpy(), hfb)
    eig = np.max(np.abs(np.linalg.eigvals(got)))
    assert abs(eig - rho) <= 1e-6 * rho
    assert np.array_equal(got, want_w * (rho / float(radius[0].cpu())))


# ---- 5. Philox streams ---------------------------------------------------------------------------------------------
def test_a_set_is_the_same_bits_in_any_batch_and_sits_in_its_slot(res):
    args = (4, 2, 33, 0.9, 0.1, 77)
    batch = [t.cpu().numpy() for t in res.generate(*args, first_set=0, n_sets=5)]
    for s in range(5):
        one = [t.cpu().numpy() for t in res.generate(*args, first_set=s, n_sets=1)]
        for b, o in zip(batch, one):
            assert np.array_equal(b[s], o[0]), s
    shifted = [t.cpu().numpy() for t in res.generate(*args, first_set=3, n_sets=5)]       # sets 3..7: set 6 in slot 1
    six = [t.cpu().numpy() for t in res.generate(*args, first_set=6, n_sets=1)]
    for b, o in zip(shifted, six):
        assert np.array_equal(b[1], o[0])
    for b, o in zip(shifted, batch):                                                      # sets 3 and 4 keep slots 3, 4
        assert np.array_equal(b[3], o[3]) and np.array_equal(b[4], o[4])
    other = res.generate(4, 2, 33, 0.9, 0.1, 78, first_set=0, n_sets=1)[0].cpu().numpy()
    assert not np.array_equal(other[0], batch[0][0])
    assert not np.array_equal(batch[0][0], batch[0][1])


def test_philox_draw_has_the_reference_distribution(res):
    import torch
    from esn_ofdm_mimo_amd import _lib
    n, n_in, n_out, p = 300, 8, 4, 0.1
    lib = _lib.load()
    dev = torch.device("cuda:0")
    W = torch.empty((1, n, n), dtype=torch.float64, device=dev)
    W_in = torch.empty((1, n, n_in), dtype=torch.float64, device=dev)
    W_fb = torch.empty((1, n, n_out), dtype=torch.float64, device=dev)
    _lib.check(lib.esn_gen_reservoirs(n, n_in, n_out, p, 5, 0, 1, None, W.data_ptr(), W_in.data_ptr(), W_fb.data_ptr(),
                                      _lib.stream_handle()), "esn_gen_reservoirs")
    w, w_in, w_fb = W[0].cpu().numpy(), W_in[0].cpu().numpy(), W_fb[0].cpu().numpy()
    zero = (w == 0).mean()
    assert abs(zero - p) <= 5 * np.sqrt(p * (1 - p) / n ** 2), zero
    live = w[w != 0]
    assert abs(live.mean()) <= 5 * np.sqrt(1 / 12 / live.size), live.mean()
    assert abs(w_in.mean()) <= 5 * np.sqrt(1 / 3 / w_in.size), w_in.mean()
    assert abs(w_fb.mean()) <= 5 * np.sqrt(1 / 3 / w_fb.size), w_fb.mean()
    assert w.min() >= -0.5 and w.max() < 0.5
    assert w_in.min() >= -1.0 and w_in.max() < 1.0 and w_fb.min() >= -1.0 and w_fb.max() < 1.0


# ---- 6. bank plumbing ----------------------------------------------------------------------------------------------
def _bank_outputs(bank, n_in, n_out, prec, rng_seed=11):
    rs = np.random.RandomState(rng_seed)
    g, f, t, tr = 5, 3, 40, 5
    U, D = rs.randn(g, t, n_in) * 0.3, rs.randn(g, t, n_out) * 0.3
    X = rs.randn(g * f, t, n_in) * 0.3
    E = bank.harvest(U, D, precision=prec, noise_mode="counter", seed=9, group_offset=7)
    bank.fit(U, D, transient=tr, precision=prec, noise_mode="counter", seed=9, group_offset=7)
    Y = bank.predict(X, f, transient=tr, precision=prec, noise_mode="counter", seed=10, group_offset=7)
    return E.cpu().numpy(), Y.cpu().numpy()


@pytest.mark.parametrize("n_res, prec", [(64, "f64"), (64, "f16"), (300, "f16")])
def test_generated_bank_equals_a_bank_built_from_its_weights(n_res, prec):
    from esn_ofdm_mimo_amd.batched import ReservoirBank
    gen = ReservoirBank.generate(4, 2, n_res, 0.9, 0.1, seed=21, first_set=0, n_sets=5)
    assert gen.n_wsets == 5 and gen.shape.n_wsets == 5
    host = ReservoirBank(4, 2, n_res, *(w.cpu().numpy() for w in gen.weights))
    e1, y1 = _bank_outputs(gen, 4, 2, prec)
    e2, y2 = _bank_outputs(host, 4, 2, prec)
    assert np.array_equal(e1, e2) and np.array_equal(y1, y2)
    assert np.isfinite(y1).all() and np.abs(y1).max() > 0


def test_set_weights_after_a_predict_takes_effect(res):
    from esn_ofdm_mimo_amd.batched import ReservoirBank
    bank = ReservoirBank.generate(4, 2, 64, 0.9, 0.1, seed=21, first_set=0, n_sets=5)
    _, y_old = _bank_outputs(bank, 4, 2, "f16")
    W, W_in, W_fb, _, _ = res.generate(4, 2, 64, 0.9, 0.1, 22, first_set=0, n_sets=3)
    bank.set_weights(W, W_in, W_fb)
    assert bank.n_wsets == 3 and bank.shape.n_wsets == 3 and bank.weights[0].data_ptr() == W.data_ptr()
    _, y_new = _bank_outputs(bank, 4, 2, "f16")
    other = ReservoirBank(4, 2, 64, W.cpu().numpy(), W_in.cpu().numpy(), W_fb.cpu().numpy())
    _, y_want = _bank_outputs(other, 4, 2, "f16")
    assert np.array_equal(y_new, y_want) and not np.array_equal(y_new, y_old)


# ---- 7. sweep ------------------------------------------------------------------------------------------------------
def test_fresh_sweep_counts_do_not_depend_on_the_chunking(res):
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    sw = DetectorSweep(LinkParams(), n_reservoir=100, reservoirs="fresh")
    ber_c, cnt_c = sw.run([6, 21], 7, frames_per_block=2, chunk_blocks=3)
    ber_u, cnt_u = sw.run([6, 21], 7, frames_per_block=2, chunk_blocks=7)
    assert np.array_equal(cnt_c, cnt_u)
    assert cnt_u[:, 1].min() > 0 and ber_u[1] < ber_u[0]
    # the unchunked run left blocks 0..6 in the bank, block b in slot b
    assert sw.bank.n_wsets == 7
    want = res.generate(sw.n_in, sw.n_out, 100, 0.9, 0.1, sw.reservoir_seed, first_set=5, n_sets=1)
    for got, w in zip(sw.bank.weights, want[:3]):
        assert np.array_equal(got[5].cpu().numpy(), w[0].cpu().numpy())


def test_fresh_sweep_default_chunk_is_bounded_by_memory_and_changes_no_counter():
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    sw = DetectorSweep(LinkParams(), n_reservoir=100, reservoirs="fresh")
    shared = DetectorSweep(LinkParams(), n_reservoir=100, reservoirs="shared")
    per_block = sw.FRESH_BYTES_PER_BLOCK_N2 * 100 ** 2
    assert sw.default_chunk_blocks(2) == min(shared.default_chunk_blocks(2), sw.FRESH_BUDGET_BYTES // per_block)
    _, want = sw.run([21], 7, frames_per_block=2, chunk_blocks=7)
    sw.FRESH_BUDGET_BYTES = 3 * per_block + 1                 # room for three blocks: the bound is what cuts the chunks
    assert sw.default_chunk_blocks(2) == 3
    _, got = sw.run([21], 7, frames_per_block=2)              # default chunk
    assert np.array_equal(got, want) and sw.bank.n_wsets == 1  # (the last chunk holds block 6 alone)
    sw.FRESH_BUDGET_BYTES = 1                                 # never less than one block
    assert sw.default_chunk_blocks(2) == 1


def test_fresh_sweep_counts_do_not_depend_on_the_world_size():
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    _, one = DetectorSweep(LinkParams(), n_reservoir=100, reservoirs="fresh").run([6, 21], 7, frames_per_block=2)
    parts = [DetectorSweep(LinkParams(), n_reservoir=100, reservoirs="fresh", rank=r, world_size=3)
             .run([6, 21], 7, frames_per_block=2, chunk_blocks=2)[1] for r in range(3)]
    assert np.array_equal(sum(parts), one)


def test_single_point_drivers_refuse_a_fresh_sweep():
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams, block_fading_point, coded_ber_point
    sw = DetectorSweep(LinkParams(), n_reservoir=100, reservoirs="fresh")
    with pytest.raises(ValueError, match="fresh"):
        coded_ber_point(sw, None, 12.0, 0, 2)
    with pytest.raises(ValueError, match="fresh"):
        block_fading_point(sw, None, 12.0, 0, 2)


def test_device_radius_matches_the_host_bank_and_host_stays_the_default():
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams, draw_reservoir
    p = LinkParams()
    host = DetectorSweep(p, n_reservoir=100, reservoirs="shared", seed=3)
    dev = DetectorSweep(p, n_reservoir=100, reservoirs="shared", seed=3, radius="device")
    hw, hin, hfb = draw_reservoir(host.n_in, host.n_out, 100, 0.9, 0.1, 3 * 7919 + 17)
    gw, gin, gfb = (t[0].cpu().numpy() for t in host.bank.weights)
    assert np.array_equal(gw, hw) and np.array_equal(gin, hin) and np.array_equal(gfb, hfb)
    dw, din, dfb = (t[0].cpu().numpy() for t in dev.bank.weights)
    assert np.abs(dw - hw).max() <= 1e-6 * np.abs(hw).max()
    assert np.array_equal(din, hin) and np.array_equal(dfb, hfb)
    pool = DetectorSweep(p, n_reservoir=100, reservoirs="per_block", pool=2, seed=3, radius="device")
    assert pool.bank.n_wsets == 2
    h1 = draw_reservoir(host.n_in, host.n_out, 100, 0.9, 0.1, 3 * 7919 + 18)[0]
    assert np.abs(pool.bank.weights[0][1].cpu().numpy() - h1).max() <= 1e-6 * np.abs(h1).max()
