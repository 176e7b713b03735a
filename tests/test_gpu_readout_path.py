"""The one call path from ReservoirBank.solve / resolve_failed to the read-out kernels (float64, no cluster kernel):

1. a repair QR-solves the flagged groups under their OWN teacher scalings -- its row is bitwise the row of a QR solve
   of the whole batch -- leaves the other rows alone and never reassigns the bank's scalings; for the pinv, ridge and
   ridge_grid fits, and at the smallest workspace-Cholesky shape (Gram dimension 129);
2. float32 extended states and the same values as float64 give, each, the W_out bytes the commit named in
   tests/golden/readout_path_parent_digests.json gave: the distance between the two has not grown;
3. a group whose status says the harvest timed out (-9: its states were never written) is never repaired:
   resolve_failed and DetectorSweep.repair_fit raise and leave W_out as it was.

Every system here is tall (40 x 24, 140 x 129), so the Gram matrix is E^T E and the consistent duplicate that makes
group 1's singular is a duplicated COLUMN (test_gpu_ridge._rank_deficient duplicates a row of its wide system)."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_readout_path_digests",
                                               os.path.join(ROOT, "tools", "record_readout_path_digests.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

RIDGE, GRID = [1e-3, 0.5, 1e-3], [1e-300, 1e-3]


def deficient(n_res, t):
    import torch
    bank, E, D = rec.bank_for(n_res, t)
    E[1, :, 11] = E[1, :, 3]
    return bank, torch.as_tensor(E, device="cuda"), D


@pytest.mark.parametrize("n_res,t,transient,mode", [(20, 45, 5, "pinv"), (20, 45, 5, "ridge"), (20, 45, 5, "ridge_grid"),
                                                    (125, 140, 0, "pinv")])
def test_repair_uses_the_groups_own_scalings_and_leaves_the_bank_alone(n_res, t, transient, mode):
    import torch
    bank, E, D = deficient(n_res, t)
    kw = {"pinv": {}, "ridge": {"ridge": RIDGE}, "ridge_grid": {"ridge_grid": GRID}}[mode]
    # (a group without a choice is re-solved at its largest finite candidate)
    W_qr, st_qr = bank.solve(E, D, transient, method="qr", **({"ridge": max(GRID)} if mode == "ridge_grid" else kw))
    W, st = bank.solve(E, D, transient, method="chol", **kw)
    if mode == "pinv":
        assert st.cpu().tolist() == [0, 1, 0]
    else:
        assert st.cpu().tolist() == [0, 0, 0]
        st[1] = 1                                   # flagged by hand
    before = W.clone()
    t_scale, t_shift = bank.t_scale, bank.t_shift
    assert bank.resolve_failed(E, D, transient, W, st, **kw) == 1
    assert bank.t_scale is t_scale and bank.t_shift is t_shift
    assert torch.equal(W[1], W_qr[1]) and not torch.equal(W[1], before[1])
    assert torch.equal(st, st_qr)
    assert torch.equal(W[0], before[0]) and torch.equal(W[2], before[2])
    if mode == "ridge_grid":
        assert float(bank.last_ridge_lambda[1]) == max(GRID)


def test_float32_and_float64_states_give_the_recorded_bytes():
    with open(rec.GOLDEN) as f:
        doc = json.load(f)
    assert doc["seed"] == rec.SEED and len(doc["commit"]) >= 7
    d32, d64, rel = rec.f32_f64_pair()
    print(f"float32 vs float64 states: {rel:.3e} relative (commit {doc['commit']}: {doc['relative_difference']:.3e})")
    assert d32 == doc["w_out_f32_states"], f"W_out from float32 states differs from commit {doc['commit']}"
    assert d64 == doc["w_out_f64_states"], f"W_out from float64 states differs from commit {doc['commit']}"
    assert rel == doc["relative_difference"]


def test_a_timed_out_harvest_is_never_repaired():
    import torch
    from esn_ofdm_mimo_amd import _lib, batched
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    rs = np.random.RandomState(5)
    _, D, t_scale, t_shift = rec.arrays()
    U = rs.randn(rec.G, rec.T, rec.N_IN)
    bank = batched.ReservoirBank(rec.N_IN, rec.N_OUT, rec.N_RES, 0.1 * rs.randn(rec.N_RES, rec.N_RES),
                                 rs.rand(rec.N_RES, rec.N_IN) - 0.5, 0.1 * (rs.rand(rec.N_RES, rec.N_OUT) - 0.5))
    bank.set_scaling(None, None, t_scale, t_shift)
    E = bank.fit(U, D, transient=rec.TRANSIENT, method="chol", noise_mode="none")
    assert bank.fit_status.cpu().tolist() == [0, 0, 0]
    bank.fit_status[1] = -9
    before = bank.W_out.clone()
    with pytest.raises(_lib.EsnHipError, match="timed out"):
        bank.resolve_failed(E, D, rec.TRANSIENT, bank.W_out, bank.fit_status)
    assert torch.equal(bank.W_out, before) and bank.fit_status.cpu().tolist() == [0, -9, 0]

    sweep = DetectorSweep(LinkParams(), n_reservoir=64)
    data = sweep.src.blocks_fast(12.0, 0, 0, 2, 1)
    sweep.set_snr(12.0, 2)
    E = sweep.train(data["pilot_y"], data["pilot_x"])
    assert sweep.bank.fit_status.cpu().tolist() == [0, 0]
    sweep.bank.fit_status[1] = -9
    before = sweep.bank.W_out.clone()
    with pytest.raises(_lib.EsnHipError, match="timed out"):
        sweep.repair_fit(E)
    assert torch.equal(sweep.bank.W_out, before)
