"""Several pilots per block without a GPU: the NumPy restatement of the hold-out score and choice
(tests/multipilot_ref.py) against an independent form, the typing and the refusals of esn_readout_holdout_score
through ctypes, the refusals of ReservoirBank.fit_pilots and DetectorSweep(n_pilots=...) that come before any device
is touched, and the finding that motivates the feature, on the CPU oracle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multipilot_ref as ref  # noqa: E402


def _pilots(P, rows, cols, n_out, seed):
    """P pilots of one group: states with uneven column scales, the teacher a linear map of them plus 30 % noise."""
    rs = np.random.RandomState(seed)
    scale = 10.0 ** rs.uniform(-2.0, 0.0, size=cols)
    truth = rs.randn(cols, n_out)
    Es = [rs.randn(rows, cols) * scale for _ in range(P)]
    Dss = []
    for E in Es:
        clean = E @ truth
        Dss.append(clean + 0.3 * np.std(clean) * rs.randn(rows, n_out))
    return Es, Dss


@pytest.mark.parametrize("P,rows,cols,n_out", [(2, 30, 50, 2), (3, 40, 24, 1), (4, 16, 70, 4)])
def test_restatement_against_lstsq_on_the_augmented_system(P, rows, cols, n_out):
    Es, Dss = _pilots(P, rows, cols, n_out, 1000 * P + cols)
    E_fit, D_fit = np.concatenate(Es[:-1]), np.concatenate(Dss[:-1])
    grid = np.sum(E_fit * E_fit) / min(E_fit.shape) * np.array([1e-6, 1e-3, 1e-1, 10.0])
    got = ref.fit_pilots(Es, Dss, grid=grid)
    # independent: ridge as least squares of [E; sqrt(lam) I] against [Ds; 0], the score as a plain loop
    want = np.zeros(len(grid))
    for l, lam in enumerate(grid):
        A = np.vstack([E_fit, np.sqrt(lam) * np.eye(cols)])
        B = np.vstack([D_fit, np.zeros((cols, n_out))])
        Wt = np.linalg.lstsq(A, B, rcond=None)[0]                      # [cols, n_out]
        for i in range(rows):
            for o in range(n_out):
                want[l] += (Es[-1][i] @ Wt[:, o] - Dss[-1][i, o]) ** 2
    rel = np.abs(got["scores"] - want) / want
    print(f"P={P} [{rows} x {cols}] n_out={n_out}: scores rel {rel.max():.2e}, choice {got['choice']}")
    assert rel.max() <= 1e-8
    assert got["choice"] == int(np.argmin(want))
    A = np.vstack([np.concatenate(Es), np.sqrt(got["lam"]) * np.eye(cols)])
    B = np.vstack([np.concatenate(Dss), np.zeros((cols, n_out))])
    W_all = np.linalg.lstsq(A, B, rcond=None)[0].T
    assert np.max(np.abs(got["W_out"] - W_all)) <= 1e-8 * np.max(np.abs(W_all))


def test_choice_rules_of_the_restatement():
    Es, Dss = _pilots(2, 20, 30, 2, 5)
    W = np.stack([ref.ridge(Es[0], Dss[0], lam) for lam in (1e-3, 1e-3, 1.0, 1e-6)])
    s = ref.holdout_scores(Es[1], Dss[1], W)
    assert s[0] == s[1] and ref.choose(s) == int(np.argmin(s)) and ref.choose(s) != 1      # the lowest index wins a tie
    best = ref.choose(s)
    masked = ref.holdout_scores(Es[1], Dss[1], W, status=np.eye(4, dtype=int)[best])
    assert np.isinf(masked[best]) and ref.choose(masked) != best
    Wn = W.copy()
    Wn[2, 0, 3] = np.nan
    assert np.isinf(ref.holdout_scores(Es[1], Dss[1], Wn)[2])
    assert ref.choose(ref.holdout_scores(Es[1], Dss[1], W, status=np.ones(4, dtype=int))) == -1
    bound = ref.score_bound(Es[1], Dss[1], W)
    assert np.all(bound > 0) and np.all(bound < 1e-9 * s)


# ---- the entry points: typed, and every refusal comes back as -1 before any HIP call ------------------------------------
NAMES = ("esn_readout_holdout_score", "esn_readout_holdout_score_f32")


@pytest.fixture(scope="module")
def lib():
    from esn_ofdm_mimo_amd import build, _lib
    build.build_library(verbose=False)
    return _lib.load()


def test_binding_types_the_entry_points(lib):
    from esn_ofdm_mimo_amd import _lib, build
    assert "esn_holdout.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 10 and lib.esn_abi_version() == 10
    for name in NAMES:
        res, args = _lib.SIGNATURES[name]
        assert len(args) == 15 and getattr(lib, name).argtypes == args
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "esn_hip.h")).read()
    for name in NAMES:
        assert name + "(" in header


# E, D, W, n_groups, T, transient, cols, n_out, t_scale, t_shift, n_ridge, status_in, score, choice, stream
# (addresses that are never dereferenced: the checks run first)
GOOD = [64, 64, 128, 3, 45, 5, 72, 4, None, None, 4, None, 192, 256, None]
REFUSALS = [
    ("null E", {0: None}, b"null"), ("null D", {1: None}, b"null"), ("null W", {2: None}, b"null"),
    ("null score", {12: None}, b"null"), ("null choice", {13: None}, b"null"),
    ("n_ridge 0", {10: 0}, b"16"), ("n_ridge 17", {10: 17}, b"16"), ("n_out 9", {7: 9}, b"8"),
    ("transient = T", {5: 45}, b"transient < T"), ("cols 0", {6: 0}, b"cols"),
    ("misaligned E", {0: 72}, b"16-byte"), ("misaligned W", {2: 136}, b"16-byte"),
]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("what,change,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_hip_call(lib, name, what, change, text):
    args = list(GOOD)
    for k, v in change.items():
        args[k] = v
    rc = getattr(lib, name)(*args)
    err = lib.esn_last_error()
    assert rc == -1, (what, rc, err)
    assert name.encode() + b":" in err and text in err, (what, err)


def _bank(n_in=16, n_out=8, n_res=512):
    """A ReservoirBank without a device: what fit_pilots checks before it touches one needs the sizes alone."""
    from esn_ofdm_mimo_amd.batched import ReservoirBank
    bank = ReservoirBank.__new__(ReservoirBank)
    bank.n_inputs, bank.n_outputs, bank.n_reservoir = n_in, n_out, n_res
    return bank


def test_fit_pilots_refuses_before_touching_a_device():
    bank = _bank()
    U, D = np.zeros((2, 5, 138, 16)), np.zeros((2, 5, 138, 8))          # 5 pilots x 128 rows = 640 > 512
    with pytest.raises(ValueError, match="512"):
        bank.fit_pilots(U, D, transient=10, method="chol")
    with pytest.raises(ValueError, match="not both"):
        bank.fit_pilots(U[:, :4], D[:, :4], transient=10, method="chol", ridge=1e-3, ridge_grid=[1e-3, 1e-2])
    with pytest.raises(ValueError, match="16"):
        bank.fit_pilots(U[:, :4], D[:, :4], transient=10, method="chol", ridge_grid=np.logspace(-8, 0, 17))
    with pytest.raises(ValueError, match=r"\[G, P, T"):
        bank.fit_pilots(U[:, 0], D[:, 0], transient=10)
    # what is served passes these checks: 4 pilots are 512 rows (Cholesky), 5 fall back to QR under "auto"
    assert bank._pilot_fit_method(U[:, :4].shape, D[:, :4].shape, 10, "chol", None, [1e-3, 1e-2]) == "chol"
    assert bank._pilot_fit_method(U.shape, D.shape, 10, "auto", 1e-3, None) == "qr"


def test_detector_sweep_refuses_before_touching_a_device():
    from esn_ofdm_mimo_amd.link import LinkParams
    from esn_ofdm_mimo_amd.sweep import DetectorSweep
    for kw, word in ((dict(track="decisions"), "track"), (dict(train_ebno=15.0), "train_ebno"),
                     (dict(ridge=1e-3, ridge_grid=[1e-3]), "not both"),
                     (dict(ridge_grid=list(np.logspace(-8, 0, 17))), "16")):
        with pytest.raises(ValueError, match=word):
            DetectorSweep(LinkParams(), n_pilots=4, **kw)
    with pytest.raises(ValueError, match="continuation"):
        DetectorSweep(LinkParams(continuation=True), n_pilots=2)
    with pytest.raises(ValueError, match="n_pilots"):
        DetectorSweep(LinkParams(), n_pilots=0)


def test_four_pilots_with_the_holdout_choice_beat_one_pilot_and_beat_pinv_on_the_oracle():
    """2 blocks x 6 frames at 21 dB, N_res 512 (6 blocks x 12 frames gave 0.019 / 0.158 / 0.339): orderings only."""
    ber = ref.oracle_finding(n_pilots_max=4, n_blocks=2, n_frames=6, ebno=21.0, n_res=512,
                             cases={(1, "pinv"), (4, "pinv"), (4, "grid")})
    print({k: round(v, 4) for k, v in sorted(ber.items())})
    assert ber[4, "grid"] < ber[1, "pinv"]
    assert ber[4, "pinv"] > ber[4, "grid"]
