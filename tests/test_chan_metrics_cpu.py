"""CPU-only checks of the channel rank / condition / capacity record (esn_channel_metrics, include/esn_hip.h): the
entry point is declared, exported and bound; its argument errors come back before anything touches a device; the ABI
number is unchanged (the addition is purely additive); no kernel instance uses scratch; the fixture made from the
reference's own statements (tests/golden/make_chan_metrics_golden.py) is self-consistent; and the device-side
percentile helper is np.percentile's default rule."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chan_metrics.npz")


@pytest.fixture(scope="module")
def lib():
    from esn_ofdm_mimo_amd import build, _lib
    build.build_library(verbose=False)
    return _lib.load()


def declared_functions():
    src = open(os.path.join(ROOT, "include", "esn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(esn_[a-z_0-9]+)\s*\(", src)))


def test_declared_exported_and_bound(lib):
    from esn_ofdm_mimo_amd import _lib
    assert "esn_channel_metrics" in declared_functions()
    raw = C.CDLL(os.path.join(ROOT, "esn_ofdm_mimo_amd", "libesn_hip.so"))
    assert hasattr(raw, "esn_channel_metrics")
    assert "esn_channel_metrics" in _lib.SIGNATURES
    assert sorted(_lib.SIGNATURES) == declared_functions()
    assert len(_lib.SIGNATURES["esn_channel_metrics"][1]) == 12


def test_abi_version_is_unchanged(lib):
    from esn_ofdm_mimo_amd import _lib
    assert lib.esn_abi_version() == 10 and _lib.ABI_VERSION == 10


def test_argument_errors(lib):
    p = 64                                   # never dereferenced: the checks run first
    good = dict(H=p, p_i=p, S=None, cond=p, rank=p, cap=p)

    def call(n_t=4, n_r=8, n_blocks=1, n_sub=128, **kw):
        a = dict(good, **kw)
        return lib.esn_channel_metrics(n_blocks, n_sub, n_t, n_r, a["H"], a["p_i"], 1e-5, a["S"], a["cond"], a["rank"],
                                       a["cap"], None)

    for name in ("H", "p_i", "cond", "rank", "cap"):
        assert call(**{name: None}) == -1, name
        err = lib.esn_last_error()
        assert b"esn_channel_metrics" in err and b"null pointer" in err, (name, err)
    for n_t, n_r in ((5, 8), (4, 9), (8, 5), (9, 1), (5, 5)):
        assert call(n_t=n_t, n_r=n_r) == -1, (n_t, n_r)
        assert b"unsupported" in lib.esn_last_error(), (n_t, n_r)
    assert call(n_blocks=0) == -1 and b"invalid sizes" in lib.esn_last_error()
    assert call(n_sub=0) == -1 and call(n_t=0) == -1 and call(n_r=-1) == -1
    assert call(H=72) == -1 and b"aligned" in lib.esn_last_error()


def test_no_kernel_instance_uses_scratch(tmp_path):
    """The 8 x 4 complex matrix of a lane must stay in registers: private_segment_fixed_size 0 in the gfx950 code object
    metadata of every channel_metrics instance (parsed as tools/skew16_isa.py parses its kernel's)."""
    from esn_ofdm_mimo_amd import build
    asm = tmp_path / "esn_chanstat.s"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, *build.FLAGS, "--cuda-device-only", "-S",
                           os.path.join(build.CSRC, "esn_chanstat.hip"), "-o", str(asm)])
    meta, cur = {}, None
    for ln in asm.read_text().splitlines():
        m = re.match(r"^\s+\.name:\s+(\S+)", ln)
        if m:
            cur = meta.setdefault(m.group(1), {}) if "channel_metrics_kernel" in m.group(1) else None
        m = re.match(r"^\s+\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    # the four reference shapes and the generic instance
    for inst in ("ILi1ELi1EE", "ILi1ELi2EE", "ILi2ELi2EE", "ILi4ELi8EE", "ILi0ELi0EE"):
        assert any(inst in name for name in meta), (inst, sorted(meta))
    for name, kv in meta.items():
        assert kv["private_segment_fixed_size"] == 0, (name, kv)
        assert kv["vgpr_spill_count"] == 0 and kv["vgpr_count"] <= 256, (name, kv)


def cases():
    z = np.load(GOLDEN)
    return z, [str(c) for c in z["cases"]]


def test_fixture_covers_the_cases():
    z, names = cases()
    shapes = {n: z[n + "_taps"].shape[1:3] for n in names}                 # (n_r, n_t)
    assert {(1, 1), (2, 1), (2, 2), (8, 4), (2, 4)} <= set(shapes.values())
    for n in ("siso", "simo12", "mimo22", "mimo48", "nr2_nt4"):
        assert list(z[n + "_ebno"]) == [0, 12, 24]
    assert list(z["loop_nbf_ebno"]) == [12, 18] and z["loop_nbf_taps"].shape[0] == 3
    for n in ("zeros", "dup_columns", "zero_column", "scaled_1e-13", "scaled_1e8"):
        assert n in names
    assert not z["zeros_taps"].any() and not z["zeros_S"].any() and not z["zeros_e0_ranks"].any()
    assert not z["zeros_conds"].any() and not z["zeros_e0_cap_k"].any()
    assert np.array_equal(z["dup_columns_taps"][:, :, 2], z["dup_columns_taps"][:, :, 0])
    assert (z["dup_columns_S"][..., -1] < 1e-12 * z["dup_columns_S"][..., 0]).all()
    assert not z["zero_column_taps"][:, :, 1].any() and (z["zero_column_S"][..., -1] < 1e-14).all()
    assert (z["scaled_1e-13_S"][..., -1] < 1e-12).all()                   # the clamp of :381 is active
    assert (z["scaled_1e8_S"][..., 0] > 1e7).all()
    assert os.path.getsize(GOLDEN) <= 220 * 1024


def test_fixture_is_self_consistent():
    z, names = cases()
    for n in names:
        taps, S, conds = z[n + "_taps"], z[n + "_S"], z[n + "_conds"]
        n_r, n_t = taps.shape[1:3]
        assert S.shape == (taps.shape[0], int(z["n_sub"]), min(n_t, n_r)) and conds.shape == S.shape[:2]
        assert (np.diff(S, axis=-1) <= 0).all()
        assert np.array_equal(conds, S[..., 0] / np.maximum(S[..., -1], 1e-12))
        for e, p_i in enumerate(z[n + "_p_i"]):
            ranks, cap_k, agg = z[f"{n}_e{e}_ranks"], z[f"{n}_e{e}_cap_k"], z[f"{n}_e{e}_agg"]
            assert agg[0] == np.mean(np.mean(cap_k, axis=1)), n
            assert agg[1] == np.mean(ranks.ravel() >= min(n_t, n_r)), n
            assert agg[2] == np.percentile(conds.ravel(), 50) and agg[3] == np.percentile(conds.ravel(), 90), n
            thr = np.maximum(1e-2 * S[..., :1] ** 2, 10 * (float(z["no"]) / p_i))
            assert np.array_equal(ranks, (S ** 2 >= thr).sum(-1)), n
            margin = float(z[f"{n}_e{e}_margin"])
            assert margin == np.abs(S ** 2 / thr - 1).min() and margin >= 1e-6, (n, e, margin)
            assert abs(p_i / (10 ** (float(z[n + "_ebno"][e]) / 10) * float(z["no"])) - 1) < 1e-15


@pytest.mark.parametrize("n", [1, 2, 3, 128, 2_600_000])
def test_percentile_helper_is_numpy_linear_rule(n):
    import torch
    from esn_ofdm_mimo_amd.montecarlo import percentiles_linear
    x = np.random.RandomState(n).lognormal(1.0, 1.5, size=n)
    got = percentiles_linear(torch.from_numpy(x), (50, 90)).numpy()
    assert np.array_equal(got, np.percentile(x, [50, 90]))


def test_summary_on_cpu_tensors_matches_the_fixture_aggregates():
    import torch
    from esn_ofdm_mimo_amd.montecarlo import summarize_channel_metrics
    z, names = cases()
    for n in names:
        n_r, n_t = z[n + "_taps"].shape[1:3]
        for e in range(len(z[n + "_ebno"])):
            cap = torch.from_numpy(np.array([np.mean(c) for c in z[f"{n}_e{e}_cap_k"]]))
            got = summarize_channel_metrics(torch.from_numpy(z[n + "_conds"]), torch.from_numpy(z[f"{n}_e{e}_ranks"]),
                                            cap, n_t, n_r)
            agg = z[f"{n}_e{e}_agg"]
            assert all(type(v) is float for v in got.values())
            assert got["frac_rank_ge_full"] == agg[1] and got["cond_p50"] == agg[2] and got["cond_p90"] == agg[3]
            assert abs(got["capacity_bits_per_sc"] - agg[0]) <= 1e-14 * (1 + abs(agg[0]))
