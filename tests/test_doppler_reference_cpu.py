"""CPU-only checks around esn_gen_taps_doppler (include/esn_hip.h): the closed-form restatement tests/doppler_ref.py has
the statistics the model promises (autocorrelation J0(2 pi fd_tsym s) per tap, tap powers = the PDP, static at
fd_tsym = 0, unit energy at s = 0 for TDL-B); the entry point is plain C and returns every argument error before a
device is touched; the binding types it and the ABI number stays 10; neither kernel instance uses scratch."""
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c_abi  # noqa: E402
import doppler_ref as dr  # noqa: E402

FD, SYMBOLS = 0.01, (0, 10, 20, 38, 60, 76)


def test_restatement_has_the_jakes_autocorrelation_and_the_pdp():
    rs = np.random.RandomState(20261018)
    ang = dr.draw_angles(rs, 16384, 1, 8)
    dr.check_statistics(dr.taps(1, ang, 8, FD, SYMBOLS), 8, FD, SYMBOLS)


def test_restatement_is_static_without_doppler():
    ang = dr.draw_angles(np.random.RandomState(1), 64, 0, 8)
    for kind, a in ((0, ang), (1, ang[:, :8])):
        h = dr.taps(kind, a, 8, 0.0, (0, 1, 17, 400))
        assert np.array_equal(h, np.repeat(h[:, :1], 4, axis=1)), kind


def test_restatement_tdlb_has_unit_energy_at_the_pilot_instant():
    ang = dr.draw_angles(np.random.RandomState(2), 256, 0, 8)
    h = dr.taps(0, ang, 8, 0.02, (0, 30))
    np.testing.assert_allclose(np.sum(np.abs(h[:, 0]) ** 2, axis=-1), 1.0, rtol=0, atol=1e-13)
    e30 = np.sum(np.abs(h[:, 1]) ** 2, axis=-1)          # afterwards the energy fades as it physically would
    assert np.abs(e30 - 1.0).max() > 0.1
    # the same placement as the block generator's: paths -> taps with the oracle's floor / ceil split
    power, place = dr.pdp(0, 8)
    assert place.shape == (23, 8) and abs(power.sum() - 1) < 1e-15
    assert np.all(place.sum(axis=1) <= 1 + 1e-15) and np.all(place >= 0)


C_SRC = r'''
#include <stdio.h>
#include <string.h>
#include "esn_hip.h"
static int named(void) { return strstr(esn_last_error(), "esn_gen_taps_doppler") != 0; }
static int call(int kind, int nb, int ns, int nr, int nt, int isi, double fd, double* taps) {
    return esn_gen_taps_doppler(kind, nb, ns, nr, nt, isi, 2048000.0, 300.0, fd, 0, 7, 0, taps, 0);
}
int main(void) {
    double* t = (double*)64;      /* never dereferenced: the checks run first */
    volatile double huge = 1e308;
    const double inf = huge * 10.0;
    const double nan = inf - inf;
    if (esn_abi_version() != 10) return 1;
    if (ESN_DOPPLER_SINUSOIDS != 16) return 2;
    if (call(0, 4, 77, 8, 4, 8, 0.01, 0) != -1 || !named() || !strstr(esn_last_error(), "null")) return 3;
    if (call(2, 4, 77, 8, 4, 8, 0.01, t) != -1 || !named() || !strstr(esn_last_error(), "kind")) return 4;
    if (call(-1, 4, 77, 8, 4, 8, 0.01, t) != -1 || !named()) return 5;
    if (call(0, 0, 77, 8, 4, 8, 0.01, t) != -1 || !named()) return 6;
    if (call(0, -2, 77, 8, 4, 8, 0.01, t) != -1 || !named()) return 7;
    if (call(0, 4, 0, 8, 4, 8, 0.01, t) != -1 || !named() || !strstr(esn_last_error(), "n_sym")) return 8;
    if (call(0, 4, 4097, 8, 4, 8, 0.01, t) != -1 || !named() || !strstr(esn_last_error(), "n_sym")) return 9;
    if (call(0, 4, -1, 8, 4, 8, 0.01, t) != -1 || !named()) return 10;
    if (call(1, 4, 77, 8, 4, 0, 0.01, t) != -1 || !named() || !strstr(esn_last_error(), "isi")) return 11;
    if (call(1, 4, 77, 8, 4, 17, 0.01, t) != -1 || !named() || !strstr(esn_last_error(), "isi")) return 12;
    if (call(1, 4, 77, 0, 4, 8, 0.01, t) != -1 || !named()) return 13;
    if (call(1, 4, 77, 8, 0, 8, 0.01, t) != -1 || !named()) return 14;
    if (call(1, 4, 77, -8, 4, 8, 0.01, t) != -1 || !named()) return 15;
    if (call(1, 4, 77, 8, -4, 8, 0.01, t) != -1 || !named()) return 16;
    if (call(1, 4, 77, 8, 4, 8, -1e-9, t) != -1 || !named() || !strstr(esn_last_error(), "fd_tsym")) return 17;
    if (call(1, 4, 77, 8, 4, 8, 0.5000001, t) != -1 || !named() || !strstr(esn_last_error(), "fd_tsym")) return 18;
    if (call(1, 4, 77, 8, 4, 8, inf, t) != -1 || !named()) return 19;
    if (call(1, 4, 77, 8, 4, 8, -inf, t) != -1 || !named()) return 20;
    if (call(1, 4, 77, 8, 4, 8, nan, t) != -1 || !named() || !strstr(esn_last_error(), "fd_tsym")) return 21;
    printf("doppler abi ok\n");
    return 0;
}
'''


def test_entry_point_links_from_c99_and_validates_without_a_device(tmp_path):
    r = c_abi.compile_and_run(tmp_path, "dop", C_SRC)
    assert "doppler abi ok" in r.stdout


def test_binding_types_the_entry_point_and_the_abi_number_stays():
    from esn_ofdm_mimo_amd import _lib
    assert _lib.ABI_VERSION == 10
    assert len(_lib.SIGNATURES["esn_gen_taps_doppler"][1]) == 14
    lib = _lib.load()
    assert lib.esn_abi_version() == 10
    assert lib.esn_gen_taps_doppler(0, 1, 77, 8, 4, 8, 2048000.0, 300.0, 0.01, None, 0, 0, None, None) == -1
    assert b"esn_gen_taps_doppler" in lib.esn_last_error()
    assert lib.esn_gen_taps_doppler(1, 1, 77, 2, 2, 8, 2048000.0, 300.0, 0.6, None, 0, 0, 64, None) == -1
    assert b"fd_tsym" in lib.esn_last_error()


def test_link_params_carry_the_fading_mode():
    import pytest
    from esn_ofdm_mimo_amd.montecarlo import LinkParams
    p = LinkParams()
    assert p.fading == "block"
    assert p.fd_tsym == 100.0 * (128 + 7) / (2 * 1.024e6)
    assert LinkParams(fading="jakes").fading == "jakes"
    with pytest.raises(ValueError):
        LinkParams(fading="rayleigh")
    with pytest.raises(ValueError):
        LinkParams(fading="jakes", channel="awgn")


def test_no_doppler_kernel_instance_uses_scratch(tmp_path):
    """4 M doubles of phasors and rotators per lane (and TDL-B's 23 placement weights) must stay in registers:
    private_segment_fixed_size 0 in the gfx950 code object metadata of both instances."""
    from esn_ofdm_mimo_amd import build
    asm = tmp_path / "esn_gen.s"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, *build.FLAGS, "--cuda-device-only", "-S", os.path.join(build.CSRC, "esn_gen.hip"),
                           "-o", str(asm)])
    meta, cur = {}, None
    for ln in asm.read_text().splitlines():
        m = re.match(r"^\s+\.name:\s+(\S+)", ln)
        if m:
            cur = meta.setdefault(m.group(1), {}) if "gen_taps_doppler_kernel" in m.group(1) else None
        m = re.match(r"^\s+\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    for inst in ("ILi0EE", "ILi1EE"):
        assert any(inst in name for name in meta), (inst, sorted(meta))
    for name, kv in meta.items():
        assert kv["private_segment_fixed_size"] == 0, (name, kv)
        assert kv["vgpr_spill_count"] == 0 and kv["vgpr_count"] <= 256, (name, kv)
