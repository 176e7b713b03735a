"""The split-operand spectral radius (esn_spectral_radius_split_workspace_bytes, esn_spectral_radius_split_batch) is plain
C beside the float64 pair: a C99 program declares both through include/esn_hip.h, links against libesn_hip.so and gets
every argument error (-1, the function named in esn_last_error()) back before anything touches a device.  They are
additions: the ABI version stays 10."""
import c_abi

SPLIT_NAMES = ("esn_spectral_radius_split_workspace_bytes", "esn_spectral_radius_split_batch")

C_SRC = r'''
#include <stdio.h>
#include <string.h>
#include "esn_hip.h"
static int named(const char* fn) { return strstr(esn_last_error(), fn) != 0; }
int main(void) {
    /* never dereferenced: the checks run first */
    const double* dp = (const double*)64;
    double* rad = (double*)256;
    int* st = (int*)64;
    void* ws = (void*)64;
    const size_t big = (size_t)1 << 46;
    int s, n, k;
    if (esn_abi_version() != 10) return 1;
    /* null pointers */
    if (esn_spectral_radius_split_batch(0, 3, 33, 24, rad, st, ws, big, 0) != -1 || !named("esn_spectral_radius_split_batch")) return 20;
    if (!strstr(esn_last_error(), "null")) return 19;
    if (esn_spectral_radius_split_batch(dp, 3, 33, 24, 0, st, ws, big, 0) != -1 || !named("esn_spectral_radius_split_batch")) return 21;
    if (esn_spectral_radius_split_batch(dp, 3, 33, 24, rad, 0, ws, big, 0) != -1 || !named("esn_spectral_radius_split_batch")) return 22;
    /* sizes */
    if (esn_spectral_radius_split_batch(dp, 0, 33, 24, rad, st, ws, big, 0) != -1 || !named("esn_spectral_radius_split_batch")) return 23;
    if (esn_spectral_radius_split_batch(dp, -2, 33, 24, rad, st, ws, big, 0) != -1) return 24;
    if (esn_spectral_radius_split_batch(dp, 3, 0, 24, rad, st, ws, big, 0) != -1) return 25;
    if (esn_spectral_radius_split_batch(dp, 3, -33, 24, rad, st, ws, big, 0) != -1) return 26;
    /* K outside 4..32 */
    if (esn_spectral_radius_split_batch(dp, 3, 33, 3, rad, st, ws, big, 0) != -1 || !named("esn_spectral_radius_split_batch")) return 27;
    if (!strstr(esn_last_error(), "n_squarings") || !strstr(esn_last_error(), "32")) return 28;
    if (esn_spectral_radius_split_batch(dp, 3, 33, 33, rad, st, ws, big, 0) != -1 || !named("esn_spectral_radius_split_batch")) return 29;
    if (!strstr(esn_last_error(), "n_squarings")) return 30;
    /* n_res beyond 4096 */
    if (esn_spectral_radius_split_batch(dp, 3, 4097, 24, rad, st, ws, big, 0) != -1 || !named("esn_spectral_radius_split_batch")) return 31;
    if (!strstr(esn_last_error(), "4096")) return 32;
    if (esn_spectral_radius_split_workspace_bytes(3, 4097) != 0 || !named("esn_spectral_radius_split_workspace_bytes")) return 33;
    if (!strstr(esn_last_error(), "4096") || esn_spectral_radius_split_workspace_bytes(3, 4096) == 0) return 34;
    /* workspace: null, short, misaligned */
    if (esn_spectral_radius_split_batch(dp, 3, 33, 24, rad, st, 0, big, 0) != -1 || !named("esn_spectral_radius_split_batch")) return 35;
    if (!strstr(esn_last_error(), "workspace")) return 36;
    if (esn_spectral_radius_split_batch(dp, 3, 33, 24, rad, st, ws, esn_spectral_radius_split_workspace_bytes(3, 33) - 1, 0) != -1) return 37;
    if (!named("esn_spectral_radius_split_batch") || !strstr(esn_last_error(), "workspace")) return 38;
    if (esn_spectral_radius_split_batch(dp, 3, 33, 24, rad, st, (void*)68, big, 0) != -1) return 39;
    /* the workspace query: positive, monotone in n_sets and in n_res, 0 for no sets; two images in two orientations
       as two 2-byte planes fit, and it stays within the float64 path's bytes plus the per-matrix norms */
    if (esn_spectral_radius_split_workspace_bytes(1, 1) == 0) return 50;
    if (esn_spectral_radius_split_workspace_bytes(0, 512) != 0 || esn_spectral_radius_split_workspace_bytes(-1, 512) != 0) return 51;
    if (esn_spectral_radius_split_workspace_bytes(4, 0) != 0) return 52;
    for (s = 1; s < 40; ++s)
        for (n = 1; n < 700; n += 7) {
            if (esn_spectral_radius_split_workspace_bytes(s + 1, n) <= esn_spectral_radius_split_workspace_bytes(s, n)) return 53;
            if (esn_spectral_radius_split_workspace_bytes(s, n + 1) < esn_spectral_radius_split_workspace_bytes(s, n)) return 54;
            if (esn_spectral_radius_split_workspace_bytes(s, n) < (size_t)s * 16 * n * n) return 55;
            if (esn_spectral_radius_split_workspace_bytes(s, n) > esn_spectral_radius_workspace_bytes(s, n) + 16) return 57;
        }
    for (k = 4; k <= 32; ++k)     /* every served K passes the K check (and stops at the workspace one) */
        if (esn_spectral_radius_split_batch(dp, 3, 33, k, rad, st, 0, 0, 0) != -1 || !strstr(esn_last_error(), "workspace")) return 56;
    printf("split radius abi ok\n");
    return 0;
}
'''


def test_split_entry_points_link_from_c99_and_validate_without_a_device(tmp_path):
    r = c_abi.compile_and_run(tmp_path, "split", C_SRC)
    assert "split radius abi ok" in r.stdout


def test_binding_types_the_split_entry_points():
    from esn_ofdm_mimo_amd import _lib, build
    for name in SPLIT_NAMES:
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 10
    assert _lib.SIGNATURES["esn_spectral_radius_split_batch"] == _lib.SIGNATURES["esn_spectral_radius_batch"]
    assert _lib.SIGNATURES["esn_spectral_radius_split_workspace_bytes"] == \
        _lib.SIGNATURES["esn_spectral_radius_workspace_bytes"]
    assert "esn_specrad_split.hip" in build.SOURCES and "esn_reservoir.hip" in build.SOURCES


def test_split_checks_through_the_binding():
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    assert lib.esn_abi_version() == 10
    assert lib.esn_spectral_radius_split_batch(None, 1, 16, 24, None, None, None, 0, None) == -1
    assert b"esn_spectral_radius_split_batch" in lib.esn_last_error()
    assert lib.esn_spectral_radius_split_batch(64, 1, 16, 3, 64, 64, 64, 1 << 40, None) == -1
    assert b"n_squarings" in lib.esn_last_error()
    assert lib.esn_spectral_radius_split_batch(64, 1, 16, 33, 64, 64, 64, 1 << 40, None) == -1
    assert lib.esn_spectral_radius_split_batch(64, 1, 4097, 24, 64, 64, 64, 1 << 40, None) == -1
    assert b"4096" in lib.esn_last_error()
    need = lib.esn_spectral_radius_split_workspace_bytes(1, 16)
    assert lib.esn_spectral_radius_split_batch(64, 1, 16, 24, 64, 64, 64, need - 1, None) == -1
    assert b"workspace" in lib.esn_last_error()
    assert need >= 16 * 16 * 16


def test_python_layers_refuse_an_unknown_radius_precision():
    import pytest
    from esn_ofdm_mimo_amd import reservoirs
    assert sorted(reservoirs.RADIUS_PRECISIONS) == ["f16x2", "f64"]
    with pytest.raises(ValueError, match="f16x2"):
        reservoirs.spectral_radius([[1.0]], precision="f16")
    with pytest.raises(ValueError, match="f16x2"):
        reservoirs.generate(4, 2, 33, 0.9, 0.1, 0, radius_precision="f32")
