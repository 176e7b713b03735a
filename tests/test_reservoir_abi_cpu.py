"""The device-reservoir entry points (esn_gen_reservoirs, esn_spectral_radius_batch, esn_scale_reservoirs and the
workspace query) are plain C: a C99 program declares them through include/esn_hip.h, links against libesn_hip.so and
gets every argument error (-1, the function named in esn_last_error()) back before anything touches a device.  They
are additions: the ABI version stays 10."""
import c_abi

RES_NAMES = ("esn_gen_reservoirs", "esn_spectral_radius_workspace_bytes", "esn_spectral_radius_batch",
             "esn_scale_reservoirs")

C_SRC = r'''
#include <stdio.h>
#include <string.h>
#include "esn_hip.h"
static int named(const char* fn) { return strstr(esn_last_error(), fn) != 0; }
int main(void) {
    /* never dereferenced: the checks run first */
    const double* dp = (const double*)64;
    double* w = (double*)64;
    double* wi = (double*)128;
    double* wf = (double*)192;
    double* rad = (double*)256;
    int* st = (int*)64;
    void* ws = (void*)64;
    const size_t big = (size_t)1 << 46;
    int s, n, k;
    volatile double huge = 1e308;
    const double nan = huge * 10.0 - huge * 10.0;      /* inf - inf */
    if (esn_abi_version() != 10) return 1;
    /* esn_gen_reservoirs: null outputs, sizes, sparsity */
    if (esn_gen_reservoirs(33, 4, 2, 0.1, 1, 0, 5, 0, 0, wi, wf, 0) != -1 || !named("esn_gen_reservoirs")) return 2;
    if (!strstr(esn_last_error(), "null")) return 3;
    if (esn_gen_reservoirs(33, 4, 2, 0.1, 1, 0, 5, 0, w, 0, wf, 0) != -1) return 4;
    if (esn_gen_reservoirs(33, 4, 2, 0.1, 1, 0, 5, 0, w, wi, 0, 0) != -1) return 5;
    if (esn_gen_reservoirs(0, 4, 2, 0.1, 1, 0, 5, 0, w, wi, wf, 0) != -1 || !named("esn_gen_reservoirs")) return 6;
    if (esn_gen_reservoirs(-3, 4, 2, 0.1, 1, 0, 5, 0, w, wi, wf, 0) != -1) return 7;
    if (esn_gen_reservoirs(33, 0, 2, 0.1, 1, 0, 5, 0, w, wi, wf, 0) != -1) return 8;
    if (esn_gen_reservoirs(33, 4, 0, 0.1, 1, 0, 5, 0, w, wi, wf, 0) != -1) return 9;
    if (esn_gen_reservoirs(33, 4, 2, 0.1, 1, 0, 0, 0, w, wi, wf, 0) != -1) return 10;
    if (esn_gen_reservoirs(33, 4, 2, 0.1, 1, 0, -1, 0, w, wi, wf, 0) != -1) return 11;
    if (esn_gen_reservoirs(33, 4, 2, -0.01, 1, 0, 5, 0, w, wi, wf, 0) != -1 || !named("esn_gen_reservoirs")) return 12;
    if (!strstr(esn_last_error(), "sparsity")) return 13;
    if (esn_gen_reservoirs(33, 4, 2, 1.01, 1, 0, 5, dp, w, wi, wf, 0) != -1) return 14;
    if (esn_gen_reservoirs(33, 4, 2, nan, 1, 0, 5, 0, w, wi, wf, 0) != -1) return 15;
    if (esn_gen_reservoirs(5000, 4, 2, 0.1, 1, 0, 5, 0, w, wi, wf, 0) != -1 || !strstr(esn_last_error(), "4096")) return 16;
    /* esn_spectral_radius_batch: null pointers, sizes, K outside 4..32, workspace */
    if (esn_spectral_radius_batch(0, 3, 33, 24, rad, st, ws, big, 0) != -1 || !named("esn_spectral_radius_batch")) return 20;
    if (esn_spectral_radius_batch(dp, 3, 33, 24, 0, st, ws, big, 0) != -1) return 21;
    if (esn_spectral_radius_batch(dp, 3, 33, 24, rad, 0, ws, big, 0) != -1) return 22;
    if (esn_spectral_radius_batch(dp, 0, 33, 24, rad, st, ws, big, 0) != -1 || !named("esn_spectral_radius_batch")) return 23;
    if (esn_spectral_radius_batch(dp, -2, 33, 24, rad, st, ws, big, 0) != -1) return 24;
    if (esn_spectral_radius_batch(dp, 3, 0, 24, rad, st, ws, big, 0) != -1) return 25;
    if (esn_spectral_radius_batch(dp, 3, -33, 24, rad, st, ws, big, 0) != -1) return 26;
    if (esn_spectral_radius_batch(dp, 3, 33, 3, rad, st, ws, big, 0) != -1 || !named("esn_spectral_radius_batch")) return 27;
    if (!strstr(esn_last_error(), "n_squarings") || !strstr(esn_last_error(), "32")) return 28;
    if (esn_spectral_radius_batch(dp, 3, 33, 33, rad, st, ws, big, 0) != -1) return 29;
    if (esn_spectral_radius_batch(dp, 3, 33, 0, rad, st, ws, big, 0) != -1) return 30;
    if (esn_spectral_radius_batch(dp, 3, 33, 24, rad, st, 0, big, 0) != -1 || !strstr(esn_last_error(), "workspace")) return 31;
    if (esn_spectral_radius_batch(dp, 3, 33, 24, rad, st, ws, esn_spectral_radius_workspace_bytes(3, 33) - 1, 0) != -1) return 32;
    if (!strstr(esn_last_error(), "workspace")) return 33;
    if (esn_spectral_radius_batch(dp, 3, 33, 24, rad, st, (void*)68, big, 0) != -1) return 34;
    /* esn_scale_reservoirs */
    if (esn_scale_reservoirs(0, 3, 33, 0.9, dp, st, 0) != -1 || !named("esn_scale_reservoirs")) return 40;
    if (esn_scale_reservoirs(w, 3, 33, 0.9, 0, st, 0) != -1) return 41;
    if (esn_scale_reservoirs(w, 3, 33, 0.9, dp, 0, 0) != -1) return 42;
    if (esn_scale_reservoirs(w, 0, 33, 0.9, dp, st, 0) != -1 || !named("esn_scale_reservoirs")) return 43;
    if (esn_scale_reservoirs(w, 3, 0, 0.9, dp, st, 0) != -1) return 44;
    if (esn_scale_reservoirs(w, 3, 33, 0.0, dp, st, 0) != -1 || !strstr(esn_last_error(), "rho")) return 45;
    if (esn_scale_reservoirs(w, 3, 4097, 0.9, dp, st, 0) != -1 || !named("esn_scale_reservoirs")) return 46;
    if (!strstr(esn_last_error(), "4096")) return 47;
    if (esn_spectral_radius_batch(dp, 3, 4097, 24, rad, st, ws, big, 0) != -1 || !strstr(esn_last_error(), "4096")) return 48;
    if (esn_spectral_radius_workspace_bytes(3, 4097) != 0 || !named("esn_spectral_radius_workspace_bytes")) return 49;
    if (!strstr(esn_last_error(), "4096") || esn_spectral_radius_workspace_bytes(3, 4096) == 0) return 57;
    /* the workspace query: positive, monotone in n_sets and in n_res, 0 for no sets; two images of n^2 doubles fit */
    if (esn_spectral_radius_workspace_bytes(1, 1) == 0) return 50;
    if (esn_spectral_radius_workspace_bytes(0, 512) != 0 || esn_spectral_radius_workspace_bytes(-1, 512) != 0) return 51;
    if (esn_spectral_radius_workspace_bytes(4, 0) != 0) return 52;
    for (s = 1; s < 40; ++s)
        for (n = 1; n < 700; n += 7) {
            if (esn_spectral_radius_workspace_bytes(s + 1, n) <= esn_spectral_radius_workspace_bytes(s, n)) return 53;
            if (esn_spectral_radius_workspace_bytes(s, n + 1) < esn_spectral_radius_workspace_bytes(s, n)) return 54;
            if (esn_spectral_radius_workspace_bytes(s, n) < (size_t)s * 2 * n * n * sizeof(double)) return 55;
        }
    for (k = 4; k <= 32; ++k)     /* every served K passes the K check (and stops at the workspace one) */
        if (esn_spectral_radius_batch(dp, 3, 33, k, rad, st, 0, 0, 0) != -1 || !strstr(esn_last_error(), "workspace")) return 56;
    printf("reservoir abi ok\n");
    return 0;
}
'''


def test_reservoir_entry_points_link_from_c99_and_validate_without_a_device(tmp_path):
    r = c_abi.compile_and_run(tmp_path, "res", C_SRC)
    assert "reservoir abi ok" in r.stdout


def test_binding_types_the_reservoir_entry_points():
    from esn_ofdm_mimo_amd import _lib, build
    for name in RES_NAMES:
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 10
    assert len(_lib.SIGNATURES["esn_gen_reservoirs"][1]) == 12
    assert len(_lib.SIGNATURES["esn_spectral_radius_batch"][1]) == 9
    assert len(_lib.SIGNATURES["esn_scale_reservoirs"][1]) == 7
    assert "esn_reservoir.hip" in build.SOURCES


def test_reservoir_checks_through_the_binding():
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    assert lib.esn_abi_version() == 10
    assert lib.esn_gen_reservoirs(33, 4, 2, 0.1, 1, 0, 5, None, None, None, None, None) == -1
    assert b"esn_gen_reservoirs" in lib.esn_last_error()
    assert lib.esn_spectral_radius_batch(None, 1, 16, 24, None, None, None, 0, None) == -1
    assert b"esn_spectral_radius_batch" in lib.esn_last_error()
    assert lib.esn_scale_reservoirs(None, 1, 16, 0.9, None, None, None) == -1
    assert b"esn_scale_reservoirs" in lib.esn_last_error()
    one = lib.esn_spectral_radius_workspace_bytes(1, 512)
    assert one >= 2 * 512 * 512 * 8 and lib.esn_spectral_radius_workspace_bytes(5, 512) == 5 * one
