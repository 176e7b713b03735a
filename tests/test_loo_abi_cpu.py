"""The leave-one-out entry points (esn_readout_ridge_loo_batch[_f32] and their workspace query) are plain C: a C99
program declares them through include/esn_hip.h, links against libesn_hip.so and gets the argument errors (-1) and
the unserved Gram dimension (-2, with the limit in the text) back before anything touches a device.  They are
additions: the ABI version stays 10."""
import c_abi

LOO_NAMES = ("esn_readout_ridge_loo_workspace_bytes", "esn_readout_ridge_loo_batch", "esn_readout_ridge_loo_batch_f32")

C_SRC = r'''
#include <stdio.h>
#include <string.h>
#include "esn_hip.h"
int main(void) {
    /* never dereferenced: the checks run first */
    const double* dp = (const double*)64;
    const float* fp = (const float*)64;
    double* w = (double*)64;
    double* sc = (double*)128;
    int* ch = (int*)64;
    int* st = (int*)128;
    void* ws = (void*)64;
    const size_t big = (size_t)1 << 40;
    int g, l;
    if (esn_abi_version() != 10) return 1;
    /* n_ridge of 0 and of 17 */
    if (esn_readout_ridge_loo_batch(dp, dp, 3, 45, 5, 72, 4, 0, 0, dp, 0, w, sc, ch, st, ws, big, 0) != -1) return 2;
    if (!strstr(esn_last_error(), "esn_readout_ridge_loo_batch") || !strstr(esn_last_error(), "n_ridge")) return 3;
    if (esn_readout_ridge_loo_batch(dp, dp, 3, 45, 5, 72, 4, 0, 0, dp, 17, w, sc, ch, st, ws, big, 0) != -1) return 4;
    if (!strstr(esn_last_error(), "16")) return 5;
    /* n_out of 9 */
    if (esn_readout_ridge_loo_batch(dp, dp, 3, 45, 5, 72, 9, 0, 0, dp, 4, w, sc, ch, st, ws, big, 0) != -1) return 6;
    if (!strstr(esn_last_error(), "n_out")) return 7;
    /* null score, null choice, null ridge, null E */
    if (esn_readout_ridge_loo_batch(dp, dp, 3, 45, 5, 72, 4, 0, 0, dp, 4, w, 0, ch, st, ws, big, 0) != -1) return 8;
    if (!strstr(esn_last_error(), "null")) return 9;
    if (esn_readout_ridge_loo_batch(dp, dp, 3, 45, 5, 72, 4, 0, 0, dp, 4, w, sc, 0, st, ws, big, 0) != -1) return 10;
    if (esn_readout_ridge_loo_batch(dp, dp, 3, 45, 5, 72, 4, 0, 0, 0, 4, w, sc, ch, st, ws, big, 0) != -1) return 11;
    if (esn_readout_ridge_loo_batch(0, dp, 3, 45, 5, 72, 4, 0, 0, dp, 4, w, sc, ch, st, ws, big, 0) != -1) return 12;
    /* workspace too small, and none */
    if (esn_readout_ridge_loo_batch(dp, dp, 3, 45, 5, 72, 4, 0, 0, dp, 4, w, sc, ch, st, ws,
                                    esn_readout_ridge_loo_workspace_bytes(3, 4, 40, 72) - 1, 0) != -1) return 13;
    if (!strstr(esn_last_error(), "workspace")) return 14;
    if (esn_readout_ridge_loo_batch(dp, dp, 3, 45, 5, 72, 4, 0, 0, dp, 4, w, sc, ch, st, 0, big, 0) != -1) return 15;
    /* min(rows, cols) = 129, wide and tall: -2, and the text names the limit */
    if (esn_readout_ridge_loo_batch(dp, dp, 3, 129, 0, 200, 4, 0, 0, dp, 4, w, sc, ch, st, ws, big, 0) != -2) return 16;
    if (!strstr(esn_last_error(), "esn_readout_ridge_loo_batch") || !strstr(esn_last_error(), "128")) return 17;
    if (esn_readout_ridge_loo_batch(dp, dp, 3, 300, 0, 129, 4, 0, 0, dp, 4, w, sc, ch, st, ws, big, 0) != -2) return 18;
    /* float32 E */
    if (esn_readout_ridge_loo_batch_f32(0, dp, 3, 45, 5, 72, 4, 0, 0, dp, 4, w, sc, ch, st, ws, big, 0) != -1) return 19;
    if (!strstr(esn_last_error(), "esn_readout_ridge_loo_batch_f32")) return 20;
    if (esn_readout_ridge_loo_batch_f32(fp, dp, 3, 45, 5, 72, 4, 0, 0, dp, 17, w, sc, ch, st, ws, big, 0) != -1) return 21;
    if (esn_readout_ridge_loo_batch_f32(fp, dp, 3, 45, 5, 72, 9, 0, 0, dp, 4, w, sc, ch, st, ws, big, 0) != -1) return 22;
    if (esn_readout_ridge_loo_batch_f32(fp, dp, 3, 45, 5, 72, 4, 0, 0, dp, 4, w, 0, ch, st, ws, big, 0) != -1) return 23;
    if (esn_readout_ridge_loo_batch_f32(fp, dp, 3, 45, 5, 72, 4, 0, 0, dp, 4, w, sc, ch, st, ws, 8, 0) != -1) return 24;
    if (esn_readout_ridge_loo_batch_f32(fp, dp, 3, 129, 0, 528, 4, 0, 0, dp, 4, w, sc, ch, st, ws, big, 0) != -2) return 25;
    if (!strstr(esn_last_error(), "128")) return 26;
    /* the workspace query: positive, non-decreasing in n_groups and in n_ridge */
    if (esn_readout_ridge_loo_workspace_bytes(1, 1, 128, 528) == 0) return 27;
    for (g = 1; g < 40; ++g)
        for (l = 1; l <= 16; ++l) {
            if (esn_readout_ridge_loo_workspace_bytes(g + 1, l, 128, 528) < esn_readout_ridge_loo_workspace_bytes(g, l, 128, 528))
                return 28;
            if (l < 16 && esn_readout_ridge_loo_workspace_bytes(g, l + 1, 200, 104) < esn_readout_ridge_loo_workspace_bytes(g, l, 200, 104))
                return 29;
        }
    if (esn_readout_ridge_loo_workspace_bytes(0, 4, 128, 528) != 0) return 30;
    printf("loo abi ok\n");
    return 0;
}
'''


def test_loo_entry_points_link_from_c99_and_validate_without_a_device(tmp_path):
    r = c_abi.compile_and_run(tmp_path, "loo", C_SRC)
    assert "loo abi ok" in r.stdout


def test_binding_types_the_loo_entry_points():
    from esn_ofdm_mimo_amd import _lib
    for name in LOO_NAMES:
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 10
    sig = _lib.SIGNATURES
    # the ridge Cholesky siblings plus (score, choice); the query has their four arguments
    assert len(sig["esn_readout_ridge_loo_batch"][1]) == len(sig["esn_readout_solve_chol_ridge_batch"][1]) + 2
    assert len(sig["esn_readout_ridge_loo_batch_f32"][1]) == len(sig["esn_readout_solve_chol_ridge_batch_f32"][1]) + 2
    assert len(sig["esn_readout_ridge_loo_workspace_bytes"][1]) == 4


def test_loo_checks_through_the_binding():
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    assert lib.esn_abi_version() == 10
    rc = lib.esn_readout_ridge_loo_batch(None, None, 1, 10, 0, 4, 1, None, None, None, 1, None, None, None, None,
                                         None, 0, None)
    assert rc == -1 and b"esn_readout_ridge_loo_batch" in lib.esn_last_error()
    one = lib.esn_readout_ridge_loo_workspace_bytes(1, 1, 128, 528)
    assert one > 0 and lib.esn_readout_ridge_loo_workspace_bytes(5, 8, 128, 528) >= 5 * one
