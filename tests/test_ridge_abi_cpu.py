"""The ridge read-out entry points (esn_readout_solve_ridge_batch, esn_readout_solve_chol_ridge_batch[_f32] and their
workspace queries) are plain C: a C99 program declares them by use through include/esn_hip.h, links against
libesn_hip.so and gets the argument errors (-1) and the unserved Cholesky shapes (-2) back before anything touches a
device.  They are additions: the ABI version stays 10."""
import c_abi

RIDGE_NAMES = ("esn_readout_solve_ridge_workspace_bytes", "esn_readout_solve_ridge_batch",
               "esn_readout_chol_ridge_workspace_bytes", "esn_readout_solve_chol_ridge_batch",
               "esn_readout_solve_chol_ridge_batch_f32")

C_SRC = r'''
#include <stdio.h>
#include <string.h>
#include "esn_hip.h"
int main(void) {
    /* never dereferenced: the checks run first */
    const double* dp = (const double*)64;
    const float* fp = (const float*)64;
    double* w = (double*)64;
    int* st = (int*)64;
    void* ws = (void*)64;
    if (esn_abi_version() != 10) return 1;
    /* QR: null ridge, null E, n_ridge = 0 */
    if (esn_readout_solve_ridge_batch(dp, dp, 3, 45, 5, 72, 4, 0, 0, 0, 1, w, st, ws, 0) != -1) return 2;
    if (!strstr(esn_last_error(), "esn_readout_solve_ridge_batch") || !strstr(esn_last_error(), "null")) return 3;
    if (esn_readout_solve_ridge_batch(0, dp, 3, 45, 5, 72, 4, 0, 0, dp, 1, w, st, ws, 0) != -1) return 4;
    if (esn_readout_solve_ridge_batch(dp, dp, 3, 45, 5, 72, 4, 0, 0, dp, 0, w, st, ws, 0) != -1) return 5;
    if (!strstr(esn_last_error(), "esn_readout_solve_ridge_batch")) return 6;
    /* Cholesky, float64 E: null ridge, null status, n_ridge = 0, Gram dimension 513, n_out = 9 */
    if (esn_readout_solve_chol_ridge_batch(dp, dp, 3, 45, 5, 72, 4, 0, 0, 0, 1, w, st, 0, 0, 0) != -1) return 7;
    if (!strstr(esn_last_error(), "esn_readout_solve_chol_ridge_batch") || !strstr(esn_last_error(), "null")) return 8;
    if (esn_readout_solve_chol_ridge_batch(dp, dp, 3, 45, 5, 72, 4, 0, 0, dp, 1, w, 0, 0, 0, 0) != -1) return 9;
    if (esn_readout_solve_chol_ridge_batch(dp, dp, 3, 45, 5, 72, 4, 0, 0, dp, 0, w, st, 0, 0, 0) != -1) return 10;
    if (esn_readout_solve_chol_ridge_batch(dp, dp, 3, 513, 0, 600, 4, 0, 0, dp, 2, w, st, ws, (size_t)1 << 40, 0) != -2)
        return 11;
    if (!strstr(esn_last_error(), "esn_readout_solve_chol_ridge_batch")) return 12;
    if (esn_readout_solve_chol_ridge_batch(dp, dp, 3, 45, 5, 72, 9, 0, 0, dp, 2, w, st, 0, 0, 0) != -2) return 13;
    /* ... workspace too small for a Gram dimension beyond 128 */
    if (esn_readout_solve_chol_ridge_batch(dp, dp, 3, 130, 0, 131, 4, 0, 0, dp, 2, w, st, ws,
                                           esn_readout_chol_ridge_workspace_bytes(3, 2, 130, 131) - 1, 0) != -1) return 14;
    if (!strstr(esn_last_error(), "workspace")) return 15;
    /* Cholesky, float32 E */
    if (esn_readout_solve_chol_ridge_batch_f32(0, dp, 3, 45, 5, 72, 4, 0, 0, dp, 1, w, st, 0, 0, 0) != -1) return 16;
    if (!strstr(esn_last_error(), "esn_readout_solve_chol_ridge_batch_f32")) return 17;
    if (esn_readout_solve_chol_ridge_batch_f32(fp, dp, 3, 45, 5, 72, 4, 0, 0, dp, 0, w, st, 0, 0, 0) != -1) return 18;
    if (esn_readout_solve_chol_ridge_batch_f32(fp, dp, 3, 600, 0, 513, 4, 0, 0, dp, 1, w, st, ws, (size_t)1 << 40, 0)
        != -2) return 19;
    if (!strstr(esn_last_error(), "esn_readout_solve_chol_ridge_batch_f32")) return 20;
    /* workspace queries */
    if (esn_readout_solve_ridge_workspace_bytes(3, 1, 128, 528, 8) < esn_readout_solve_workspace_bytes(3, 128, 528, 8))
        return 21;
    if (esn_readout_solve_ridge_workspace_bytes(3, 2, 128, 528, 8)
        != 2 * esn_readout_solve_ridge_workspace_bytes(3, 1, 128, 528, 8)) return 22;
    if (esn_readout_solve_ridge_workspace_bytes(3, 0, 128, 528, 8) != 0) return 23;
    if (esn_readout_chol_ridge_workspace_bytes(3, 4, 40, 72) != 0) return 24;              /* LDS kernel */
    if (esn_readout_chol_ridge_workspace_bytes(3, 4, 130, 131)
        != 4 * esn_readout_chol_workspace_bytes(3, 130, 131)) return 25;
    printf("ridge abi ok\n");
    return 0;
}
'''


def test_ridge_entry_points_link_from_c99_and_validate_without_a_device(tmp_path):
    r = c_abi.compile_and_run(tmp_path, "ridge", C_SRC)
    assert "ridge abi ok" in r.stdout


def test_binding_types_the_ridge_entry_points():
    from esn_ofdm_mimo_amd import _lib
    for name in RIDGE_NAMES:
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 10
    sig = _lib.SIGNATURES
    # the pinv siblings plus (ridge, n_ridge); the queries plus n_ridge
    assert len(sig["esn_readout_solve_ridge_batch"][1]) == len(sig["esn_readout_solve_batch"][1]) + 2
    assert len(sig["esn_readout_solve_chol_ridge_batch"][1]) == len(sig["esn_readout_solve_chol_batch"][1]) + 2
    assert len(sig["esn_readout_solve_chol_ridge_batch_f32"][1]) == len(sig["esn_readout_solve_chol_batch_f32"][1]) + 2
    assert len(sig["esn_readout_solve_ridge_workspace_bytes"][1]) == len(sig["esn_readout_solve_workspace_bytes"][1]) + 1
    assert len(sig["esn_readout_chol_ridge_workspace_bytes"][1]) == len(sig["esn_readout_chol_workspace_bytes"][1]) + 1


def test_ridge_workspace_queries_through_the_binding():
    """The QR ridge solve factorises the augmented matrix (rows + cols matrix rows per entry): its workspace is never
    smaller than the pinv one and is proportional to n_ridge, wide and tall."""
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    assert lib.esn_abi_version() == 10
    for rows, cols, n_out in ((128, 528, 8), (512, 104, 4), (20, 36, 4), (50, 12, 4)):
        pinv = lib.esn_readout_solve_workspace_bytes(3, rows, cols, n_out)
        one = lib.esn_readout_solve_ridge_workspace_bytes(3, 1, rows, cols, n_out)
        assert one >= pinv > 0
        n = min(rows, cols)
        extra = n_out if rows >= cols else 0
        assert one == 3 * 8 * ((n + extra) * (rows + cols) + n_out * (rows + cols) + 2 * n)
        for nl in (2, 5):
            assert lib.esn_readout_solve_ridge_workspace_bytes(3, nl, rows, cols, n_out) == nl * one
    # null pointers / n_ridge = 0 through ctypes, too: rejected before any device call, the text names the function
    rc = lib.esn_readout_solve_ridge_batch(None, None, 1, 10, 0, 4, 1, None, None, None, 1, None, None, None, None)
    assert rc == -1 and b"esn_readout_solve_ridge_batch" in lib.esn_last_error()
