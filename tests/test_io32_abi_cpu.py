"""The float32 / complex64 I/O entry points (esn_predict_batch_f32, esn_detect_count_f32, esn_gen_frames_c64) are
plain C: a C99 program declares them by use through include/esn_hip.h, links against libesn_hip.so and gets the
argument errors (-1) and the unserved precision (-2) back before anything touches a device."""
import c_abi

C_SRC = r'''
#include <stdio.h>
#include <string.h>
#include "esn_hip.h"
int main(void) {
    esn_shape_t sh = {512, 16, 8, 1, 1};
    const void* pw = (const void*)16;                /* never dereferenced: the checks run first */
    float* y32 = (float*)64;
    if (esn_abi_version() != 10) return 1;
    /* null U, then null Y */
    if (esn_predict_batch_f32(ESN_F16, &sh, pw, pw, 0, 0, 0, 0, 0, 4, 4, 10, 10, 2, 0, 0, 0.0, 0, 0, 0, 0, y32, 0, 0, 0)
        != -1) return 2;
    if (!strstr(esn_last_error(), "esn_predict_batch_f32") || !strstr(esn_last_error(), "null")) return 3;
    if (esn_predict_batch_f32(ESN_F16, &sh, pw, pw, 0, 0, 0, 0, (const float*)64, 4, 4, 10, 10, 2, 0, 0, 0.0, 0, 0, 0, 0,
                              0, 0, 0, 0) != -1) return 4;
    if (esn_last_error()[0] == 0) return 5;
    /* misaligned Y, bad sizes */
    if (esn_predict_batch_f32(ESN_F32, &sh, pw, pw, 0, 0, 0, 0, (const float*)64, 4, 4, 10, 10, 2, 0, 0, 0.0, 0, 0, 0, 0,
                              (float*)68, 0, 0, 0) != -1) return 6;
    if (!strstr(esn_last_error(), "aligned")) return 7;
    if (esn_predict_batch_f32(ESN_F32, &sh, pw, pw, 0, 0, 0, 0, (const float*)64, 4, 4, 10, 10, 10, 0, 0, 0.0, 0, 0, 0,
                              0, y32, 0, 0, 0) != -1) return 8;
    /* float64 precision: not served with float32 I/O */
    if (esn_predict_batch_f32(ESN_F64, &sh, pw, pw, 0, 0, 0, 0, (const float*)64, 4, 4, 10, 10, 2, 0, 0, 0.0, 0, 0, 0, 0,
                              y32, 0, 0, 0) != -2) return 9;
    if (!strstr(esn_last_error(), "ESN_F64")) return 10;
    /* detector: null Y */
    if (esn_detect_count_f32(0, 1, 1, 128, 4, 4, (const double*)8, (const uint8_t*)8, (long long*)8, (long long*)8, 0, 0)
        != -1) return 11;
    if (!strstr(esn_last_error(), "esn_detect_count_f32")) return 12;
    /* generator: null y_cp, then N not a power of two */
    if (esn_gen_frames_c64(1, 1, 128, 9, 4, 8, 8, 4, 0, (const double*)8, (const double*)8, 1e-5, (const double*)8,
                           0, 0, 0, 0, (uint8_t*)8, 0, 0, 0) != -1) return 13;
    if (!strstr(esn_last_error(), "esn_gen_frames_c64")) return 14;
    if (esn_gen_frames_c64(1, 1, 100, 7, 4, 8, 8, 4, 0, (const double*)8, (const double*)8, 1e-5, (const double*)8,
                           0, 0, 0, 0, (uint8_t*)8, 0, (float*)8, 0) != -1) return 15;
    printf("io32 abi ok\n");
    return 0;
}
'''


def test_io32_entry_points_link_from_c99_and_validate_without_a_device(tmp_path):
    r = c_abi.compile_and_run(tmp_path, "io32", C_SRC)
    assert "io32 abi ok" in r.stdout


def test_binding_types_the_io32_entry_points():
    from esn_ofdm_mimo_amd import _lib
    for name in ("esn_predict_batch_f32", "esn_detect_count_f32", "esn_gen_frames_c64"):
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 10
    # same arity as the float64 siblings: only the array types differ
    assert len(_lib.SIGNATURES["esn_predict_batch_f32"][1]) == len(_lib.SIGNATURES["esn_predict_batch"][1])
    assert len(_lib.SIGNATURES["esn_detect_count_f32"][1]) == len(_lib.SIGNATURES["esn_detect_count"][1])
    assert len(_lib.SIGNATURES["esn_gen_frames_c64"][1]) == len(_lib.SIGNATURES["esn_gen_frames"][1])
