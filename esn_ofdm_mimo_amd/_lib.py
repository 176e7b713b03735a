"""ctypes binding of libesn_hip.so (include/esn_hip.h).  Fails loudly: a missing
library or a missing GPU is an error, never a silent CPU path."""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ESN_HIP_LIB") or os.path.join(_PKG, "libesn_hip.so")   # env: tuning builds only

F64, F32, F16, BF16 = 0, 1, 2, 3
PRECISIONS = {"f64": F64, "f32": F32, "f16": F16, "bf16": BF16}
NOISE_NONE, NOISE_TENSOR, NOISE_COUNTER = 0, 1, 2
ABI_VERSION = 10
MEM_DEVICE, MEM_HOST = 0, 1
# enum esn_path, by value: the recurrence kernel a call dispatches to (recur_path below)
PATHS = ("mfma", "skew16", "f64_valu", "f64_mfma", "cluster_f64", "big_predict", "big_harvest", "harvest_cluster")


class Shape(C.Structure):
    _fields_ = [("n_res", C.c_int), ("n_in", C.c_int), ("n_out", C.c_int),
                ("teacher_forcing", C.c_int), ("n_wsets", C.c_int),
                ("leak_rate", C.c_double)]       # extension: 0 or 1 = the reference's update (include/esn_hip.h)


class EsnHipError(RuntimeError):
    pass


_vp, _dp, _ip = C.c_void_p, C.c_void_p, C.c_void_p   # device pointers travel as integers
SIGNATURES = {
    "esn_last_error": (C.c_char_p, []),
    "esn_abi_version": (C.c_int, []),
    "esn_debug_set": (C.c_int, [C.c_char_p, C.c_char_p]),
    "esn_recur_path": (C.c_int, [C.c_int, C.c_int, C.POINTER(Shape), C.c_int, C.c_int, C.c_int]),
    "esn_device_info": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                  C.c_char_p, C.c_int]),
    "esn_tile_frames": (C.c_int, [C.c_int, C.POINTER(Shape)]),
    "esn_packed_weights_bytes": (C.c_size_t, [C.c_int, C.POINTER(Shape)]),
    "esn_packed_readout_bytes": (C.c_size_t, [C.c_int, C.POINTER(Shape)]),
    "esn_pack_weights": (C.c_int, [C.c_int, C.POINTER(Shape), _dp, _dp, _dp, _vp, _vp]),
    "esn_pack_readout": (C.c_int, [C.c_int, C.POINTER(Shape), C.c_int, _dp, _vp, _vp]),
    "esn_predict_batch": (C.c_int, [C.c_int, C.POINTER(Shape), _vp, _vp, _dp, _dp, _dp, _dp, _dp,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp,
                                    C.c_double, C.c_int, _dp, C.c_uint64, C.c_uint64, _dp, _vp, C.c_size_t, _vp]),
    "esn_predict_batch_f32": (C.c_int, [C.c_int, C.POINTER(Shape), _vp, _vp, _dp, _dp, _dp, _dp, _vp,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp,
                                        C.c_double, C.c_int, _dp, C.c_uint64, C.c_uint64, _vp, _vp, C.c_size_t, _vp]),
    "esn_predict_workspace_bytes": (C.c_size_t, [C.c_int, C.POINTER(Shape), C.c_int, C.c_int]),
    "esn_harvest_batch": (C.c_int, [C.c_int, C.POINTER(Shape), _vp, _dp, _dp, _dp, _dp, _dp, _dp,
                                    C.c_int, C.c_int, C.c_double, C.c_int, _dp, C.c_uint64, C.c_uint64, _dp,
                                    _vp, C.c_size_t, _vp]),
    "esn_harvest_workspace_bytes": (C.c_size_t, [C.c_int, C.POINTER(Shape), C.c_int]),
    "esn_harvest_batch_f32": (C.c_int, [C.c_int, C.POINTER(Shape), _vp, _dp, _dp, _dp, _dp, _dp, _dp,
                                        C.c_int, C.c_int, C.c_double, C.c_int, _dp, C.c_uint64, C.c_uint64, _vp,
                                        _vp, C.c_size_t, _vp]),
    "esn_readout_solve_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "esn_readout_solve_batch": (C.c_int, [_dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          _dp, _dp, _dp, _ip, _vp, _vp]),
    "esn_readout_chol_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "esn_readout_solve_chol_batch": (C.c_int, [_dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                               _dp, _dp, _dp, _ip, _vp, C.c_size_t, _vp]),
    "esn_readout_solve_chol_batch_f32": (C.c_int, [_vp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   _dp, _dp, _dp, _ip, _vp, C.c_size_t, _vp]),
    # ridge read-out (extension): lambda [G][L] between t_shift and W_out; W_out [G][L][n_out][cols], status [G][L]
    "esn_readout_solve_ridge_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "esn_readout_solve_ridge_batch": (C.c_int, [_dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                _dp, _dp, _dp, C.c_int, _dp, _ip, _vp, _vp]),
    "esn_readout_chol_ridge_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "esn_readout_solve_chol_ridge_batch": (C.c_int, [_dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                     _dp, _dp, _dp, C.c_int, _dp, _ip, _vp, C.c_size_t, _vp]),
    "esn_readout_solve_chol_ridge_batch_f32": (C.c_int, [_vp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                         _dp, _dp, _dp, C.c_int, _dp, _ip, _vp, C.c_size_t, _vp]),
    # leave-one-out choice among L candidates: W_out [G][n_out][cols], score [G][L], choice [G], status [G][L]
    "esn_readout_ridge_loo_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "esn_readout_ridge_loo_batch": (C.c_int, [_dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              _dp, _dp, _dp, C.c_int, _dp, _dp, _ip, _ip, _vp, C.c_size_t, _vp]),
    "esn_readout_ridge_loo_batch_f32": (C.c_int, [_vp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  _dp, _dp, _dp, C.c_int, _dp, _dp, _ip, _ip, _vp, C.c_size_t, _vp]),
    # hold-out score of the candidates W [G][L][n_out][cols] on a pilot the fit has not seen: E, D, W, n_groups, T,
    # transient, cols, n_out, t_scale, t_shift, n_ridge, status_in, score [G][L], choice [G], stream
    "esn_readout_holdout_score": (C.c_int, [_dp, _dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            _dp, _dp, C.c_int, _ip, _dp, _ip, _vp]),
    "esn_readout_holdout_score_f32": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                _dp, _dp, C.c_int, _ip, _dp, _ip, _vp]),
    # running normal equations: E, D, n_groups, T, transient, cols, n_out, t_scale, t_shift, decay, Gm [G][cols][cols],
    # Cm [G][n_out][cols], stream; and Gm, Cm, n_groups, cols, n_out, ridge [G][L], n_ridge, W_out [G][L][n_out][cols],
    # status [G][L], workspace, workspace_bytes, stream
    "esn_gram_accumulate": (C.c_int, [_dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_double,
                                      _dp, _dp, _vp]),
    "esn_gram_accumulate_f32": (C.c_int, [_vp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_double,
                                          _dp, _dp, _vp]),
    "esn_gram_solve_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "esn_gram_solve": (C.c_int, [_dp, _dp, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp, _ip, _vp, C.c_size_t, _vp]),
    # reservoirs drawn on the device: W [S][n][n], W_in [S][n][n_in], W_fb [S][n][n_out], radius [S], status [S]
    "esn_gen_reservoirs": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_uint64, C.c_uint64, C.c_int,
                                     _dp, _dp, _dp, _dp, _vp]),
    "esn_spectral_radius_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "esn_spectral_radius_batch": (C.c_int, [_dp, C.c_int, C.c_int, C.c_int, _dp, _ip, _vp, C.c_size_t, _vp]),
    "esn_spectral_radius_split_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "esn_spectral_radius_split_batch": (C.c_int, [_dp, C.c_int, C.c_int, C.c_int, _dp, _ip, _vp, C.c_size_t, _vp]),
    "esn_scale_reservoirs": (C.c_int, [_dp, C.c_int, C.c_int, C.c_double, _dp, _ip, _vp]),
    "esn_gen_taps": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _dp,
                               C.c_uint64, C.c_uint64, _dp, _vp]),
    # Jakes taps inside a coherence block: taps [n_blocks][n_sym][n_r][n_t][isi]; angles_in [links][paths][16][2]
    "esn_gen_taps_doppler": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                       C.c_double, _dp, C.c_uint64, C.c_uint64, _dp, _vp]),
    "esn_gen_frames": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 _dp, _dp, C.c_double, _dp, _vp, _dp, C.c_uint64, C.c_uint64, _vp, _dp, _dp, _vp]),
    "esn_gen_frames_c64": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, _dp, _dp, C.c_double, _dp, _vp, _dp, C.c_uint64, C.c_uint64, _vp, _vp, _vp,
                                     _vp]),
    "esn_channel_estimate": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp,
                                       C.c_double, _vp, _dp, C.c_int, _dp, _vp]),
    "esn_mmse_detect_count": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp,
                                        C.c_double, _dp, _dp, _vp, _vp, _vp, _dp, _vp]),
    "esn_zf_detect_count": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp,
                                      _dp, _dp, _vp, _vp, _vp, _dp, _vp]),
    # equalised time-domain rows: n_frames, frames_per_group, N, cp, pad, n_t, n_r, p_i, no, H, y_cp, U_eq, X_hat, stream
    "esn_mmse_equalize_rows": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp,
                                         C.c_double, _dp, _dp, _dp, _dp, _vp]),
    "esn_mmse_equalize_rows_f32": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp,
                                             C.c_double, _dp, _dp, _vp, _dp, _vp]),
    "esn_taps_to_freq": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _vp]),
    "esn_channel_metrics": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_double, _dp, _dp, _vp, _dp, _vp]),
    # decision-directed channel estimate: y_cp, X_hat | bits, n_est, window, est_per_group, N, cp, n_t, n_r, isi, m, p_i,
    # reg, taps, H, status, stream
    "esn_channel_track": (C.c_int, [_dp, _dp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _vp]),
    # windowed ELM: precision, n_in, n_hidden, window, bias_col, n_wsets, W_in, b, in_scale, in_shift, U, n_groups, T_in,
    # T, group_offset, E, e_f32, e_cols, stream
    "esn_elm_features": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp,
                                   C.c_int, C.c_int, C.c_int, C.c_uint64, _vp, C.c_int, C.c_int, _vp]),
    # precision, n_in, n_hidden, window, bias_col, n_wsets, n_out, W_in, b, W_out, e_cols, in_scale, in_shift, t_scale,
    # t_shift, U, n_frames, frames_per_group, T_in, T, transient, group_offset, Y, stream
    "esn_elm_predict": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int,
                                  _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, _dp,
                                  _vp]),
    # windowed FNN: n_in, n_hidden, window, n_out, n_groups, T -> bytes of esn_fnn_train's workspace
    "esn_fnn_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    # precision, n_in, n_hidden, window, n_out, n_isets, W1_0, b1_0, W2_0, b2_0, in_scale, in_shift, t_scale, t_shift, U,
    # D, n_groups, T_in, T, transient, group_offset, epochs, lr, beta1, beta2, eps, W1, b1, W2, b2, loss, workspace,
    # workspace_bytes, stream
    "esn_fnn_train": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                _dp, _dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_double,
                                C.c_double, C.c_double, C.c_double, _dp, _dp, _dp, _dp, _dp, _vp, C.c_size_t, _vp]),
    # precision, n_in, n_hidden, window, n_out, W1, b1, W2, b2, in_scale, in_shift, t_scale, t_shift, U, n_frames,
    # frames_per_group, T_in, T, transient, Y, stream
    "esn_fnn_predict": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                  _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _vp]),
    # windowed CNN: n_in, c1, c2, n_out, kernel, n_groups, n_frames, T -> bytes of the workspace of train / predict
    "esn_cnn_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    # precision, n_in, c1, c2, n_out, kernel, n_isets, W1_0, b1_0, W2_0, b2_0, W3_0, b3_0, in_scale, in_shift, t_scale,
    # t_shift, U, D, n_groups, T_in, T, transient, group_offset, epochs, lr, beta1, beta2, eps, W1, b1, W2, b2, W3, b3,
    # loss, workspace, workspace_bytes, stream
    "esn_cnn_train": (C.c_int, [C.c_int] * 7 + [_dp] * 12 + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int,
                                C.c_double, C.c_double, C.c_double, C.c_double] + [_dp] * 7 + [_vp, C.c_size_t, _vp]),
    # precision, n_in, c1, c2, n_out, kernel, W1, b1, W2, b2, W3, b3, in_scale, in_shift, t_scale, t_shift, U, n_frames,
    # frames_per_group, T_in, T, transient, Y, workspace, workspace_bytes, stream
    "esn_cnn_predict": (C.c_int, [C.c_int] * 6 + [_dp] * 11 + [C.c_int] * 5 + [_dp, _vp, C.c_size_t, _vp]),
    # LSTM comparator: n_in, n_hidden, n_out, n_groups, n_frames, T -> bytes of the workspace of train / predict
    "esn_lstm_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    # precision, n_in, n_hidden, n_out, n_isets, W_ih_0, W_hh_0, b_ih_0, b_hh_0, W_fc_0, b_fc_0, in_scale, in_shift,
    # t_scale, t_shift, U, D, n_groups, T_in, T, transient, group_offset, epochs, lr, beta1, beta2, eps, W_ih, W_hh, b_ih,
    # b_hh, W_fc, b_fc, loss, workspace, workspace_bytes, stream
    "esn_lstm_train": (C.c_int, [C.c_int] * 5 + [_dp] * 12 + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int,
                                 C.c_double, C.c_double, C.c_double, C.c_double] + [_dp] * 7 + [_vp, C.c_size_t, _vp]),
    # precision, n_in, n_hidden, n_out, W_ih, W_hh, b_ih, b_hh, W_fc, b_fc, in_scale, in_shift, t_scale, t_shift, U,
    # n_frames, frames_per_group, T_in, T, transient, Y, workspace, workspace_bytes, stream
    "esn_lstm_predict": (C.c_int, [C.c_int] * 4 + [_dp] * 11 + [C.c_int] * 5 + [_dp, _vp, C.c_size_t, _vp]),
    "esn_ldpc_encode": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "esn_qam_llr": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _vp]),
    "esn_ldpc_decode_count": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _ip, _ip, _dp,
                                        C.c_double, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp]),
    "esn_detect_count": (C.c_int, [_dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _vp,
                                   _vp, _vp, _dp, _vp]),
    "esn_detect_count_f32": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _vp,
                                       _vp, _vp, _dp, _vp]),
    # ensemble tail: Y [K, B, N, 2 n_t], K, B, F, N, n_t, m, p_i, weights, tx_bits, err, bits, member_err, X_hat, stream
    "esn_detect_count_ens": (C.c_int, [_dp] + [C.c_int] * 6 + [_dp, _dp, _vp, _vp, _vp, _vp, _dp, _vp]),
    "esn_detect_count_ens_f32": (C.c_int, [_vp] + [C.c_int] * 6 + [_dp, _dp, _vp, _vp, _vp, _vp, _dp, _vp]),
    # decide and re-modulate: Y, B, F, N, cp, delay, n_t, m, p_i, tx_bits, err, bits, X_hat, dec_bits, D_hat, stream
    "esn_detect_remod": (C.c_int, [_dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _vp,
                                   _vp, _vp, _dp, _vp, _dp, _vp]),
}
# host-memory front ends: the arguments of esn_X behind a leading esn_mem_kind (include/esn_hip.h)
for _name in ("esn_pack_weights", "esn_pack_readout", "esn_predict_batch", "esn_harvest_batch",
              "esn_readout_solve_batch", "esn_detect_count"):
    SIGNATURES[_name + "_mem"] = (C.c_int, [C.c_int] + SIGNATURES[_name][1])
SIGNATURES["esn_device_alloc"] = (C.c_void_p, [C.c_size_t])
SIGNATURES["esn_device_free"] = (C.c_int, [C.c_void_p])

_lib = None


def load():
    """Load (once) and type the library.  Raises EsnHipError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EsnHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the ESN hot path.")
    # torch first: libesn_hip.so must resolve libamdhip64 to the copy torch has already loaded -- loaded before torch it
    # binds the system ROCm runtime instead, the process ends up with two HIP runtimes and every launch of this
    # library fails with hipErrorNoDevice (seen with build() + smoke() in one process)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype, fn.argtypes = res, args
    if lib.esn_abi_version() != ABI_VERSION:
        raise EsnHipError(f"libesn_hip.so ABI {lib.esn_abi_version()} != binding {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().esn_last_error().decode(errors="replace")
        raise EsnHipError(f"{what} failed ({rc}): {msg}")


def ptr(t):
    """data_ptr of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise EsnHipError("no HIP device visible: the ESN hot path runs on the GPU only "
                          "(no CPU fallback is provided)")
    return torch


def stream_handle():
    import torch
    return torch.cuda.current_stream().cuda_stream


def debug_set(key, value):
    """Tuning knob of the library (benchmarks / A-B tests): see esn_debug_set in include/esn_hip.h."""
    check(load().esn_debug_set(key.encode(), None if value is None else str(value).encode()), "esn_debug_set")


def recur_path(harvest, precision, shape, n_sequences, frames_per_group=1, have_workspace=True):
    """Name (PATHS) of the kernel esn_harvest_batch (harvest) / esn_predict_batch runs for this call under the current
    knobs: esn_recur_path in include/esn_hip.h.  `precision` is a key of PRECISIONS."""
    rc = load().esn_recur_path(int(bool(harvest)), PRECISIONS[precision], C.byref(shape), int(n_sequences),
                               int(frames_per_group), int(bool(have_workspace)))
    if rc < 0:
        check(rc, "esn_recur_path")
    return PATHS[rc]


def device_info():
    lib = load()
    cu, lds, clk = C.c_int(), C.c_int(), C.c_int()
    name = C.create_string_buffer(64)
    check(lib.esn_device_info(C.byref(cu), C.byref(lds), C.byref(clk), name, 64), "esn_device_info")
    return dict(cu_count=cu.value, lds_bytes_per_cu=lds.value, clock_khz=clk.value,
                arch=name.value.decode())
