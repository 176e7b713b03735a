// Host-side functions one translation unit of the library offers the others: geometry, size and "applies"
// predicates and the kernel launchers, grouped by the file that defines them.  Included by the callers
// (esn_api.hip, esn_host.hip) AND by every defining file, so a definition is compiled against the declaration its
// caller sees; default arguments live here only.  Launchers return 0, a hipError_t (> 0), or -1 for "no kernel
// instance for this shape".
#pragma once
#include <atomic>
#include "esn_common.h"

namespace esn {
// Raises the dynamic-LDS ceiling of `kernel` to `bytes` (the most any shape may ask for) once per device: `raised`, a
// static of the calling launcher, holds one bit per device.  For launchers that run per symbol of a tracking loop.
inline int raise_dynamic_lds_once(const void* kernel, size_t bytes, std::atomic<unsigned long long>& raised) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    const unsigned long long bit = 1ULL << (dev & 63);
    if (!(raised.load(std::memory_order_relaxed) & bit)) {
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return (int)e;
        raised.fetch_or(bit, std::memory_order_relaxed);
    }
    return 0;
}
// esn_api.hip: sets esn_last_error(), returns `code`
int api_fail(int code, const char* fmt, ...);
#ifdef ESN_STAMPS
unsigned long long* stamp_buffer();
#endif
// esn_recur_f64.hip
int launch_recur_f64(const RecurParams& p, hipStream_t stream);
size_t recur_f64_lds_bytes(int FB, int n_res, int n_in, int n_out);
// esn_recur_f64_mfma.hip
bool f64_mfma_geometry(int n_res, int n_in, int n_out, bool harvest, Geometry* g);
int launch_recur_f64_mfma(const RecurParams& p, hipStream_t stream);
// esn_big_predict.hip (the read-out image at p.wo16_off of a group's packed read-out)
bool big_path_applies(int precision, const RecurParams& p);
int big_slots(const RecurParams& p);
size_t big_workspace_bytes(int n_slots, int Mp, int Kp);
size_t big_wout_image_bytes(int Mp);
int launch_recur_big(int precision, const RecurParams& p, void* workspace, hipStream_t stream, bool io32 = false);
// esn_big_harvest.hip
bool big_harvest_applies(int precision, const RecurParams& p);
size_t big_harvest_workspace_bytes(int n_groups, int Kp);
int launch_harvest_big(int precision, const RecurParams& p, void* workspace, hipStream_t stream);
// esn_recur_cluster.hip
bool cluster_applies(int precision, const RecurParams& p);
size_t cluster_workspace_bytes(int n_res, int n_in, int n_out, bool harvest);
int launch_recur_cluster(const RecurParams& p, void* workspace, hipStream_t stream);
// esn_recur_mfma.hip, and the per-precision instantiations it dispatches to (esn_recur_mfma_{f32,f16,bf16}.hip)
bool mfma_geometry(int precision, int n_res, int n_in, int n_out, bool harvest, Geometry* g);
int launch_recur_mfma(int precision, const RecurParams& p, hipStream_t stream, bool io32 = false);
int launch_recur_mfma_f32(const RecurParams& p, hipStream_t stream, bool io32);
int launch_recur_mfma_f16(const RecurParams& p, hipStream_t stream, bool io32);
int launch_recur_mfma_bf16(const RecurParams& p, hipStream_t stream, bool io32);
// esn_harvest_cluster.hip
bool harvest_cluster_applies(int precision, const RecurParams& p);
size_t harvest_cluster_workspace_bytes(int n_pilots, int n_wsets);
int launch_harvest_cluster(int precision, const RecurParams& p, void* workspace, hipStream_t stream);
// esn_recur_skew16.hip
int launch_recur_skew16(int precision, const RecurParams& p, hipStream_t stream, bool io32 = false);
// esn_pack.hip
size_t packed_w_bytes(int precision, int n_res, int n_in, int n_out, const Geometry& g);
size_t packed_wout_bytes(int precision, int n_res, int n_in, int n_out, const Geometry& g);
size_t wout_big_offset(int precision, int n_out, const Geometry& g);
size_t f64_w_offset(int n_res, int n_in, int n_out);
size_t f64_wout_offset(int n_res, int n_in, int n_out);
int launch_pack_weights(int precision, const esn_shape_t* sh, const Geometry& g, const double* W,
                        const double* Win, const double* Wfb, void* packed, hipStream_t stream);
int launch_pack_readout(int precision, const esn_shape_t* sh, const Geometry& g, int n_groups,
                        const double* Wout, void* packed, hipStream_t stream);
// The arguments of one read-out entry point, from the ABI to the launch; what an entry point does not take stays
// nullptr (and n_ridge 1).  ridge != nullptr (device, [n_groups][n_ridge]): the ridge instances, one workgroup per
// (group, lambda); W_out, status and the workspace then hold n_groups * n_ridge entries.
struct ReadoutArgs {
    const double* E; const float* E32; const double* D;
    int n_groups, T, transient, cols, n_out;
    const double *t_scale, *t_shift, *ridge; int n_ridge;
    double *W_out, *score; int *choice, *status;
    void* workspace; size_t workspace_bytes; hipStream_t stream;
};
// esn_solve_qr.hip, esn_solve_chol.hip, esn_solve_chol_big.hip (esn_solve.h: the parameter block, the workspace sizes)
int launch_readout_solve(const ReadoutArgs& a);
int launch_readout_chol(const ReadoutArgs& a);
int launch_readout_chol_big(const ReadoutArgs& a);
// esn_loo.hip: leave-one-out choice among n_ridge candidates per group; the workspace holds ridge_loo_work_doubles()
// doubles per group (the un-factored Gram matrix, the right-hand side and the best solution so far)
size_t ridge_loo_work_doubles();
int launch_ridge_loo(const ReadoutArgs& a);
// esn_holdout.hip: the candidates W [n_groups][n_ridge][n_out][cols] of a multi-lambda solve scored on rows
// [transient, T) of a held-out segment; exactly one of E / E32; t_scale, t_shift and status_in may be nullptr
struct HoldoutArgs {
    const double* E; const float* E32; const double* D; const double* W;
    int n_groups, T, transient, cols, n_out, n_ridge;
    const double *t_scale, *t_shift; const int* status_in;
    double* score; int* choice; hipStream_t stream;
};
int launch_holdout_score(const HoldoutArgs& a);
// esn_gram.hip: running normal equations.  Gm [n_groups][cols][cols] <- decay Gm + E^T E and Cm [n_groups][n_out][cols]
// <- decay Cm + D_s^T E over rows [transient, T), exactly one of E / E32; and (Gm + lambda I) W^T = Cm^T for n_ridge
// lambdas per group out of one factor buffer of gram_solve_work_doubles(cols) doubles per group
struct GramAccArgs {
    const double* E; const float* E32; const double* D;
    int n_groups, T, transient, cols, n_out;
    const double *t_scale, *t_shift; double decay;
    double *Gm, *Cm; hipStream_t stream;
};
struct GramSolveArgs {
    const double *Gm, *Cm; int n_groups, cols, n_out;
    const double* ridge; int n_ridge;
    double* W_out; int* status; void* workspace; size_t workspace_bytes; hipStream_t stream;
};
int gram_max_cols();
size_t gram_solve_work_doubles(int cols);
int launch_gram_accumulate(const GramAccArgs& a);
int launch_gram_solve(const GramSolveArgs& a);
// esn_reservoir.hip: reservoirs drawn, measured (spectral radius by repeated squaring) and rescaled on the device; the
// workspace holds specrad_work_doubles(n_res) doubles per matrix (two padded images, the per-tile norms, the log)
size_t specrad_work_doubles(int n_res);
int launch_gen_reservoirs(int n_res, int n_in, int n_out, double sparsity, uint64_t seed, uint64_t first_set,
                          int n_sets, const double* uniforms, double* W, double* W_in, double* W_fb,
                          hipStream_t stream);
int launch_spectral_radius(const double* W, int n_sets, int n_res, int n_squarings, double* radius, int* status,
                           void* workspace, hipStream_t stream);
int launch_scale_reservoirs(double* W, int n_sets, int n_res, double rho, const double* radius, const int* status,
                            hipStream_t stream);
// esn_specrad_split.hip: the same radius with every squaring as three fp16 MFMA products of split operands; the
// workspace (16-byte aligned) holds specrad_split_work_bytes(n_res) bytes per matrix
size_t specrad_split_work_bytes(int n_res);
int launch_spectral_radius_split(const double* W, int n_sets, int n_res, int n_squarings, double* radius, int* status,
                                 void* workspace, hipStream_t stream);
// esn_gen.hip
int launch_gen_taps(const TapParams& tp, hipStream_t stream);
int launch_gen_taps_doppler(const DopplerParams& dp, hipStream_t stream);
int launch_gen_frames(const FrameGenParams& fp, hipStream_t stream, bool c64 = false);
// esn_baseline.hip; MMSE_LDS_MAX: the dynamic LDS one workgroup of mmse_detect_kernel / mmse_equalize_rows_kernel may ask for
constexpr size_t MMSE_LDS_MAX = 150 * 1024;
// the LDS of one workgroup of channel_estimate_kernel, a function of the shape alone (served up to MMSE_LDS_MAX; -1 beyond)
size_t channel_estimate_lds_bytes(int n_sub, int n_t, int isi);
int launch_channel_estimate(const ChanEstParams& cp, hipStream_t stream);
int launch_mmse_detect(const MmseParams& mp, hipStream_t stream);
int launch_taps_to_freq(const TapsFreqParams& tp, hipStream_t stream);
// esn_equalize.hip: the LDS of one workgroup, a function of the shape alone (served up to MMSE_LDS_MAX)
size_t equalize_rows_lds_bytes(int n_sub, int n_t, int n_r);
int launch_equalize_rows(const EqRowsParams& ep, hipStream_t stream, bool io32);
// esn_dcc.hip: the LDS of one workgroup, a function of the shape alone (served up to MMSE_LDS_MAX; -1 beyond); DCC_MAX_ITER:
// the cancellation passes one launch serves
constexpr int DCC_MAX_ITER = 8;
size_t mmse_dcc_lds_bytes(int n_sub, int n_t, int n_r);
int launch_mmse_dcc(const DccParams& dp, hipStream_t stream);
// esn_chanstat.hip
int launch_channel_metrics(const ChanStatParams& cp, hipStream_t stream);
// esn_coded.hip
int launch_ldpc_encode(const LdpcEncodeParams& ep, hipStream_t stream);
int launch_qam_llr(const LlrParams& lp, hipStream_t stream);
int launch_ldpc_decode(const LdpcDecodeParams& dp, hipStream_t stream);
// esn_soft.hip; detect_llr_lds_bytes: the LDS of one workgroup of detect_llr_kernel (all n_t rows [N + 1] and N/2
// twiddles, double2), a function of the shape alone; launch_detect_llr returns -1 where it passes MMSE_LDS_MAX, before any
// HIP call -- the one check of it, which the entry point reports as -2 with the figures
int launch_mmse_sinr(const SinrParams& sp, hipStream_t stream);
int launch_qam_llr_weighted(const SoftLlrParams& lp, hipStream_t stream);
size_t detect_llr_lds_bytes(int n_sub, int n_t);
int launch_detect_llr(const DetectLlrParams& dp, hipStream_t stream, bool io32);
// esn_detect.hip; detect_geometry: the launch of the generic detector kernels (detect_count_kernel, detect_remod_kernel) --
// as many antennas per workgroup as fit LDS (rows [na][N + 1] and N/2 twiddles, double2), one workgroup per (frame,
// chunk of antennas), 32 threads per antenna; false where not even one antenna fits
struct DetectGeometry { int na_wg; size_t lds; dim3 grid, block; };
bool detect_geometry(const DetectParams& dp, DetectGeometry* g);
int launch_detect_count(const DetectParams& dp, hipStream_t stream, bool io32 = false);
// esn_ensemble.hip: the generic tail's geometry; with member_err a second row buffer per antenna
int launch_detect_count_ens(const EnsParams& ep, hipStream_t stream, bool io32);
// esn_remod.hip
int launch_detect_remod(const RemodParams& rp, hipStream_t stream);
// esn_chantrack.hip: the k ranges a sum is split into and the LDS of one workgroup, functions of the shape alone
int chantrack_segments(int n_sub, int n_t, int n_r);
size_t chantrack_lds_bytes(int n_sub, int n_t, int n_r, int isi);
int launch_channel_track(const ChanTrackParams& cp, hipStream_t stream);
// esn_elm.hip: float64 features (p.E) or fused float64 / fp16 prediction (p.Y) of the windowed ELM
int launch_elm_features(const ElmParams& p, hipStream_t stream);
int launch_elm_predict(int precision, const ElmParams& p, hipStream_t stream);
// the same kernels with max(., 0) for tanh and the bias column's weights in p.b_out: the windowed FNN's prediction
int launch_fnn_predict(int precision, const ElmParams& p, hipStream_t stream);
// esn_fnn.hip: per-group Adam training of the windowed FNN, one workgroup per group; the LDS image of one workgroup
// (a function of the shape alone) and the workspace that holds Adam's moments of W1
size_t fnn_train_lds_bytes(int n_in, int n_hidden, int window, int n_out, int T);
size_t fnn_train_workspace_bytes(int n_in, int n_hidden, int window, int n_groups);
int launch_fnn_train(const FnnTrainParams& p, hipStream_t stream);
// esn_cnn.hip: the windowed CNN.  cnn_shape_limit: nullptr if the shape is served, else the limit it misses;
// cnn_workspace_bytes: what n_groups trainings or a prediction of n_frames frames (either may be 0) need
const char* cnn_shape_limit(int n_in, int c1, int c2, int n_out, int kernel, int T);
size_t cnn_workspace_bytes(int n_in, int c1, int c2, int n_out, int kernel, int n_groups, int n_frames, int T);
int launch_cnn_train(const CnnParams& p, hipStream_t stream);
int launch_cnn_predict(const CnnParams& p, hipStream_t stream);
// esn_lstm.hip: the LSTM comparator, with the CNN's contract
const char* lstm_shape_limit(int n_in, int n_hidden, int n_out, int T);
size_t lstm_workspace_bytes(int n_in, int n_hidden, int n_out, int n_groups, int n_frames, int T);
int launch_lstm_train(const LstmParams& p, hipStream_t stream);
int launch_lstm_predict(const LstmParams& p, hipStream_t stream);
}  // namespace esn
