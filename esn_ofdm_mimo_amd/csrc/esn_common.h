// Shared host/device definitions for the ESN hot-path kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <type_traits>
#include "../../include/esn_hip.h"

namespace esn {

// Padded geometry of one recurrence problem.  The GEMM of one timestep is
//   P[Mp x Bt] = Wext[Mp x Kp] * Z[Kp x Bt],   Z = [X ; U ; F]
// with the state rows at k in [0,Mp), the (scaled) inputs at [kin, kin+n_in)
// and the fed-back output / teacher at [kfb, kfb+n_out).
struct Geometry {
    int Mp;     // n_res rounded up to the row tiling of the kernel
    int kin;    // == Mp
    int kfb;    // kin + round4(n_in)
    int Kp;     // total K, multiple of 32
    int Ks;     // LDS row stride in elements (Kp + conflict-avoidance pad)
    int Bt;     // frames per workgroup tile
    int NW, MT, NT;  // waves, row tiles / wave, column tiles / wave (MFMA kernels)
    int ro_parts;    // readout images per group: 1, or 2 (hi + lo) for fp16/bf16 with n_out > 8
    int ro_fold;     // fp16/bf16, n_out <= 8: rows 0-7 = hi, rows 8-15 = lo of ONE 16-row image
    int skew;        // predict: the two waves of a SIMD run one third of a step apart (esn_recur_mfma_impl.h)
    int big;         // fp16/bf16, N_res > 1024: the launch-per-step GEMM path (esn_big_predict.hip, esn_big_harvest.hip)
                     // serves this shape; the packed read-out then carries that path's image behind the persistent kernel's
    int s16;         // fp16/bf16: the 16x16x32 skewed predict kernel (esn_recur_skew16_impl.h) serves this shape; the
                     // packed weights and read-out then carry that kernel's images behind the 32x32x16 ones
    int m64;         // ESN_F64: 1 = the float64 matrix-pipe kernel (esn_recur_f64_mfma.hip) fits this shape;
    int Bt64;        //          then Mp..Ks, MT, NT describe ITS tiling, Bt64 its frames per tile and Bt
                     //          stays the tile of the vector-ALU kernel (esn_recur_f64.hip)
};

// Dynamic LDS of the persistent MFMA kernel (esn_recur_mfma_impl.h carves it in this order): the Zt image, the frame
// table, the {scale, shift} tables of inputs and outputs per 16-frame column tile, the raw-input staging area (the skewed
// schedule: one 1 KB slot per DMA instruction, two per column tile) and the input offsets of the frames.  mfma_geometry
// and the launch both ask here.
inline size_t mfma_lds_bytes(const Geometry& g, int es, int n_in, bool skew) {
    const size_t nown = g.Bt / 16;
    return (size_t)g.Bt * g.Ks * es + 4 * (size_t)g.Bt + 8 * nown * ((g.kfb - g.kin) + 16)
           + (skew ? nown * 2048 : 8 * (size_t)g.Bt * n_in) + 4 * (size_t)g.Bt;
}

struct RecurParams {
    int n_res, n_in, n_out, teacher_forcing;
    Geometry g;
    // Frames are ordered by group (frame = grp*F + j).  Workgroup tiles are cut from a padded
    // "slot" axis: slot = grp*Fpad + j, j < Fpad, valid iff j < F.  Fpad is a multiple of 16
    // when a readout runs (one W_out per 16-frame column tile) and a multiple of the tile when
    // every group has its own weight set, so a tile never mixes weight sets.
    int n_frames;          // total sequences
    int n_groups;
    int F;                 // frames per group
    int Fpad;              // slots per group
    int n_wsets;
    int spw;               // n_wsets > 1: slots per weight set (whole tiles); the slot axis is then SET-MAJOR -- set w
                           // owns slots [w spw, (w+1) spw) holding its groups w, w + n_wsets, w + 2 n_wsets, ... at
                           // Fpad slots each -- so a tile never mixes weight sets yet packs several groups; 0 = one set
    int T_in;              // valid input rows per frame
    int S;                 // recurrence steps
    int in_row_off;        // input row fed at step s is s + in_row_off (harvest: 1)
    int transient;
    int harvest;           // 1: teacher feedback, write E; 0: own-output feedback, write Y
    int n_tiles;
    const void* packed_w;   size_t wset_stride;   // bytes per weight set
    const void* packed_wout; size_t wout_stride;  // bytes per group
    size_t w64_off, wo64_off;                     // ESN_F64 images: byte offset of the MFMA-ordered copy
    size_t w16_off, wo16_off;                     // g.s16: byte offset of the 16x16x32 kernel's images
    const double* in_scale; const double* in_shift;
    const double* t_scale;  const double* t_shift;
    union { const double* U; const float* U32; };   // U32: predict with float32 I/O (esn_predict_batch_f32)
    const double* D;
    const double* x0; const double* y0;
    const double* noise_u;
    double noise; int noise_mode; uint64_t seed;
    double leak;           // leak rate a in (0, 1]: x = (1 - a) x_prev + a tanh(.) + noise; 1 = the reference (float64 kernels only)
    uint32_t frame_off;    // counter noise: global index of this launch's frame 0 (= group_offset * F, mod 2^32), so a
                           // frame draws the same noise whichever launch, chunk or rank it lands in
    int wset_rot;          // n_wsets > 1: group g uses weight set (g + wset_rot) % n_wsets (= group_offset % n_wsets)
    union { double* Y; float* Y32; };               // Y32: predict with float32 I/O
    double* E;
    float* E32;            // harvest: when set, the extended states are stored as float32 here (E unused)
    unsigned long long* stamps;   // diagnostic build (-DESN_STAMPS) only: [block0 wave][8] cycle sums
};

struct DetectParams {
    union { const double* Y; const float* Y32; };   // Y32: esn_detect_count_f32 (widened on load)
    int n_frames, frames_per_group, n_sub, log2n, n_t, m;
    const double* p_i; const uint8_t* tx_bits;
    long long* err; long long* bits; double* X_hat;
    int na_wg;             // antennas per workgroup (set by the launcher: all of them unless LDS is short)
};
// ensemble tail (esn_ensemble.hip): d.Y holds n_members slabs [K][B][N][2 n_t], d.err / d.bits / d.X_hat are the combination's
struct EnsParams {
    DetectParams d;
    int n_members;
    const double* weights;     // [groups][K], or nullptr: 1 / K each
    long long* member_err;     // [groups][K], or nullptr: no member is transformed on its own
};
// decide and re-modulate (esn_remod.hip): the tail above, then the decisions back in the time domain
struct RemodParams {
    DetectParams d;        // tx_bits may be nullptr (nothing is counted; err and bits are then not touched)
    int cp, delay;
    uint8_t* dec_bits;     // [B][N m][n_t] decided bits, or nullptr
    double* D_hat;         // [B][delay + cp + N][2 n_t] teacher rows of the decisions
};

// frame generator (esn_gen.hip)
struct TapParams {
    int kind;            // 0 = TDL-B, 1 = exponential PDP, 2 = flat unit-modulus (AWGN driver)
    int n_links;         // n_blocks * n_r * n_t
    int isi;
    int n_paths;         // 23 for TDL-B, isi for the exponential PDP, 1 for flat
    double path_sqrt_pow[24];        // sqrt of the (normalised) linear power of each path / tap
    double path_delay_samples[24];   // TDL-B: normalised delay * DS * fs
    const double* gains_in;          // optional complex [n_links][n_paths] standard normals (parity)
    uint64_t seed; uint64_t link_offset;
    double* taps;        // complex [n_links][isi]
};

// Doppler taps (gen_taps_doppler_kernel): the paths, powers and delays of TapParams, one tap set per OFDM symbol
struct DopplerParams {
    TapParams tp;        // kind 0 / 1 tables; n_links = n_blocks * links_per_block; gains_in unused;
                         // taps = complex [n_blocks][n_sym][links_per_block][isi]
    int n_sym;           // symbols stored per block: s = 0 .. n_sym - 1
    int links_per_block; // n_r * n_t
    double fd_tsym;      // Doppler frequency * symbol time, cycles per symbol
    const double* angles_in;   // optional [n_links][n_paths][ESN_DOPPLER_SINUSOIDS][2] = (a, phi) in half-turns (parity)
};

struct FrameGenParams {
    int n_frames, frames_per_block, n_sub, log2n, cp, n_t, n_r, isi, m;
    const double* p_i;        // [n_blocks]  Pi = 10^(EbNo/10) No
    const double* a_clip;     // [n_blocks]  PA clip level
    double no;
    const double* taps;       // complex [n_blocks][n_r][n_t][isi]
    const uint8_t* bits_in;   // optional [B][N*m][n_t]
    const double* noise_in;   // optional complex [B][T][n_r], unit-variance real and imaginary parts
    uint64_t seed; uint64_t frame_offset;
    uint8_t* bits;            // [B][N*m][n_t]
    union { double* x_cp; float* x_cp32; };   // optional complex [B][T][n_t] (pre-PA: the ESN teacher); x_cp32 complex64
    union { double* y_cp; float* y_cp32; };   // complex [B][T][n_r]; y_cp32: complex64 (esn_gen_frames_c64)
    int ls_pattern;           // 1: sparse LS pilot, subcarrier sc carries only tx = sc % n_t (driver:330-333)
    int ko;                   // diagnostic (esn_debug_set "gen_ko"): bit0 no AWGN draw, bit1 no channel MACs, bit2 no IFFT, bit3 no PA
};

// baseline equaliser (esn_baseline.hip)
struct ChanEstParams {
    int n_blocks, n_sub, log2n, cp, n_t, n_r, isi, m;
    int ls_only;                 // 1: stop at the interpolated LS estimate (H_LS), no time-domain MMSE refinement
    const double* p_i; double no;
    const uint8_t* pilot_bits;   // [G][N*m][n_t]
    const double* y_ls_cp;       // complex [G][T][n_r]
    double* H;                   // complex [G][N][n_r][n_t]
};
struct TapsFreqParams {
    int n_blocks, n_sub, n_t, n_r, isi;
    const double* taps;          // complex [G][n_r][n_t][isi]
    double* H;                   // complex [G][N][n_r][n_t]
};
// channel rank / condition / capacity record (esn_chanstat.hip)
struct ChanStatParams {
    int n_blocks, n_sub, n_t, n_r;
    const double* H;             // complex [G][N][n_r][n_t]
    const double* p_i; double no;
    double* S;                   // optional [G][N][min(n_t, n_r)], descending
    double* cond;                // [G][N]
    uint8_t* rank;               // [G][N]
    double* cap;                 // [G]
};
struct MmseParams {
    int n_frames, frames_per_group, n_sub, log2n, cp, n_t, n_r, m;
    int zf;                      // 1: zero forcing, G = H^H H + 1e-12 I (driver :34-39); 0: MMSE, G = H^H H + No/Pi I
    const double* p_i; double no;
    const double* H;             // complex [G][N][n_r][n_t]
    const double* y_cp;          // complex [B][T][n_r]
    const uint8_t* tx_bits;      // [B][N*m][n_t]
    long long* err; long long* bits; double* X_hat;
};
// the equaliser's output back in the time domain (esn_equalize.hip)
struct EqRowsParams {
    int n_frames, frames_per_group, n_sub, log2n, cp, pad, n_t, n_r;
    const double* p_i; double no;
    const double* H;             // complex [G][N][n_r][n_t]
    const double* y_cp;          // complex [B][T][n_r]
    void* U_eq;                  // [B][cp + N + pad][2 n_t], float64 or float32
    double* X_hat;               // optional complex [B][N][n_t]
};
// the MMSE detector with decision-aided cancellation of the amplifier's distortion (esn_dcc.hip)
struct DccParams {
    int n_frames, frames_per_group, n_sub, log2n, cp, n_t, n_r, m, n_iter;
    const double* p_i;           // [groups]
    const double* a_clip;        // [groups]
    double no;
    const double* H;             // complex [G][N][n_r][n_t]
    const double* y_cp;          // complex [B][T][n_r]
    const uint8_t* tx_bits;      // [B][N*m][n_t], or nullptr: nothing is counted
    long long* err; long long* bits;
    long long* err_iter;         // optional [groups][n_iter + 1]
    double* X_hat;               // optional complex [B][N][n_t]
};
// decision-directed channel estimate (esn_chantrack.hip): estimate e reads frames e window .. e window + window - 1
struct ChanTrackParams {
    int n_est, window, est_per_group, n_sub, log2n, cp, n_t, n_r, isi, m;
    const double* y_cp;          // complex [n_est window][T][n_r]
    const double* X_hat;         // complex [n_est window][N][n_t], or nullptr: then bits
    const uint8_t* bits;         // [n_est window][N*m][n_t]
    const double* p_i;           // [groups]
    const double* reg;           // [groups][isi]
    double* taps;                // complex [n_est][n_r][n_t][isi], or nullptr
    double* H;                   // complex [n_est][N][n_r][n_t]
    int* status;                 // [n_est]
    int n_seg, log2m2;           // set by the launcher: k ranges per sum; log2 of n_t isi rounded up to a power of two
};
// windowed ELM (esn_elm.hip): a random tanh layer over the last `window` input rows, a bias column, a linear read-out.
// Sequence q belongs to group q / seq_per_group and reads weight set (group_offset + group) % n_wsets.
struct ElmParams {
    int n_in, n_hidden, window, bias_col, n_wsets, n_out, e_cols;
    int n_seq, seq_per_group, T_in, T, transient;      // features: one sequence per group, transient 0
    unsigned long long group_offset;
    const double* W_in;          // [n_wsets][n_hidden][window n_in], window sample 0 the oldest
    const double* b;             // [n_wsets][n_hidden]
    const double* W_out;         // [groups][n_out][e_cols]                       (predict)
    const double *in_scale, *in_shift;   // [groups][n_in] or nullptr
    const double *t_scale, *t_shift;     // [groups][n_out] or nullptr             (predict)
    const double* U;             // [n_seq][T_in][n_in]
    double* Y;                   // [n_seq][T - transient][n_out]                 (predict)
    void* E; int e_f32;          // [groups][T][e_cols] float64 or float32         (features)
    const double* b_out;         // [groups][n_out]: the ReLU instantiations (windowed FNN) read the weights of the bias
                                 // column here, W_out = W2 has rows of e_cols = n_hidden; the tanh ones never look
};
// windowed FNN (esn_fnn.hip): Linear -> ReLU -> Linear over the ELM's window, trained per group by full-batch Adam
struct FnnTrainParams {
    int n_in, n_hidden, window, n_out, n_isets, n_groups, T_in, T, transient, epochs;
    unsigned long long group_offset;
    double lr, beta1, beta2, eps;
    const double *W1_0, *b1_0, *W2_0, *b2_0;         // [n_isets][...]: group g starts from (group_offset + g) % n_isets
    const double *in_scale, *in_shift, *t_scale, *t_shift;   // [groups][n] or nullptr
    const double* U;             // [groups][T_in][n_in]
    const double* D;             // [groups][T][n_out]
    double *W1, *b1, *W2, *b2;   // [groups][...]
    double* loss;                // [groups][epochs] or nullptr
    double* workspace;           // the moments of W1: fnn_train_workspace_bytes
};
// windowed CNN (esn_cnn.hip): three Conv1d layers n_in -> c1 -> c2 -> n_out of one odd kernel size over the whole
// sequence, zero padded, ReLU after the first two; trained per group by full-batch Adam (T_in .. group_offset, epochs ..
// loss as in FnnTrainParams) or evaluated per frame (n_frames, frames_per_group, Y)
struct CnnParams {
    int n_in, c1, c2, n_out, kernel, n_isets, n_groups, T_in, T, transient, epochs;
    int n_frames, frames_per_group;                  // predict: frame f reads the set of group f / frames_per_group
    unsigned long long group_offset;
    double lr, beta1, beta2, eps;
    const double* W0[3];         // train: [n_isets][c_l][c_{l-1}][kernel] initial;  predict: [groups][...] trained
    const double* b0[3];         // [..][c_l]
    const double *in_scale, *in_shift, *t_scale, *t_shift;   // [groups][n] or nullptr
    const double* U;             // [groups | n_frames][T_in][n_in]
    const double* D;             // [groups][T][n_out]                              (train)
    double* W[3];                // [groups][c_l][c_{l-1}][kernel]                  (train)
    double* b[3];                // [groups][c_l]
    double* loss;                // [groups][epochs] or nullptr
    double* Y;                   // [n_frames][T - transient][n_out]                (predict)
    double* workspace;           // cnn_workspace_bytes
};
// LSTM comparator (esn_lstm.hip): one LSTM layer n_in -> n_hidden and a linear read-out n_hidden -> n_out over the whole
// sequence, parameters in torch's layout (gate order i, f, g, o), sets l = 0, 1, 2 = (W_ih, b_ih), (W_hh, b_hh),
// (W_fc, b_fc); trained per group by full-batch Adam or evaluated per frame, every other field as in CnnParams
struct LstmParams {
    int n_in, n_hidden, n_out, n_isets, n_groups, T_in, T, transient, epochs;
    int n_frames, frames_per_group;
    unsigned long long group_offset;
    double lr, beta1, beta2, eps;
    const double* W0[3];         // train: [n_isets][4H][n_in], [n_isets][4H][H], [n_isets][n_out][H] initial;  predict: [groups]
    const double* b0[3];         // [..][4H], [..][4H], [..][n_out]
    const double *in_scale, *in_shift, *t_scale, *t_shift;   // [groups][n] or nullptr
    const double* U;             // [groups | n_frames][T_in][n_in]
    const double* D;             // [groups][T][n_out]                              (train)
    double* W[3];                // [groups][...]                                   (train)
    double* b[3];
    double* loss;                // [groups][epochs] or nullptr
    double* Y;                   // [n_frames][T - transient][n_out]                (predict)
    double* workspace;           // lstm_workspace_bytes
};

// coded leg (esn_coded.hip)
struct LdpcEncodeParams {
    int n_frames, n_t, k, n;
    const uint8_t* P;        // [n-k][k] parity part of the systematic generator (bytes 0/1)
    const uint8_t* u;        // [B][n_t][k] information bits
    uint8_t* bits;           // [B][n][n_t]  (TxBits layout, n = N*m)
};
struct LlrParams {
    int n_frames, n_sub, n_t, m;
    const double* X_hat;     // complex [B][N][n_t]
    double* llr;             // [B][n_t][N*m]
    double* sigma2;          // optional [B]
};
// SINR-weighted soft outputs (esn_soft.hip)
struct SinrParams {
    int n_blocks, n_sub, n_t, n_r;
    const double* p_i; double no;
    const double* H;         // complex [G][N][n_r][n_t]
    double* w;               // [G][N][n_t] SINR over the block's mean SINR
    double* mu;              // [G][N][n_t] bias 1 - t
    double* gamma_mean;      // optional [G]
};
struct SoftLlrParams {
    LlrParams l;             // frames, shape, X_hat, llr, sigma2 as qam_llr_kernel reads them
    int frames_per_group;
    const double* w;         // [G][N][n_t], or nullptr: 1
    const double* mu;        // [G][N][n_t], or nullptr: 1
};
struct DetectLlrParams {
    DetectParams d;          // tx_bits may be nullptr (nothing is counted; err and bits are then not touched)
    const double* w;         // as SoftLlrParams
    const double* mu;
    double* llr;             // [B][n_t][N*m]
    double* sigma2;          // optional [B]
};
struct LdpcDecodeParams {
    int n_cw, n, k, m_checks, n_edges, maxiter, cw_per_group;
    double var;              // 10^(-snr_db/10)
    const int* chk_ptr;      // [m_checks+1] edges of check c: chk_ptr[c] .. chk_ptr[c+1]
    const int* edge_var;     // [E] variable of edge e (check-major order)
    const int* var_ptr;      // [n+1]
    const int* var_edge;     // [E] edge ids of variable v
    const double* y;         // [n_cw][n] observations (bit 0 <-> +)
    const uint8_t* u_true;   // optional [n_cw][k]
    uint8_t* x_out;          // optional [n_cw][n]
    long long* err; long long* bits;
};

// slot -> group (n_groups or beyond = none) and the position j inside the group's Fpad slots
__device__ __forceinline__ int slot_group(const RecurParams& p, int slot, int& j) {
    if (p.spw == 0) {
        const int grp = slot / p.Fpad;
        j = slot - grp * p.Fpad;
        return grp;
    }
    const int w = slot / p.spw, ls = slot - w * p.spw;
    const int gi = ls / p.Fpad;
    j = ls - gi * p.Fpad;
    const int grp = gi * p.n_wsets + w;
    return (w < p.n_wsets) ? grp : p.n_groups;
}
__device__ __forceinline__ int slot_group(const RecurParams& p, int slot) { int j; return slot_group(p, slot, j); }
// weight set of the tile that starts at slot0
__device__ __forceinline__ int slot_wset(const RecurParams& p, int slot0) {
    if (!p.spw) return 0;
    const int w = slot0 / p.spw + p.wset_rot;
    return w >= p.n_wsets ? w - p.n_wsets : w;
}
// slot -> frame index (or -1 for padding) and its group
__device__ __forceinline__ int slot_frame(const RecurParams& p, int slot, int& grp) {
    int j;
    grp = slot_group(p, slot, j);
    const int fr = grp * p.F + j;
    return (j < p.F && grp < p.n_groups && fr < p.n_frames) ? fr : -1;
}

// predict I/O element: float64 (esn_predict_batch) or float32 (esn_predict_batch_f32).  The kernels narrow every
// input to float (or scale it in double) before any arithmetic, so a float32 input widened to double gives the same
// recurrence; the float32 output is the rounded float64 one.
template <bool IO32> using io_elem = typename std::conditional<IO32, float, double>::type;
template <bool IO32> __device__ __forceinline__ const io_elem<IO32>* in_ptr(const RecurParams& p) {
    if constexpr (IO32) return p.U32; else return p.U;
}
template <bool IO32> __device__ __forceinline__ io_elem<IO32>* out_ptr(const RecurParams& p) {
    if constexpr (IO32) return p.Y32; else return p.Y;
}

inline __host__ __device__ int round_up(int x, int m) { return (x + m - 1) / m * m; }

// one Adam step of one parameter with gradient q (include/esn_hip.h, the FNN block): step = lr / (1 - beta1^e),
// rs2 = sqrt(1 - beta2^e).  Shared by the trainings of the windowed FNN and CNN.
__device__ __forceinline__ void fnn_adam(double& prm, double& m, double& v, double q, double beta1, double beta2,
                                         double step, double rs2, double eps) {
    m = beta1 * m + (1.0 - beta1) * q;
    v = beta2 * v + (1.0 - beta2) * (q * q);
    prm -= step * (m / (sqrt(v) / rs2 + eps));
}

// k order of the 16x16x32 skewed kernel (esn_recur_skew16_impl.h): position of natural column k inside the padded
// K axis.  State rows: R = 32 kk + 16 t + 4 g + e  ->  32 kk + 8 g + 4 t + e (the accumulator rows 4 g .. 4 g + 3 of two
// row tiles form one 16-byte chunk of the next step's B operand); the [U ; F] group (k >= 512) keeps natural order.
inline __host__ __device__ int s16_pos(int k) {
    return k < 512 ? (k & ~31) + 8 * ((k & 15) >> 2) + 4 * ((k & 31) >> 4) + (k & 3) : k;
}
inline __host__ __device__ int s16_nat(int pos) {       // inverse of s16_pos
    return pos < 512 ? (pos & ~31) + 16 * ((pos & 7) >> 2) + 4 * ((pos & 31) >> 3) + (pos & 3) : pos;
}

// Tuning / diagnostic knobs (benchmarks and A/B tests only).  Read ONCE per process from the
// environment and changed afterwards only through the debug entry point esn_debug_set -- never re-read per
// launch; keys, variables and parse rules are the rows of ONE table (esn_api.hip: kKnobTable).  None of
// them changes a packed image: the weight image depends on (precision, n_res, n_in, n_out) alone.
struct Knobs {
    int skew;              // 1 (default): skewed schedule where it applies; 0: in-step schedule
    int geom16[3];         // fp16/bf16 predict tiling override {NW, MT, NT}; {0,0,0} = table
    int geom32[3];         // float32 predict tiling override
    int chol_skip;         // bit mask of Cholesky-solve phases to drop (tools/time_chol.py)
    int chol_dma;          // 1 (default): the LDS Cholesky solve feeds its Gram and W_out passes of float32 E by LDS-DMA
                           // rings; 0: the register-staged passes (A/B and bitwise tests)
    int f64_mfma;          // 1 (default): float64 batches run on the matrix pipe; 0: vector-ALU kernel (A/B tests)
    int big_gemm;          // 1 (default): N_res > 1024 predict runs as one GEMM launch per step when a workspace is given
    int cluster;           // 1 (default): ONE float64 sequence runs on the LDS-resident cluster kernel when a workspace is given
    int gen_ko;            // frame generator knock-out mask for tools/time_gen.py (timing only, wrong frames)
    int s16;               // 1 (default): fp16/bf16 predict at 257..512 units on the 16x16x32 kernel; 0: the 32x32x16 one (A/B)
    int hcluster;          // 1 (default): fp16/bf16 harvest at 257..512 units on the cluster kernel (two members per cluster)
                           // when a workspace is given; 0: the persistent kernel (A/B and the tests' reference)
    int detect_fixed;      // 1 (default): the detector tail at (N 128, n_t 4, 16-QAM) runs its fixed-shape instance; 0: every
                           // call runs the generic kernel (A/B and bitwise tests)
};
Knobs& knobs();

// Bijective XCD-aware remap (guide T1): consecutive logical tiles land on the
// same XCD so tiles of one weight set share that XCD's L2.  Speed only.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int nx = 8;
    if (nwg < nx) return bid;
    int q = nwg / nx, r = nwg % nx, x = bid % nx, i = bid / nx;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// Counter-based uniform in [0,1): two 16-bit samples per 32-bit hash.  Keyed by
// (seed, frame, step) once per column, then one integer mix per pair of rows.
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t noise_key(uint64_t seed, uint32_t frame, uint32_t step) {
    uint32_t k = mix32((uint32_t)seed ^ (frame * 0x9E3779B9U));
    k = mix32(k ^ (uint32_t)(seed >> 32) ^ (step * 0x85EBCA6BU + 0x27d4eb2fU));
    return k;
}
// Four uniform bytes for reservoir rows 4*row4 .. 4*row4+3 under key `k`: additive counter, fold,
// one full-rate 24-bit multiply (v_mul_u32_u24), fold -- 4 integer ops per 4 samples.  Measured on
// 82 800 keys x 128 quads x 4 bytes: byte histogram chi2/255 = 0.93, rms correlation between any
// two (row, byte) positions 3.9e-3 (sampling floor 3.5e-3), max 0.046, lag-1 correlation across
// steps / frames < 1e-4.  A pure function of (seed, frame, step, row): every kernel, tiling and
// rank draws the same noise.
__device__ __forceinline__ uint32_t noise_mix(uint32_t s) {
    s ^= s >> 16;
    s = __umul24(s, 0x9E3779U);
    s ^= s >> 16;
    return s;
}
// the additive counter's step per row quad: a schedule may fold part of row4 into its key ahead of time
// (key + part * NOISE_ROW4_STRIDE) and pass noise_quad the rest
constexpr uint32_t NOISE_ROW4_STRIDE = 0x9E3779B9U;
__device__ __forceinline__ uint32_t noise_quad(uint32_t k, uint32_t row4) {
    return noise_mix(k + row4 * NOISE_ROW4_STRIDE);
}
// uniform in (0,1) with 8-bit resolution for byte `b` (0..3) of a quad: (byte + 0.5) / 256
__device__ __forceinline__ float noise_byte(uint32_t quad, int b) {
    return (float)((quad >> (8 * b)) & 0xffU) * (1.0f / 256.0f) + (0.5f / 256.0f);
}
__device__ __forceinline__ float noise_uniform(uint32_t k, uint32_t row) {
    return noise_byte(noise_quad(k, row >> 2), (int)(row & 3));
}

// float32 tanh: odd Taylor polynomial below 0.3 (truncation < 2e-9 relative),
// 1 - 2/(exp(2|x|)+1) above; both evaluated, selected per lane (no divergence).
constexpr float TANH32_SERIES_MAX = 0.3f;
__device__ __forceinline__ float tanh_f32_series(float x) {
    float x2 = x * x;
    float p = -0.00886323552990220f;            // -1382/155925
    p = fmaf(p, x2, 0.0218694885361552f);      //  62/2835
    p = fmaf(p, x2, -0.0539682539682540f);     // -17/315
    p = fmaf(p, x2, 0.133333333333333f);       //  2/15
    p = fmaf(p, x2, -0.333333333333333f);      // -1/3
    return fmaf(p * x2, x, x);
}
__device__ __forceinline__ float tanh_f32(float x) {
    float ax = fabsf(x);
    float p = tanh_f32_series(x);
    float e = __expf(2.0f * ax);                // v_exp_f32 path
    float r = 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);   // v_rcp_f32 (1 ulp), not an IEEE divide
    r = copysignf(r, x);
    return ax < TANH32_SERIES_MAX ? p : r;
}

// float64 tanh on |x| <= TANH64_SERIES_MAX: the odd Maclaurin series through x^21 in Horner form (12 DP
// instructions against ~80 of the library routine).  Coefficients are the exact rationals
// B_2n 4^n (4^n - 1) / (2n)!; the first dropped term is 3.9e-5 x^23, below 2.3e-18 |x| on the interval, so
// the result is the correctly rounded series to ~1 ulp.  Callers test the whole wave's pre-activations and
// fall back to tanh() when any lies outside.
constexpr double TANH64_SERIES_MAX = 0.25;
__device__ __forceinline__ double tanh_f64_series(double x) {
    const double u = x * x;
    double p = 9.691537956929451e-05;             //  18888466084/194896477400625
    p = fma(p, u, -2.3912911424355248e-04);       // -443861162/1856156927625
    p = fma(p, u, 5.90027440945586e-04);          //  6404582/10854718875
    p = fma(p, u, -1.4558343870513183e-03);       // -929569/638512875
    p = fma(p, u, 3.592128036572481e-03);         //  21844/6081075
    p = fma(p, u, -8.863235529902197e-03);        // -1382/155925
    p = fma(p, u, 2.1869488536155203e-02);        //  62/2835
    p = fma(p, u, -5.396825396825397e-02);        // -17/315
    p = fma(p, u, 1.3333333333333333e-01);        //  2/15
    p = fma(p, u, -3.333333333333333e-01);        // -1/3
    return fma(p * u, x, x);
}

// tanh for the fp16/bf16 kernels.  The packed weights of those kernels are pre-multiplied by
// ACT_PRESCALE = 2 log2(e), so the accumulator already holds z = 2 log2(e) P and
//   tanh(P) = 1 - 2 / (1 + 2^z)            (v_exp_f32, v_add, v_rcp_f32, v_fma: 4 instructions)
// +-inf are handled by the instructions themselves (2^z -> inf -> rcp 0 -> 1; 2^z -> 0 -> -1).
// Absolute error ~6e-8 (float32 cancellation near 0), far below the 2^-11 relative rounding of
// the fp16 state the result is stored in.
constexpr double ACT_PRESCALE = 2.8853900817779268;   // 2 / ln 2
__device__ __forceinline__ float tanh_prescaled(float z) {
    float e = __builtin_amdgcn_exp2f(z);
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
}

#ifdef ESN_STAMPS
#define ESN_STAMP(var) unsigned long long var; { __builtin_amdgcn_sched_barrier(0); \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var) :: "memory"); __builtin_amdgcn_sched_barrier(0); }
#define ESN_STAMP_SET(var) { __builtin_amdgcn_sched_barrier(0); \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var) :: "memory"); __builtin_amdgcn_sched_barrier(0); }
#define ESN_STAMPS_ONLY(...) __VA_ARGS__      // what only the diagnostic build holds: accumulators, sums, the write-out
#else
#define ESN_STAMP(var)
#define ESN_STAMP_SET(var)
#define ESN_STAMPS_ONLY(...)
#endif

}  // namespace esn
