/* esn_hip.h -- C ABI of the MI355X-native ESN OFDM/MIMO detector hot path.
 *
 * Shared library: esn_ofdm_mimo_amd/libesn_hip.so (built by __graft_entry__.build()).
 * Every entry point is extern "C", takes plain pointers and sizes, returns an int
 * status (0 = ok, <0 = error; text via esn_last_error()) and launches its work
 * on the caller's hipStream_t (passed as void*; NULL = default stream).  No
 * hidden global state besides a thread-local error string and the tuning knobs
 * of esn_debug_set (below; never needed by a user); no exceptions cross
 * the boundary.  All array arguments are DEVICE pointers, except in the `esn_*_mem` entry points
 * called with ESN_MEM_HOST (below).  Arrays keep the reference's own row-major float64 layouts so a
 * binding needs no repacking:
 *
 *   inputs   U  [B][T_in][n_in]     (== complex128 [B][T_in][N_r] viewed as float64
 *                                    with Re/Im interleaved: the packing of
 *                                    Demo_MIMO_4x8_Sionna_CDL_ESN_v2.py:433-436 and
 *                                    helper_mimo_esn_generic.py:30-33 is a VIEW; the
 *                                    d trailing zero rows are synthesised: T > T_in)
 *   outputs  Y  [B][T-transient][n_out]  (== complex128 [B][N][N_t] view, :47-58)
 *
 * Reference interface each entry point replaces (paths relative to the
 * reference tree, libs/pyESN.py unless noted):
 *
 *   esn_pack_weights        ESN.initweights result W/W_in/W_feedb (:93-109) ->
 *                           device-resident, MFMA-fragment-ordered copy.
 *   esn_pack_readout        W_out of ESN.fit (:191-192) -> fragment-ordered copy.
 *   esn_predict_batch       ESN.predict (:218-255) incl. _scale_inputs (:127-135),
 *                           _update (:111-125), readout (:252), _unscale_teacher
 *                           (:146-152); batched over B frames in G groups.
 *   esn_harvest_batch       state-harvest loop of ESN.fit (:176-182,189) ->
 *                           extended states [states, inputs_scaled].
 *   esn_readout_solve_batch, esn_readout_solve_chol_batch
 *                           pinv solve of ESN.fit (:191-192).
 *   esn_gen_taps, esn_gen_frames   transmitter + channel + noise of the drivers (:127-177, :397-427).
 *   esn_channel_estimate, esn_mmse_detect_count   LS/MMSE baseline (:358-382, :40-45, :444-448).
 *   esn_detect_count        driver tail: reconstruct (:47-58 of the 4x8 driver),
 *                           (1/N) FFT / sqrt(Pi) (:439-441), hard decision
 *                           (:95-103), bit-error count (:451-456).
 */
#ifndef ESN_HIP_H
#define ESN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Arithmetic of the recurrence. */
enum esn_precision {
    ESN_F64 = 0,   /* float64, the reference's arithmetic: v_mfma_f64_16x16x4_f64 for batches (N_res <= 1024),
                      float64 FMA on the vector ALU for a single sequence and larger reservoirs */
    ESN_F32 = 1,   /* v_mfma_f32_32x32x2_f32: exact float32 products + accumulate */
    ESN_F16 = 2,   /* v_mfma_f32_16x16x32_f16 (predict at 257..512 units) / v_mfma_f32_32x32x16_f16: fp16 operands,
                      float32 accumulate */
    ESN_BF16 = 3   /* the same with bf16 operands */
};

/* State-noise source (pyESN.py:124-125: + noise * (U[0,1) - 0.5)). */
enum esn_noise_mode {
    ESN_NOISE_NONE = 0,     /* noise == 0                                             */
    ESN_NOISE_TENSOR = 1,   /* caller supplies the uniforms [B][S][n_res] (parity)     */
    ESN_NOISE_COUNTER = 2   /* counter-based generator keyed (seed, frame, step, row)  */
};

/* Geometry shared by the recurrence entry points. */
typedef struct esn_shape {
    int n_res;            /* reservoir size                                          */
    int n_in;             /* input units  (2 N_r)                                    */
    int n_out;            /* output units (2 N_t)                                    */
    int teacher_forcing;  /* 1: W_feedb term active (pyESN.py:117-120)               */
    int n_wsets;          /* number of (W, W_in, W_feedb) sets: 1 = shared reservoir */
    double leak_rate;     /* EXTENSION (the reference has none): x[t] = (1-a) x[t-1] + a tanh(...) + noise.
                             0 (what `{n_res, n_in, n_out, tf, n_wsets}` initialises it to) or 1 = the reference's
                             update.  Values in (0, 1) are served by ESN_F64 only (other precisions answer -2). */
} esn_shape_t;

const char* esn_last_error(void);

/* ABI version (bumped on any signature change): stated here only.  esn_abi_version() returns the value the library was
 * built with; a binding compares the two. */
#define ESN_ABI_VERSION 10
int esn_abi_version(void);

/* Tuning / diagnostic knobs for benchmarks and A/B tests (no counterpart in the reference).  The
 * library reads the initial value of every key but "gen_ko" from the environment ONCE, at its first call -- the
 * variable is ESN_ + the key in capitals: ESN_SKEW, ESN_MFMA_GEOM, ESN_MFMA_GEOM_F32, ESN_CHOL_SKIP, ESN_CHOL_DMA,
 * ESN_F64_MFMA, ESN_S16, ESN_BIG_GEMM, ESN_CLUSTER, ESN_HCLUSTER, ESN_DETECT_FIXED
 * (one table in csrc/esn_api.hip serves both) -- and afterwards only this call changes them:
 *   "skew"          "0" = in-step schedule for the fp16/bf16 predict kernel, else skewed (default)
 *   "mfma_geom"     "NW,MT,NT" re-cuts the fp16/bf16 predict tiling; ignored unless 32*NW*MT equals
 *   "mfma_geom_f32" the table's padded row count, so a packed image never goes stale; NULL = table
 *   "chol_skip"     bit mask of Cholesky-solve phases to drop (timing only, wrong results; Gram dimension <= 128):
 *                   1 Gram over the first 32-wide k-chunk only, 2 factorisation of the first 16-column block
 *                   only, 4 no blocked triangular solves, 8 no W_out = A^T alpha pass
 *   "chol_dma"      "0" = the Cholesky solve (Gram dimension <= 128, float32 E, rows < cols) stages E through
 *                   registers instead of LDS-DMA rings in its Gram and W_out passes (bitwise the same results; A/B runs)
 *   "f64_mfma"      "0" = ESN_F64 batches on the vector-ALU kernel instead of the float64 matrix pipe
 *   "s16"           "0" = fp16/bf16 predict at 257..512 units on the 32x32x16 skewed kernel instead of the 16x16x32 one
 *                   (esn_recur_skew16_impl.h, the default: same schedule, 4 % less wall time at a higher clock; A/B runs)
 *   "big_gemm"      "0" = N_res > 1024 predict on the persistent kernel even when a workspace is given
 *   "cluster"       "0" = a single float64 sequence on the vector-ALU kernel even when a workspace is given
 *   "hcluster"      "0" = fp16/bf16 harvest at 257..512 units on the persistent kernel even when a workspace is given
 *                   (default: pairs of workgroups, esn_harvest_cluster.hip).  esn_harvest_workspace_bytes follows the
 *                   knob: ask for the size after setting it
 *   "gen_ko"        frame-generator knock-out mask for tools/time_gen.py (timing only, wrong frames)
 *   "detect_fixed"  "0" = esn_detect_count / esn_detect_count_f32 always on the generic kernel.  By default a call
 *                   at N = 128, N_t = 4, 16-QAM with 16-byte aligned tx_bits and Y (8-byte for float Y) runs the
 *                   fixed-shape instance (esn_detect.hip: one wave per frame, eight frames per workgroup); counts
 *                   and X_hat are bitwise the same (tx_bits bytes are 0 or 1); A/B runs (ESN_DETECT_FIXED)
 * Returns 0, or -1 for an unknown key. */
int esn_debug_set(const char* key, const char* value);

/* The recurrence kernels behind esn_predict_batch / esn_harvest_batch.  Which one serves a call is decided in ONE
 * place (plan_recur, csrc/esn_api.hip) from the precision, the shape, the batch, the knobs above and whether the
 * caller lends a workspace; the first that applies, in this order:
 *   workspace lent:  CLUSTER_F64      ESN_F64, ONE sequence ("cluster")
 *                    HARVEST_CLUSTER  harvest, fp16/bf16, 257..512 units, n_in 2/4/8/16, n_out <= 8 ("hcluster")
 *                    BIG_PREDICT /    fp16/bf16, one weight set, n_in <= 16, n_out <= 8, beyond 1024 units ("big_gemm")
 *                    BIG_HARVEST
 *   predict:         SKEW16           fp16/bf16, 257..512 units, n_in 2/4/8/16, n_out <= 8 ("s16", "skew")
 *   otherwise:       F64_MFMA         ESN_F64, more than 8 sequences, where the matrix-pipe tiling fits ("f64_mfma")
 *                    F64_VALU         ESN_F64
 *                    MFMA             ESN_F32 / ESN_F16 / ESN_BF16: in-step or 32x32x16 skewed schedule ("skew") */
enum esn_path {
    ESN_PATH_MFMA = 0,             /* persistent MFMA kernel (esn_recur_mfma_impl.h)                         */
    ESN_PATH_SKEW16 = 1,           /* 16x16x32 skewed predict kernel (esn_recur_skew16_impl.h)               */
    ESN_PATH_F64_VALU = 2,         /* float64 on the vector ALU (esn_recur_f64.hip)                          */
    ESN_PATH_F64_MFMA = 3,         /* float64 matrix pipe (esn_recur_f64_mfma.hip)                           */
    ESN_PATH_CLUSTER_F64 = 4,      /* single float64 sequence, workgroup cluster (esn_recur_cluster.hip)     */
    ESN_PATH_BIG_PREDICT = 5,      /* one GEMM launch per step, predict (esn_big_predict.hip)                */
    ESN_PATH_BIG_HARVEST = 6,      /* one GEMM launch per step, harvest (esn_big_harvest.hip)                */
    ESN_PATH_HARVEST_CLUSTER = 7   /* fp16/bf16 harvest, workgroup clusters (esn_harvest_cluster.hip)        */
};
/* Which kernel esn_predict_batch (harvest = 0) / esn_harvest_batch (harvest = 1) runs for this call when a
 * workspace of the advertised size is lent (have_workspace = 1) or not (0), under the current knobs: the answer of
 * the same function the calls dispatch through.  n_sequences = n_frames (predict) or n_groups (harvest, where
 * frames_per_group is ignored).  The paths CLUSTER_F64, BIG_PREDICT, BIG_HARVEST and HARVEST_CLUSTER read the
 * workspace; of these CLUSTER_F64 and HARVEST_CLUSTER keep an error word in its last 64 bytes.
 * Returns an esn_path value >= 0, or a negative error as the calls themselves would.  Diagnostic. */
int esn_recur_path(int harvest, int precision, const esn_shape_t* shape, int n_sequences,
                   int frames_per_group, int have_workspace);

/* Device facts used for roofline reporting (any pointer may be NULL). */
int esn_device_info(int* cu_count, int* lds_bytes_per_cu, int* clock_khz,
                    char* arch_name, int arch_name_len);

/* Frames per workgroup tile the recurrence kernel uses for this shape and
 * precision (>= 1).  Padding happens inside the kernel, never in the caller's
 * arrays: a group's frames are padded to a multiple of 16 (the MFMA column
 * tile; no padding on the float64 vector-ALU path), and with n_wsets > 1 the
 * groups of one weight set are laid end to end and that span is rounded up to
 * whole tiles, so a tile streams one weight image and may serve several groups. */
int esn_tile_frames(int precision, const esn_shape_t* shape);

/* Bytes of the packed weight image for one weight set / one readout. */
size_t esn_packed_weights_bytes(int precision, const esn_shape_t* shape);
size_t esn_packed_readout_bytes(int precision, const esn_shape_t* shape);

/* W [n_wsets][n_res][n_res], W_in [n_wsets][n_res][n_in], W_fb [n_wsets][n_res][n_out]
 * (float64, row-major) -> packed [n_wsets][esn_packed_weights_bytes]. */
int esn_pack_weights(int precision, const esn_shape_t* shape,
                     const double* W, const double* W_in, const double* W_fb,
                     void* packed, void* stream);

/* W_out [n_groups][n_out][n_res+n_in] (float64) -> packed [n_groups][esn_packed_readout_bytes]. */
int esn_pack_readout(int precision, const esn_shape_t* shape, int n_groups,
                     const double* W_out, void* packed, void* stream);

/* Batched ESN.predict.
 *
 * Frames are ordered by group: frame b belongs to group b / frames_per_group
 * (its W_out, scalings, initial state) and, when shape->n_wsets > 1, to weight
 * set (group_offset + b / frames_per_group) % n_wsets.
 *
 *   group_offset  global index of this call's group 0 in the caller's sweep (0 for a stand-alone call).  The
 *                 counter noise of frame b is keyed by (seed, group_offset * frames_per_group + b, step, row) and the
 *                 weight set by the global group, so cutting a sweep into chunks, launches or ranks
 *                 changes neither: a frame's result is a function of its global index only.  (The frame index
 *                 enters the key modulo 2^32.)
 *
 *   packed_w      from esn_pack_weights            packed_wout  from esn_pack_readout
 *   in_scale/in_shift   [n_groups][n_in]  or NULL (=1 / =0)        (pyESN.py:131-134)
 *   t_scale/t_shift     [n_groups][n_out] or NULL                  (pyESN.py:140-151)
 *   U             [B][T_in][n_in]; rows T_in..T-1 are zeros before scaling
 *   x0, y0        [n_groups][n_res], [n_groups][n_out] start state and fed-back
 *                 output (continuation=True: laststate/lastoutput, :234-237) or NULL (zeros)
 *   noise_u       [B][T][n_res] uniforms when noise_mode == ESN_NOISE_TENSOR
 *   Y             [B][T-transient][n_out], unscaled (:255); 16-byte aligned (rows are written as 16-byte pairs)
 *   workspace     device scratch of esn_predict_workspace_bytes(...) bytes, or NULL.  The paths BIG_PREDICT and
 *                 CLUSTER_F64 use it (enum esn_path; esn_recur_path tells which one a call takes): reservoirs
 *                 beyond 1024 units in fp16/bf16 (the recurrence runs as one tiled GEMM launch
 *                 per timestep with the state images in the workspace), and ONE float64 sequence (n_frames = 1:
 *                 the reference's own call pattern) -- the matrix then stays resident in the LDS of a cluster of
 *                 co-resident workgroups that exchange the state through the workspace every step
 *                 (esn_recur_cluster.hip); its last 64 bytes hold an error word that is non-zero if a workgroup
 *                 timed out waiting for the others (the outputs are then invalid).  With NULL every shape runs on
 *                 the persistent kernels.  No allocation happens inside the call either way.
 */
size_t esn_predict_workspace_bytes(int precision, const esn_shape_t* shape, int n_frames, int frames_per_group);
int esn_predict_batch(int precision, const esn_shape_t* shape,
                      const void* packed_w, const void* packed_wout,
                      const double* in_scale, const double* in_shift,
                      const double* t_scale, const double* t_shift,
                      const double* U, int n_frames, int frames_per_group,
                      int T_in, int T, int transient,
                      const double* x0, const double* y0,
                      double noise, int noise_mode, const double* noise_u,
                      uint64_t seed, uint64_t group_offset,
                      double* Y, void* workspace, size_t workspace_bytes, void* stream);

/* Same predict with float32 I/O: U float [B][T_in][n_in] (16-byte aligned when n_in is a multiple of 4, else 4-byte),
 * Y float [B][T-transient][n_out] (16-byte aligned); every
 * other argument (scalings, x0 / y0, noise_u, workspace) as above.  Half the bytes of U and Y; no counterpart in the
 * reference, whose arrays are float64.
 *   Bitwise contract: Y equals (float) of the Y esn_predict_batch writes for the same call with U widened to double.
 *   Every kernel that serves it narrows an input to float (or scales it in double) before any arithmetic, so the
 *   recurrence is the same; the store rounds the value the float64 path would write (a float in the persistent
 *   kernels, a double in the N_res > 1024 GEMM path).
 *   Served: precisions ESN_F32 / ESN_F16 / ESN_BF16 on every path esn_predict_batch takes for them (the 16x16x32 and
 *   32x32x16 skewed kernels, the in-step kernel, N_res > 1024 with or without a workspace), any n_in (n_in = 2 included).
 *   Returns -2 for ESN_F64 (the vector-ALU, float64 matrix-pipe and single-sequence cluster kernels read and write
 *   float64 only), -1 for null pointers, bad sizes or a misaligned U or Y; all of these
 *   before any HIP call. */
int esn_predict_batch_f32(int precision, const esn_shape_t* shape,
                          const void* packed_w, const void* packed_wout,
                          const double* in_scale, const double* in_shift,
                          const double* t_scale, const double* t_shift,
                          const float* U, int n_frames, int frames_per_group,
                          int T_in, int T, int transient,
                          const double* x0, const double* y0,
                          double noise, int noise_mode, const double* noise_u,
                          uint64_t seed, uint64_t group_offset,
                          float* Y, void* workspace, size_t workspace_bytes, void* stream);

/* Batched state harvest of ESN.fit: one training sequence per group.
 *
 *   U [n_groups][T][n_in], D [n_groups][T][n_out] (teacher, unscaled)
 *   E [n_groups][T][n_res+n_in] = hstack(states, inputs_scaled) (:189); row 0 of
 *   the states is zero and input row 0 is never fed (:179-182).
 *   noise_u [n_groups][T-1][n_res] when noise_mode == ESN_NOISE_TENSOR.
 *   group_offset: as in esn_predict_batch (noise key and weight set follow the GLOBAL group index);
 *   E is 16-byte aligned.
 *   workspace: device scratch of esn_harvest_workspace_bytes(...) bytes, or NULL.  The paths BIG_HARVEST,
 *   HARVEST_CLUSTER and CLUSTER_F64 use it (enum esn_path; esn_recur_path tells which one a call takes): reservoirs
 *   beyond 1024 units in fp16/bf16 (one tiled GEMM launch per timestep, 128 x 64 tiles: a fit has one sequence per
 *   trained ESN, so the tile is cut for workgroup count); fp16/bf16 at 257..512 units (pairs
 *   of co-resident workgroups keep the weight matrix in registers and exchange their state slices through the
 *   workspace every step, esn_harvest_cluster.hip; its last 64 bytes hold an error word that is non-zero if a
 *   workgroup timed out waiting for its peer: the states are then invalid); and ONE float64 sequence (the cluster
 *   kernel of esn_predict_batch).  With NULL the persistent kernels run.
 *   precision: ESN_F64 / ESN_F32 keep the states at (better than) float32; ESN_F16 / ESN_BF16
 *   harvest states rounded to the operand type (round-off ~6e-6 abs, far below the model's own
 *   state noise 2.9e-4 rms) -- statistically equivalent, not bit-comparable.
 */
size_t esn_harvest_workspace_bytes(int precision, const esn_shape_t* shape, int n_groups);
int esn_harvest_batch(int precision, const esn_shape_t* shape,
                      const void* packed_w,
                      const double* in_scale, const double* in_shift,
                      const double* t_scale, const double* t_shift,
                      const double* U, const double* D, int n_groups, int T,
                      double noise, int noise_mode, const double* noise_u,
                      uint64_t seed, uint64_t group_offset, double* E,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Same harvest, extended states stored as float32 (MFMA precisions only: their state columns are
 * exactly representable, the scaled-input columns round at 6e-8 relative).  Halves the harvest's
 * store tail and the two passes esn_readout_solve_chol_batch_f32 makes over E.  No counterpart in
 * the reference (its states are float64, :176); an internal fast path of the batched fit. */
int esn_harvest_batch_f32(int precision, const esn_shape_t* shape,
                          const void* packed_w,
                          const double* in_scale, const double* in_shift,
                          const double* t_scale, const double* t_shift,
                          const double* U, const double* D, int n_groups, int T,
                          double noise, int noise_mode, const double* noise_u,
                          uint64_t seed, uint64_t group_offset, float* E,
                          void* workspace, size_t workspace_bytes, void* stream);

/* W_out[g] = (pinv(E[g][transient:]) @ (D[g][transient:]*t_scale + t_shift)).T  (:191-192)
 *
 * float64 Householder QR: of E^T when rows < cols (minimum-norm solution, what
 * pinv returns for the under-determined 4x8 case) and of E otherwise.
 *   workspace      esn_readout_solve_workspace_bytes(...) bytes of device memory
 *   status [n_groups]  0 = ok, 1 = numerically rank deficient (|r_jj| <= 1e-13 max|r|;
 *                  the dependent direction is dropped), written on device
 */
size_t esn_readout_solve_workspace_bytes(int n_groups, int rows, int cols, int n_out);
int esn_readout_solve_batch(const double* E, const double* D, int n_groups, int T,
                            int transient, int cols, int n_out,
                            const double* t_scale, const double* t_shift,
                            double* W_out, int* status, void* workspace, void* stream);

/* Same contract, normal equations in float64 on the float64 matrix pipe -- the fast path for well-conditioned
 * batched fits (with the model's state noise cond(E) ~ 1e3, error ~ cond^2 eps ~ 1e-10).  min(rows, cols) <= 128:
 * Gram matrix and Cholesky factor resident in LDS, no workspace (NULL).  129 .. 512 (4x8 at N = 512: 512 x 528;
 * N_res = 300: 512 x 316): Gram matrix / factor column-major in the caller's workspace of
 * esn_readout_chol_workspace_bytes(...) bytes (16-byte aligned, as E), left-looking blocked factorisation.
 * status[g] = 1 when a pivot was rejected: re-solve that group with esn_readout_solve_batch.  Needs n_out <= 8;
 * returns -2 when the shape is not served. */
size_t esn_readout_chol_workspace_bytes(int n_groups, int rows, int cols);
int esn_readout_solve_chol_batch(const double* E, const double* D, int n_groups, int T,
                                 int transient, int cols, int n_out,
                                 const double* t_scale, const double* t_shift,
                                 double* W_out, int* status, void* workspace, size_t workspace_bytes, void* stream);
/* ... with E as written by esn_harvest_batch_f32 (arithmetic still float64). */
int esn_readout_solve_chol_batch_f32(const float* E, const double* D, int n_groups, int T,
                                     int transient, int cols, int n_out,
                                     const double* t_scale, const double* t_shift,
                                     double* W_out, int* status, void* workspace, size_t workspace_bytes, void* stream);

/* Ridge-regression read-out -- an extension, OFF unless these entry points are called: the reference has no
 * counterpart (its ESN.fit is the pinv solve above, :191-192, and pinv stays this library's default and its
 * reference-parity mode).  For every trained ESN g and every l < n_ridge, over rows [transient, T) of E[g] and the
 * scaled teacher D_s = D[g]*t_scale + t_shift:
 *
 *     W_out[g][l] = argmin_W |E W^T - D_s|^2 + lambda |W|^2,     lambda = ridge[g][l] >= 0
 *
 * lambda is absolute, in the units of the Gram matrix of the (scaled) extended states: it is added to the diagonal
 * of E E^T (rows < cols: W^T = E^T (E E^T + lambda I)^-1 D_s) or E^T E (W^T = (E^T E + lambda I)^-1 E^T D_s); the
 * two forms are the same solution.  lambda = 0 is the pinv solve of the entry points above, bit for bit.
 *   ridge   [n_groups][n_ridge] float64, device: several lambda per pilot are solved in one launch
 *   W_out   [n_groups][n_ridge][n_out][cols];  status [n_groups][n_ridge]
 *   status  as in the pinv solves (0 ok, 1 rank deficient / pivot rejected), and 2 = lambda negative or not
 *           finite: that entry's W_out is all zero, the other entries are unaffected
 * The QR solve factorises the augmented matrix ([A ; sqrt(lambda) I], or [A  sqrt(lambda) I]^T when rows < cols),
 * so its workspace per entry holds rows + cols matrix rows; the Cholesky solves add lambda to the Gram diagonal
 * (same shapes as the pinv Cholesky solves: min(rows, cols) <= 512 and n_out <= 8, else -2; one workspace slice per
 * (group, lambda) beyond 128). */
size_t esn_readout_solve_ridge_workspace_bytes(int n_groups, int n_ridge, int rows, int cols, int n_out);
int esn_readout_solve_ridge_batch(const double* E, const double* D, int n_groups, int T,
                                  int transient, int cols, int n_out,
                                  const double* t_scale, const double* t_shift,
                                  const double* ridge, int n_ridge,
                                  double* W_out, int* status, void* workspace, void* stream);
size_t esn_readout_chol_ridge_workspace_bytes(int n_groups, int n_ridge, int rows, int cols);
int esn_readout_solve_chol_ridge_batch(const double* E, const double* D, int n_groups, int T,
                                       int transient, int cols, int n_out,
                                       const double* t_scale, const double* t_shift,
                                       const double* ridge, int n_ridge,
                                       double* W_out, int* status, void* workspace, size_t workspace_bytes,
                                       void* stream);
int esn_readout_solve_chol_ridge_batch_f32(const float* E, const double* D, int n_groups, int T,
                                           int transient, int cols, int n_out,
                                           const double* t_scale, const double* t_shift,
                                           const double* ridge, int n_ridge,
                                           double* W_out, int* status, void* workspace, size_t workspace_bytes,
                                           void* stream);

/* Leave-one-out choice of the ridge parameter (an extension, like the ridge solves above).  For every trained ESN g,
 * over rows [transient, T) of E[g] and the scaled teacher D_s (n = rows, c = cols), and for each candidate
 * lambda = ridge[g][l]: loo[i][o] is the residual of fit row i, output o, under the ridge fit on the other n - 1
 * rows, in closed form:
 *     n <= c:  K = E E^T + lambda I,  A = K^-1 D_s,                      loo[i][o] = A[i][o] / (K^-1)[i][i]
 *     n >  c:  G = E^T E + lambda I,  W^T = G^-1 E^T D_s,  R = D_s - E W^T,  loo[i][o] = R[i][o] / (1 - e_i^T G^-1 e_i)
 *     score[g][l] = sum_i sum_o loo[i][o]^2          (one lambda for all outputs; scaled-teacher units)
 * The Gram matrix is formed once per pilot, not once per candidate.
 *   ridge   [n_groups][n_ridge] float64, device; 1 <= n_ridge <= 16
 *   status  [n_groups][n_ridge]: 0 ok, 1 a pivot of the factorisation was rejected, 2 lambda negative or not finite;
 *           score is +inf where status is not 0
 *   choice  [n_groups]: the lowest l with the smallest finite score among the entries with status 0, -1 if none
 *   W_out   [n_groups][n_out][cols]: the ridge solution at ridge[g][choice[g]], all zero where choice is -1
 * A group's score, choice and W_out are bitwise the same alone and inside any batch.
 * Shapes: min(rows, cols) <= 128 (else -2, esn_last_error() names the limit), n_out <= 8 and n_ridge <= 16 (else -1).
 * The workspace (esn_readout_ridge_loo_workspace_bytes, 8-byte aligned) is always needed. */
size_t esn_readout_ridge_loo_workspace_bytes(int n_groups, int n_ridge, int rows, int cols);
int esn_readout_ridge_loo_batch(const double* E, const double* D, int n_groups, int T,
                                int transient, int cols, int n_out,
                                const double* t_scale, const double* t_shift,
                                const double* ridge, int n_ridge,
                                double* W_out, double* score, int* choice, int* status,
                                void* workspace, size_t workspace_bytes, void* stream);
int esn_readout_ridge_loo_batch_f32(const float* E, const double* D, int n_groups, int T,
                                    int transient, int cols, int n_out,
                                    const double* t_scale, const double* t_shift,
                                    const double* ridge, int n_ridge,
                                    double* W_out, double* score, int* choice, int* status,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* Hold-out score of the candidates of a multi-lambda solve (an extension, like the ridge solves above: the ABI version
 * is unchanged).  With several pilots per coherence block the read-outs W[g][l] fitted on all pilots but one are scored
 * on the pilot left out.  For every trained ESN g and every candidate l < n_ridge, over rows [transient, T) of the
 * held-out segment:
 *     D_s         = D[g] * t_scale[g] + t_shift[g]                          (NULL scale / shift: 1 / 0)
 *     r[i][o]     = sum_c E[g][i][c] * W[g][l][o][c] - D_s[i][o]
 *     score[g][l] = sum_i sum_o r[i][o]^2                                   (scaled-teacher units, as the LOO score)
 *     choice[g]   = the lowest l with the smallest finite score among the entries with status_in[g][l] == 0; -1 if none
 *   E          [n_groups][T][cols], float64 (or float32 for the _f32 twin: what esn_harvest_batch_f32 writes)
 *   D          [n_groups][T][n_out], unscaled
 *   W          [n_groups][n_ridge][n_out][cols] float64: the W_out of esn_readout_solve_*_ridge_batch
 *   status_in  [n_groups][n_ridge] (that solve's status), or NULL for all 0
 *   score      [n_groups][n_ridge]: +inf where status_in is not 0 or the sum is not finite
 *   choice     [n_groups] int32
 * Every output element is written in every case.  A group's scores and choice are bitwise the same alone and inside
 * any batch: the summation order is a function of the shape alone and there are no floating-point atomics.
 * Served: n_out <= 8, 1 <= n_ridge <= 16, any cols >= 1, 0 <= transient < T, E and W 16-byte aligned; anything else
 * returns -1 before any HIP call and esn_last_error() names the limit.  Explicit stream, no allocation, no workspace. */
int esn_readout_holdout_score(const double* E, const double* D, const double* W, int n_groups, int T,
                              int transient, int cols, int n_out,
                              const double* t_scale, const double* t_shift,
                              int n_ridge, const int* status_in,
                              double* score, int* choice, void* stream);
int esn_readout_holdout_score_f32(const float* E, const double* D, const double* W, int n_groups, int T,
                                  int transient, int cols, int n_out,
                                  const double* t_scale, const double* t_shift,
                                  int n_ridge, const int* status_in,
                                  double* score, int* choice, void* stream);

/* Running normal equations: the primal form of the ridge fit (an extension, like the ridge solves above: the ABI version
 * is unchanged).  A read-out is kept as
 *     Gm[g] = sum_s gamma^age(s) E_s^T E_s        [cols][cols]   float64, symmetric, both triangles stored
 *     Cm[g] = sum_s gamma^age(s) D_s^T E_s        [n_out][cols]  float64
 * over the training segments s it has seen; its size does not depend on their number.  esn_gram_accumulate adds one
 * segment, rows [transient, T) of E[g]:
 *     D_s   = D[g] * t_scale[g] + t_shift[g]                                (NULL scale / shift: 1 / 0)
 *     Gm[g] = decay * Gm[g] + E^T E,      Cm[g] = decay * Cm[g] + D_s^T E
 *   E      [n_groups][T][cols], float64 (or float32 for the _f32 twin: what esn_harvest_batch_f32 writes)
 *   D      [n_groups][T][n_out], unscaled
 *   decay  in [0, 1]: the forgetting factor gamma.  decay == 0 starts a new sum and does not read Gm / Cm, which may
 *          hold anything (NaN included).
 * Gm is symmetric bit for bit, and a group's result is bitwise the same alone and inside any batch: the summation order
 * is a function of the shape alone and there are no floating-point atomics.
 * esn_gram_solve solves, for every group and each of its n_ridge lambdas (ridge [n_groups][n_ridge], absolute, >= 0),
 *     (Gm[g] + lambda I) W^T = Cm[g]^T
 * by blocked Cholesky -- the ridge solution of the stacked (weighted) rows.  Gm and Cm are only read.
 *   W_out   [n_groups][n_ridge][n_out][cols], in the units esn_pack_readout takes
 *   status  [n_groups][n_ridge]: 0; 1 where a pivot was <= 1e-14 * the largest diagonal entry of Gm + lambda I (that
 *           entry's W_out is zero, the group's other candidates are unaffected); 2 for a negative or non-finite lambda
 *           (W_out zero)
 *   workspace: esn_gram_solve_workspace_bytes(n_groups, n_ridge, cols) bytes, 16-byte aligned: ONE factor per group --
 *           the candidates of a group are factorised one after the other -- so the size does not grow with n_ridge.
 * Served: 1 <= cols <= 544, 1 <= n_out <= 16, 1 <= n_ridge <= 16, 0 <= transient < T, E 16-byte aligned.  cols > 544
 * returns -2 and esn_last_error() names the limit; anything else invalid returns -1; both before any HIP call.
 * Explicit stream, no allocation. */
int esn_gram_accumulate(const double* E, const double* D, int n_groups, int T, int transient, int cols, int n_out,
                        const double* t_scale, const double* t_shift, double decay,
                        double* Gm, double* Cm, void* stream);
int esn_gram_accumulate_f32(const float* E, const double* D, int n_groups, int T, int transient, int cols, int n_out,
                            const double* t_scale, const double* t_shift, double decay,
                            double* Gm, double* Cm, void* stream);
size_t esn_gram_solve_workspace_bytes(int n_groups, int n_ridge, int cols);
int esn_gram_solve(const double* Gm, const double* Cm, int n_groups, int cols, int n_out,
                   const double* ridge, int n_ridge, double* W_out, int* status,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Reservoirs drawn on the device (an extension: the reference draws them on the host, pyESN.py:93-109, once per
 * coherence block).  All float64, device pointers, explicit stream, no allocation; every check returns -1 before any
 * HIP call and esn_last_error() names the function and the limit.  These are additions: the ABI version is unchanged.
 *
 * esn_gen_reservoirs  the sets with global index first_set .. first_set + n_sets - 1, UNSCALED:
 *     W [n_sets][n_res][n_res] = u - 0.5, zero where a second uniform < sparsity;
 *     W_in [n_sets][n_res][n_in] = 2u - 1;  W_fb [n_sets][n_res][n_out] = 2u - 1.
 *   The set with global index s is written to slot s % n_sets: the recurrence kernels pick weight set
 *   (group_offset + g) % n_wsets, so a chunk of blocks [b0, b0 + n) generated with first_set = b0, n_sets = n is
 *   aligned with group_offset = b0.
 *   uniforms == NULL: Philox4x32-10 keyed by (seed, global set, purpose, element) -- set s is the same bits in any
 *   batch, chunk or rank.  uniforms != NULL: [n_sets][2 n_res^2 + n_res n_in + n_res n_out] values in [0, 1), the i-th
 *   row for set first_set + i, in the reference's draw order rand(n,n), mask rand(n,n), rand(n,n_in), rand(n,n_out);
 *   the results are then bitwise the NumPy expressions on those values.
 *   0 <= sparsity <= 1; n_res, n_in, n_out <= 4096.
 *
 * esn_spectral_radius_batch  radius[s] of W [n_sets][n_res][n_res] by repeated squaring, |.| the Frobenius norm:
 *     f_0 = |W|, A_0 = W / f_0, l_0 = ln f_0
 *     k = 1..K:  B = A_{k-1} A_{k-1};  f_k = |B|;  l_k = 2 l_{k-1} + ln f_k;  A_k = B / f_k
 *     radius = exp((l_{K-1} + ln f_K) / 2^(K-1))
 *   K = n_squarings in 4..32 (24: within 1e-7 relative of max|eig| on the reference's matrices).  status[s] = 1 and
 *   radius[s] = 0 when some f_k is zero or not finite (a zero or nilpotent W); the other matrices are unaffected.  The
 *   sums run in an order fixed by n_res alone: a matrix's radius is bitwise the same alone and inside any batch.
 *   The workspace (esn_spectral_radius_workspace_bytes, 8-byte aligned) holds two zero-padded images per matrix; the
 *   query answers 0 for n_sets <= 0, n_res <= 0 or n_res > 4096 (the last with the limit in esn_last_error()).
 *
 * esn_spectral_radius_split_batch  the same recurrence, ratio form, arguments, checks, status and batch invariance, with
 *   every squaring on the fp16 matrix pipe: X = s B (s a power of two fixed by n_res alone, |B| <= 1) is split into
 *   hi = fp16(X) and lo = fp16((X - hi) 2^11), and X X ~ hi hi + 2^-11 (hi lo + lo hi) is three products accumulated
 *   in float32; the norms f_k stay float64.  Within 1e-6 relative of esn_spectral_radius_batch at the same K on the
 *   reference's matrices (the two pieces carry 22 bits).  A matrix whose powers fall below the fp16 range may be
 *   flagged (status 1) where esn_spectral_radius_batch would still measure it.  Its workspace
 *   (esn_spectral_radius_split_workspace_bytes, 8-byte aligned) holds two images per matrix in both orientations as
 *   fp16 hi / lo planes: the bytes of the float64 path's two images.
 *
 * esn_scale_reservoirs  W[s] *= rho / radius[s] where status[s] == 0; a flagged set is left as it is. */
int esn_gen_reservoirs(int n_res, int n_in, int n_out, double sparsity, uint64_t seed, uint64_t first_set, int n_sets,
                       const double* uniforms, double* W, double* W_in, double* W_fb, void* stream);
size_t esn_spectral_radius_workspace_bytes(int n_sets, int n_res);
int esn_spectral_radius_batch(const double* W, int n_sets, int n_res, int n_squarings, double* radius, int* status,
                              void* workspace, size_t workspace_bytes, void* stream);
size_t esn_spectral_radius_split_workspace_bytes(int n_sets, int n_res);
int esn_spectral_radius_split_batch(const double* W, int n_sets, int n_res, int n_squarings, double* radius,
                                    int* status, void* workspace, size_t workspace_bytes, void* stream);
int esn_scale_reservoirs(double* W, int n_sets, int n_res, double rho, const double* radius, const int* status,
                         void* stream);

/* Fused detector tail: Y [B][N][2 N_t] time-domain ESN outputs
 * -> (1/N) FFT_N / sqrt(Pi[group]) -> nearest unit-power square-QAM point ->
 * natural-binary LSB-first bits -> compare with tx_bits [B][N*m][N_t] (uint8) ->
 * err_count[group] += mismatches, bit_count[group] += N*m*N_t  (int64, device).
 * X_hat (complex128 [B][N][N_t] as float64 pairs) is optional (NULL to skip). */
int esn_detect_count(const double* Y, int n_frames, int frames_per_group,
                     int n_sub, int n_t, int bits_per_sym,
                     const double* p_i, const uint8_t* tx_bits,
                     long long* err_count, long long* bit_count,
                     double* X_hat, void* stream);
/* Same with Y float [B][N][2 N_t] (8-byte aligned), as esn_predict_batch_f32 writes it: widened to double on load,
 * then the float64 FFT and slicer of esn_detect_count -- counts and X_hat (still float64) are bitwise those of
 * esn_detect_count on the widened Y.  Checks (-1) before any HIP call, as above. */
int esn_detect_count_f32(const float* Y, int n_frames, int frames_per_group,
                         int n_sub, int n_t, int bits_per_sym,
                         const double* p_i, const uint8_t* tx_bits,
                         long long* err_count, long long* bit_count,
                         double* X_hat, void* stream);

/* Ensemble tail (extension: K independently drawn reservoirs per coherence block, each with its own read-out fitted on
 * the block's pilot; their time-domain outputs are combined and the tail of esn_detect_count runs once).
 *   Y        [K][B][N][2 N_t], member-major: slab k is what member k's esn_predict_batch wrote; 16-byte aligned
 *            (8-byte for the float entry point, whose members are widened to double first)
 *   weights  [groups][K] float64, or NULL: 1 / K each
 *   acc = weights[g][0] y_0, then acc = acc + weights[g][k] y_k for k = 1 .. K-1 in this order, per element, every
 *   product and every sum rounded on its own (no contraction): float64 NumPy reproduces acc bit for bit.  acc then
 *   goes through the transform, scale, slicer and counters of esn_detect_count -- one FFT per frame and antenna whatever
 *   K is -- so err_count, bit_count and X_hat are bitwise those of esn_detect_count on the combined Y, and with K = 1
 *   and NULL weights (1.0 y = y) those of esn_detect_count / esn_detect_count_f32 on the slab.
 *   member_err  optional [groups][K] int64, accumulated like err_count: member k's own error count, that of
 *            esn_detect_count on slab k alone.  Each member is then transformed and sliced as well (K + 1 transforms
 *            per frame and antenna, each slab still read once); when NULL no extra transform is issued.
 * Served: K in [1, 16], N a power of two in [2, 2048], N_t <= 16, m even in [2, 10]; anything else, a null Y, p_i,
 * tx_bits or counter, or a misaligned Y returns -1 before any HIP call, the reason in esn_last_error().  There is no
 * fixed-shape instance and no esn_*_mem front end. */
int esn_detect_count_ens(const double* Y, int n_members, int n_frames, int frames_per_group,
                         int n_sub, int n_t, int bits_per_sym,
                         const double* p_i, const double* weights, const uint8_t* tx_bits,
                         long long* err_count, long long* bit_count, long long* member_err,
                         double* X_hat, void* stream);
int esn_detect_count_ens_f32(const float* Y, int n_members, int n_frames, int frames_per_group,
                             int n_sub, int n_t, int bits_per_sym,
                             const double* p_i, const double* weights, const uint8_t* tx_bits,
                             long long* err_count, long long* bit_count, long long* member_err,
                             double* X_hat, void* stream);

/* Decide and re-modulate (extension: decision-directed tracking of the read-out).  The tail of esn_detect_count --
 * err_count, bit_count and X_hat are bitwise those of esn_detect_count on the same Y -- and then, in the same launch
 * (the spectrum never leaves the chip), the decisions back in the time domain as the teacher of a re-fit:
 *   X_dec = the constellation point of the decided index;  x_t = N IFFT_N(X_dec) sqrt(Pi[group]);
 *   D_hat [B][delay + cp + N][2 N_t]: rows [0, delay) zero, rows [delay, delay + cp) the last cp samples of x_t, rows
 *   [delay + cp, delay + cp + N) x_t; Re/Im interleaved per antenna -- the teacher layout of esn_harvest_batch
 *   (helper_mimo_esn_generic.py:26-38).  Every element is written.
 * tx_bits may be NULL: nothing is counted and err_count / bit_count (may be NULL too) are not touched.  dec_bits
 * (uint8 [B][N*m][N_t], the decided bits in the layout of tx_bits) and X_hat are optional.  A frame's outputs do not
 * depend on what else is in the launch.  Served: N a power of two in [2, 2048], N_t <= 16, m even in [2, 10],
 * 0 <= cp < N, 0 <= delay <= 2^20; anything else returns -1 before any HIP call, the limit in esn_last_error(). */
int esn_detect_remod(const double* Y, int n_frames, int frames_per_group,
                     int n_sub, int cp, int delay, int n_t, int bits_per_sym,
                     const double* p_i, const uint8_t* tx_bits,
                     long long* err_count, long long* bit_count,
                     double* X_hat, uint8_t* dec_bits, double* D_hat, void* stream);

/* ---- Host-memory front ends ("caller-owned device or host pointers flagged by an enum").
 * The reference's callers hold C-contiguous float64 NumPy arrays on the host (pyESN.py:154,218); a binding that
 * lives there passes them as they are with ESN_MEM_HOST.  Each `esn_X_mem(mem_kind, ...)` takes the arguments
 * of `esn_X(...)`:
 *   ESN_MEM_DEVICE  forwards to esn_X unchanged (asynchronous on `stream`, no allocation).
 *   ESN_MEM_HOST    every ARRAY argument (weights, scalings, U, D, x0, y0, noise_u, Y, E, W_out, status, p_i,
 *                   tx_bits, counters, X_hat) is host memory: the call stages it in device memory from the
 *                   stream-ordered pool, runs esn_X on `stream`, copies the results back and returns after
 *                   the stream has drained, so the host arrays are complete on return.  The counters of
 *                   esn_detect_count_mem are read, added to and written back.
 * `packed` images and `workspace` are device memory in both kinds -- esn_device_alloc / esn_device_free hand
 * them to a caller that has no HIP toolchain of its own (sizes from esn_packed_*_bytes / esn_*_workspace_bytes;
 * esn_readout_solve_batch_mem takes its scratch from the pool when `workspace` is NULL).
 * Returns as esn_X; -1 for an unknown mem_kind. */
enum esn_mem_kind {
    ESN_MEM_DEVICE = 0,
    ESN_MEM_HOST = 1
};
void* esn_device_alloc(size_t bytes);   /* NULL on failure (esn_last_error()) */
int esn_device_free(void* p);
int esn_pack_weights_mem(int mem_kind, int precision, const esn_shape_t* shape,
                         const double* W, const double* W_in, const double* W_fb,
                         void* packed, void* stream);
int esn_pack_readout_mem(int mem_kind, int precision, const esn_shape_t* shape, int n_groups,
                         const double* W_out, void* packed, void* stream);
int esn_predict_batch_mem(int mem_kind, int precision, const esn_shape_t* shape,
                          const void* packed_w, const void* packed_wout,
                          const double* in_scale, const double* in_shift,
                          const double* t_scale, const double* t_shift,
                          const double* U, int n_frames, int frames_per_group,
                          int T_in, int T, int transient,
                          const double* x0, const double* y0,
                          double noise, int noise_mode, const double* noise_u,
                          uint64_t seed, uint64_t group_offset,
                          double* Y, void* workspace, size_t workspace_bytes, void* stream);
int esn_harvest_batch_mem(int mem_kind, int precision, const esn_shape_t* shape,
                          const void* packed_w,
                          const double* in_scale, const double* in_shift,
                          const double* t_scale, const double* t_shift,
                          const double* U, const double* D, int n_groups, int T,
                          double noise, int noise_mode, const double* noise_u,
                          uint64_t seed, uint64_t group_offset, double* E,
                          void* workspace, size_t workspace_bytes, void* stream);
int esn_readout_solve_batch_mem(int mem_kind, const double* E, const double* D, int n_groups, int T,
                                int transient, int cols, int n_out,
                                const double* t_scale, const double* t_shift,
                                double* W_out, int* status, void* workspace, void* stream);
int esn_detect_count_mem(int mem_kind, const double* Y, int n_frames, int frames_per_group,
                         int n_sub, int n_t, int bits_per_sym,
                         const double* p_i, const uint8_t* tx_bits,
                         long long* err_count, long long* bit_count,
                         double* X_hat, void* stream);

/* ---- Monte-Carlo frame generator: the producer directly upstream of the detector.
 * float64 / complex128 like the reference; counter-based random streams keyed by
 * (seed, global frame / link index), so a frame is identical on any rank and launch shape.
 * Each random input may instead be supplied (bits_in, noise_in, gains_in = standard normals):
 * the deterministic mode the parity tests use.
 *
 * esn_gen_taps   per-link impulse responses [n_blocks][n_r][n_t][isi] complex128:
 *                kind 0 TDL-B (Demo_MIMO_4x8_Sionna_CDL_ESN_v2.py:127-177: 23 paths, delays
 *                tau*DS*fs split linearly between floor/ceil taps, CN(0,p) gains, unit energy),
 *                kind 1 exponential-PDP Rayleigh (OFDM_MIMO_2-2_NBF_LDPC.py:162-164,272-279),
 *                kind 2 flat unit-modulus (Demo_SISO_QPSK_AWGN_LDPC_ESN_with_ZF_LS.py:205-206).
 * esn_gen_frames bits -> 2^m-QAM (:406-411) -> N*ifft (:416) -> CP (:417) -> sqrt(Pi) -> PA (:419)
 *                -> per-link FIR with zero initial state (:422-425) -> AWGN sqrt(T No/2) (:426).
 *                p_i / a_clip are per block [n_blocks]; x_cp (pre-PA teacher) may be NULL.
 *                ls_pattern = 1 keeps only tx = sc % n_t on subcarrier sc (the sparse LS pilot of
 *                :330-333); with the pilot's seed / frame index it shares the pilot's bits AND noise
 *                (:354-356), as the reference does.
 * esn_gen_taps_doppler  (extension) the taps of esn_gen_taps kinds 0 and 1 moving INSIDE a coherence block: complex128
 *                [n_blocks][n_sym][n_r][n_t][isi], one tap set per OFDM symbol s = 0 .. n_sym - 1.  Clarke / Jakes
 *                sum of sinusoids: path p of link l = (block, rx, tx) is
 *                    g(s) = sqrt(P_p / M) sum_{m<M} exp(j pi (2 fd_tsym s cos(pi a_m) + phi_m)),  M = ESN_DOPPLER_SINUSOIDS,
 *                a and phi uniform on [0, 2) half-turns from Philox (key = seed, counter = (global link lo, hi, 4,
 *                p M + m), words 0 and 1, (w + 0.5) / 2^31), or supplied as angles_in [n_links][n_paths][M][2]
 *                = (a, phi) (n_paths = 23 for kind 0, isi for kind 1).  Paths, powers and delays are those of
 *                esn_gen_taps; kind 0's unit-energy factor is computed at s = 0 and applied to the whole block.
 *                fd_tsym = f_d T_sym in cycles per symbol, 0 .. 0.5; the ensemble autocorrelation of a path is
 *                P_p J0(2 pi fd_tsym s).  The phasors are seeded exactly at s = 0 and advanced by one complex
 *                multiplication per symbol, always from s = 0: symbol s is a function of (seed, global link, s), and
 *                with fd_tsym = 0 all symbols are bitwise equal.  The marginal is Gaussian up to a kurtosis of 2 - 1/M,
 *                so fd_tsym = 0 is the block channel of esn_gen_taps statistically, not bitwise.  Viewed as
 *                [n_blocks * n_sym][n_r][n_t][isi] the output is the `taps` of esn_gen_frames / esn_taps_to_freq
 *                with frames_per_block = 1.  Device pointers only.  -1: null taps, kind outside {0, 1}, n_blocks,
 *                n_r or n_t <= 0, n_sym outside 1 .. 4096, isi outside 1 .. 16, fd_tsym negative, not finite or above 0.5
 *                (more than half a cycle per symbol aliases). */
#define ESN_DOPPLER_SINUSOIDS 16
int esn_gen_taps_doppler(int kind, int n_blocks, int n_sym, int n_r, int n_t, int isi,
                         double fs_hz, double ds_ns, double fd_tsym,
                         const double* angles_in, uint64_t seed, uint64_t link_offset,
                         double* taps, void* stream);
int esn_gen_taps(int kind, int n_blocks, int n_r, int n_t, int isi, double fs_hz, double ds_ns,
                 const double* gains_in, uint64_t seed, uint64_t link_offset,
                 double* taps, void* stream);
int esn_gen_frames(int n_frames, int frames_per_block, int n_sub, int cp, int n_t, int n_r, int isi,
                   int bits_per_sym, int ls_pattern, const double* p_i, const double* a_clip, double no,
                   const double* taps, const uint8_t* bits_in, const double* noise_in,
                   uint64_t seed, uint64_t frame_offset,
                   uint8_t* bits, double* x_cp, double* y_cp, void* stream);
/* esn_gen_frames with complex64 outputs: x_cp (optional) and y_cp as float pairs [B][T][n] (8-byte aligned; a 16-byte
 * aligned y_cp with even n_r is written one antenna pair per 16-byte store).  The arithmetic stays float64 and only
 * the store rounds: bits are equal and x_cp / y_cp are bitwise the complex128 outputs of esn_gen_frames rounded to
 * complex64, for the same seed and frame_offset, for supplied bits_in / noise_in and for ls_pattern = 1. */
int esn_gen_frames_c64(int n_frames, int frames_per_block, int n_sub, int cp, int n_t, int n_r, int isi,
                       int bits_per_sym, int ls_pattern, const double* p_i, const double* a_clip, double no,
                       const double* taps, const uint8_t* bits_in, const double* noise_in,
                       uint64_t seed, uint64_t frame_offset,
                       uint8_t* bits, float* x_cp, float* y_cp, void* stream);

/* ---- Baseline equaliser the reference compares the ESN with, float64.
 * esn_channel_estimate   pilot_bits [G][N*m][n_t], y_ls_cp complex [G][T][n_r] (received sparse LS
 *                        pilot) -> H complex [G][N][n_r][n_t]: LS at sc = tx + n_t i, linear
 *                        inter/extrapolation, IFFT -> isi taps, diagonal MMSE shrinkage, DFT
 *                        (Demo_MIMO_4x8_Sionna_CDL_ESN_v2.py:358-382); ls_only = 1 stops at the interpolated LS
 *                        estimate, the H_LS the block-fading drivers feed their LS-ZF detector
 *                        (OFDM_MIMO_2-2_NBF_LDPC.py:321-333,457).  isi <= 64 and N / n_t >= 2, else -1; one workgroup
 *                        holds 16 (2N + N/n_t + 1 + isi + N/2) bytes of LDS (90,256 at N = 2048, n_t = 4, isi = 8): a
 *                        shape beyond the 150 KiB served is -2 with the byte count in esn_last_error().
 * esn_mmse_detect_count  y_cp complex [B][T][n_r] -> X = (H^H H + No/Pi I)^-1 H^H Y / sqrt(Pi) per
 *                        subcarrier (:40-45, :444-448), hard decision + error count as in
 *                        esn_detect_count; n_t <= 4.  X_hat complex [B][N][n_t] optional.
 * esn_zf_detect_count    the same with G = H^H H + 1e-12 I: equalize_zf (:34-39; OFDM_MIMO_2-2_NBF_LDPC.py:41-47),
 *                        "LS-ZF" with an estimated H and "Perfect-ZF" with the true one (:450-460).
 * esn_taps_to_freq       taps complex [G][n_r][n_t][isi] -> the true channel H complex [G][N][n_r][n_t]
 *                        = FFT_N of the zero-padded impulse response (H_true, OFDM_MIMO_2-2_NBF_LDPC.py:273-279). */
int esn_channel_estimate(int n_blocks, int n_sub, int cp, int n_t, int n_r, int isi, int bits_per_sym,
                         const double* p_i, double no, const uint8_t* pilot_bits,
                         const double* y_ls_cp, int ls_only, double* H, void* stream);
int esn_mmse_detect_count(int n_frames, int frames_per_group, int n_sub, int cp, int n_t, int n_r,
                          int bits_per_sym, const double* p_i, double no, const double* H,
                          const double* y_cp, const uint8_t* tx_bits,
                          long long* err_count, long long* bit_count, double* X_hat, void* stream);
int esn_zf_detect_count(int n_frames, int frames_per_group, int n_sub, int cp, int n_t, int n_r,
                        int bits_per_sym, const double* p_i, const double* H,
                        const double* y_cp, const uint8_t* tx_bits,
                        long long* err_count, long long* bit_count, double* X_hat, void* stream);
int esn_taps_to_freq(int n_blocks, int n_sub, int n_t, int n_r, int isi, const double* taps, double* H, void* stream);

/* ---- The equaliser's output back in the time domain (extension: the input rows of an ESN that stands behind the
 * LS-MMSE equaliser), float64.  Frame f belongs to group g = f / frames_per_group (p_i [groups], H [groups]):
 *   Y_k[rx] = (1/N) sum_i y[cp + i][rx] e^{-2 pi i ik/N}              y_cp complex [B][cp + N][n_r]
 *   X_k     = (H_k^H H_k + (no / Pi_g) I)^-1 H_k^H Y_k / sqrt(Pi_g)   the operations and order of esn_mmse_detect_count:
 *             X_hat (optional, complex [B][N][n_t]) is bitwise what that entry point writes for the same inputs
 *   z_i[tx] = sqrt(Pi_g) sum_k X_k[tx] e^{+2 pi i ik/N}               (N IFFT_N and the scaling of esn_detect_remod)
 *   U_eq [B][cp + N + pad][2 n_t]: rows [0, cp) the last cp samples of z, rows [cp, cp + N) z, rows [cp + N, cp + N + pad)
 *   zero; Re/Im interleaved per antenna -- the input layout of esn_predict_batch / esn_harvest_batch at n_in = 2 n_t.
 * Every element is written; no counters, no atomics; a frame's outputs do not depend on what else is in the launch.
 * The _f32 entry point writes the float64 value rounded to float32.  One workgroup per frame holds
 * 16 (max(n_r, n_t) N + N/2) bytes of LDS (the Y image, which X then replaces, and the twiddle table), at most 150 KiB:
 * n_r <= 74 at N = 128, n_r <= 4 at N = 2048.  Served: N a power of two in [2, 2048], n_t <= 4, 0 <= cp < N,
 * 0 <= pad <= 2^20, n_r within that LDS, U_eq 16-byte (float32: 8-byte) aligned; anything else returns -1 before any HIP
 * call, the limit in esn_last_error(). */
int esn_mmse_equalize_rows(int n_frames, int frames_per_group, int n_sub, int cp, int pad, int n_t, int n_r,
                           const double* p_i, double no, const double* H, const double* y_cp,
                           double* U_eq, double* X_hat, void* stream);
int esn_mmse_equalize_rows_f32(int n_frames, int frames_per_group, int n_sub, int cp, int pad, int n_t, int n_r,
                               const double* p_i, double no, const double* H, const double* y_cp,
                               float* U_eq, double* X_hat, void* stream);

/* ---- Amplifier-aware LS-MMSE (extension: a classical baseline that knows the transmit amplifier), float64.  The frame
 * recipe passes x through x / sqrt(1 + (|x|/A)^2), A = a_clip; this detector slices, re-modulates, passes its decisions
 * through that amplifier and subtracts the distortion it predicts, n_iter times, inside one launch.  Frame f belongs to
 * group g = f / frames_per_group (p_i, a_clip [groups], H [groups]); lam = no / Pi_g, A = a_clip[g], side = 2^(m/2):
 *   Y_k, X0_k   exactly as esn_mmse_detect_count: X0 is bitwise its X_hat
 *   for it = 1 .. n_iter:
 *     S_k[tx]  = the grid point nearest X^{it-1}_k[tx] (slicer and levels of esn_detect_count)
 *     xt_i[tx] = sqrt(Pi_g) sum_k S_k[tx] e^{+2 pi i ik/N}, i < N (no prefix)
 *     d_i[tx]  = xt_i / sqrt(1 + (|xt_i|/A)^2) - xt_i
 *     D_k[tx]  = (1 / (N sqrt(Pi_g))) sum_i d_i[tx] e^{-2 pi i ik/N}
 *     X^it_k   = X0_k - (H_k^H H_k + lam I)^-1 H_k^H (H_k D_k)
 *   slicer, bit errors and counters of esn_mmse_detect_count on X^{n_iter}: n_iter = 0 is that entry point bit for bit,
 *   counters and X_hat.  X_hat (optional, complex [B][N][n_t]) is X^{n_iter}.
 * err_iter (optional, [groups][n_iter + 1], added to like err_count) takes the bit errors of X^0 .. X^{n_iter}, from the
 * slicer passes the loop makes anyway.  tx_bits may be NULL: then no counter is touched (err_count, bit_count and err_iter
 * may be NULL too) and X_hat must be given.  Every sum runs in an order the shape alone decides: a frame's X_hat and error
 * counts are bitwise the same alone and in any batch.  One workgroup per frame holds esn_mmse_dcc_lds_bytes(N, n_t, n_r) =
 * 16 ((n_r + 2 n_t) N + N/2) bytes of LDS (Y / H D, X0, the work rows, the twiddle table): 33,792 at N = 128 and 4x8,
 * 135,168 at N = 512 and 4x8.  Served: N a power of two in [2, 2048], 1 <= n_t <= 4, n_r >= 1, 0 <= cp < N,
 * 0 <= n_iter <= 8, even bits_per_sym in [2, 10], LDS within 150 KiB; anything else returns -1 before any HIP call, the
 * argument named in esn_last_error().  a_clip lives in device memory and is not read by the host: its entries must be
 * finite and positive (a huge A switches the correction off: d = 0). */
size_t esn_mmse_dcc_lds_bytes(int n_sub, int n_t, int n_r);
int esn_mmse_dcc_detect_count(int n_frames, int frames_per_group, int n_sub, int cp, int n_t, int n_r,
                              int bits_per_sym, int n_iter, const double* p_i, const double* a_clip, double no,
                              const double* H, const double* y_cp, const uint8_t* tx_bits,
                              long long* err_count, long long* bit_count, long long* err_iter, double* X_hat,
                              void* stream);

/* ---- Decision-directed channel estimate (extension: the MMSE baseline tracked through a block under Doppler), float64.
 * Estimate e is made from `window` frames stored consecutively, frames e window .. e window + window - 1, and belongs to
 * group e / est_per_group (p_i [groups], reg [groups][isi]).  With w = exp(-2 pi i / N), L = isi, Pi = p_i[group]:
 *   Y_f[k, r] = (1/N) FFT_N(y_f[cp:, r])[k] / sqrt(Pi)               y_cp complex [n_est window][cp + N][n_r]
 *   X_f[k, t] = the unit-power square QAM point decided for (k, t): the nearest point to X_hat complex
 *               [n_est window][N][n_t] (slicer and index rule of esn_detect_count), or the point of `bits`
 *               [n_est window][N*m][n_t] (layout of tx_bits: natural binary, LSB first) -- exactly one of the two.
 *   model       Y_f[k, r] ~ sum_t X_f[k, t] sum_{l<L} c[r, t, l] w^{kl}
 *   G[(t,l),(t',l')] = sum_f sum_k conj(X_f[k,t]) X_f[k,t'] w^{k(l'-l)} + delta reg[l]   (block-Toeplitz: computed as
 *                      n_t^2 L lag sums), b[(t,l), r] = sum_f sum_k conj(X_f[k,t]) w^{-kl} Y_f[k,r]
 *   c[r] = G^-1 b[:, r] by root-free Cholesky (G = L D L^H);   H[k, r, t] = sum_l c[r,t,l] w^{kl}
 * reg[l] >= 0 is the caller's prior weight: the MAP weight of a tap of variance r_h[l] under noise of variance
 * T No / (N Pi) on Y is reg[l] = T No / (N Pi r_h[l]), T = N + cp.  Outputs: H complex [n_est][N][n_r][n_t], taps
 * complex [n_est][n_r][n_t][isi] (optional), status [n_est].  A pivot D_j that is not finite or not above 64 2^-52 times
 * its original diagonal entry sets status[e] = 1 and that estimate's taps and H to NaN; otherwise status[e] = 0.  Every
 * output element is written in every case.  Sums run in a fixed order (frame after frame, k ascending inside one of S
 * contiguous ranges of k, the ranges joined pairwise, S a function of the shape), so an estimate is bitwise the same
 * alone or inside any launch.  Served: N a power of two in [2, 2048], n_t <= 4, n_r <= 8, isi <= 16, n_t isi <=
 * min(64, N), 1 <= window <= 8, 0 <= cp < N, m even in [2, 10], 16-byte aligned y_cp / X_hat / taps / H, and a workgroup
 * image of at most 150 KB of LDS (16 (N (1 + n_r + n_t) + n_r) bytes plus the solver's: up to N = 512 at 4x8 with
 * isi = 8, up to N = 2048 at 2x2 -- wider than the N the detector's other limits suggest, since LDS allows it); anything
 * else returns -1 before any HIP call, the limit in esn_last_error(). */
int esn_channel_track(const double* y_cp, const double* X_hat, const uint8_t* bits,
                      int n_est, int window, int est_per_group,
                      int n_sub, int cp, int n_t, int n_r, int isi, int bits_per_sym,
                      const double* p_i, const double* reg,
                      double* taps, double* H, int* status, void* stream);

/* ---- Windowed ELM (extension of the batched kind; the reference's pinv-trained comparator: class ELM,
 * system_model_2_all_comparision.py:51-69, windowed as trainMIMOModel('ELM') does, :115-127, :147-149, :551-575): a random
 * tanh layer over the last `window` input rows, a bias column, a linear read-out.  With w = window, K = w n_in, frame (or
 * training sequence) b in group g = b / frames_per_group (features: g = b) and weight set s = (group_offset + g) % n_wsets:
 *   us[t][i]  = U[b][t][i] in_scale[g][i] + in_shift[g][i]     0 <= t < T_in      (NULL scale / shift: 1 / 0)
 *             = in_shift[g][i]                                 T_in <= t < T      (zero rows BEFORE scaling, as
 *                                                                                  esn_predict_batch)
 *   pre[t][h] = b[s][h] + sum_{k<w} sum_{i<n_in} W_in[s][h][k n_in + i] us[t-(w-1)+k][i]                     t >= w-1
 *   row[t]    = [ tanh(pre[t][0..n_hidden)) | 1.0 if bias_col | 0.0 up to e_cols ]                           t >= w-1
 *             = all zeros (the bias column too)                                                              t <  w-1
 *   Ys[t][o]  = sum_c W_out[g][o][c] row[t][c]
 *   Y[b][t-transient][o] = (Ys[t][o] - t_shift[g][o]) / t_scale[g][o]    t >= max(transient, w-1);
 *                          exactly 0.0 for transient <= t < w-1
 * The flat window index k n_in + i with k = 0 the oldest sample is ESN_input[j:j+w].flatten() (:118-120); only whole
 * windows give a row (:117) and the rows before them are the reference's x_hat_temp[:window-1] = 0 (:147-148).
 * W_in [n_wsets][n_hidden][K], b [n_wsets][n_hidden], W_out [groups][n_out][e_cols], scalings [groups][n], all float64
 * on the device.  e_cols >= n_hidden + bias_col: the extra columns of E are written as zeros (a read-out solve takes its
 * 16-byte path when cols % 4 == 0, float32 E, or cols % 2 == 0, float64 E; a zero column takes zero weight in the
 * minimum-norm and ridge solutions) and the extra columns of W_out are not read.
 * esn_elm_features  the fit side, one sequence per group: E [n_groups][T][e_cols], float64 or (e_f32) the float64 value
 *                   rounded to float32 -- what the read-out solves take.  ESN_F64 only (ESN_F16: -2).
 * esn_elm_predict   fused: the hidden rows never reach memory.  ESN_F64: plain FMA, every sum in an order that depends on
 *                   the shape alone, so a frame is bitwise the same alone and inside any batch.  ESN_F16:
 *                   v_mfma_f32_16x16x32_f16 with W_in, us, the hidden rows and W_out rounded to fp16 (from the float64
 *                   arrays, at load: there is no packed image), float32 accumulators, bias add and tanh, and the
 *                   un-scaling as a multiplication by 1 / t_scale in float64.
 * ESN_F32 / ESN_BF16 return -2.  Served: 1 <= n_in, 1 <= window <= 16, K <= 256, 1 <= n_hidden <= 1024, n_out <= 8,
 * bias_col 0 or 1, n_hidden + bias_col <= e_cols <= n_hidden + 4, 1 <= T_in <= T <= 2^20, window <= T,
 * 0 <= transient < T, fewer than 2^31 tiles of 16 rows, E / Y 16-byte aligned; anything else returns -1 before any HIP
 * call, the limit in esn_last_error().  There is no float32 I/O variant and no _mem front end.  These are additions: the
 * ABI version is unchanged. */
int esn_elm_features(int precision, int n_in, int n_hidden, int window, int bias_col, int n_wsets,
                     const double* W_in, const double* b, const double* in_scale, const double* in_shift,
                     const double* U, int n_groups, int T_in, int T, uint64_t group_offset,
                     void* E, int e_f32, int e_cols, void* stream);
int esn_elm_predict(int precision, int n_in, int n_hidden, int window, int bias_col, int n_wsets, int n_out,
                    const double* W_in, const double* b, const double* W_out, int e_cols,
                    const double* in_scale, const double* in_shift, const double* t_scale, const double* t_shift,
                    const double* U, int n_frames, int frames_per_group, int T_in, int T, int transient,
                    uint64_t group_offset, double* Y, void* stream);

/* ---- Windowed FNN (the reference's second learned comparator: class FNNModel, system_model_2_all_comparision.py:40-49,
 * trained as trainMIMOModel('FNN') does, :115-122, :129-149): the ELM's window of scaled input rows feeding
 * Linear -> ReLU -> Linear, trained per group by `epochs` full-batch Adam steps on the mean squared error.  Notation as in
 * the ELM block: w = window, K = w n_in, group g, us[t][i] the scaled input with the zero rows before scaling for
 * T_in <= t < T, and x[t][k n_in + i] = us[t-(w-1)+k][i] for t >= w-1.  With the trained rows
 * R = { t : max(transient, w-1) <= t < T } and Ds[t][o] = D[g][t][o] t_scale[g][o] + t_shift[g][o]:
 *   pre[t][h] = b1[h] + sum_k W1[h][k] x[t][k]         h[t] = max(pre[t], 0)
 *   ys[t][o]  = b2[o] + sum_h W2[o][h] h[t][h]
 *   loss      = sum_{t in R, o} (ys - Ds)^2 / (|R| n_out)                                      (nn.MSELoss, mean)
 *   Adam, epoch e = 1..epochs, for every parameter p with gradient q = dloss/dp (the gradient of ReLU at 0 is 0):
 *     m = beta1 m + (1-beta1) q;   v = beta2 v + (1-beta2) q^2
 *     p -= (lr / (1-beta1^e)) m / ( sqrt(v)/sqrt(1-beta2^e) + eps )       (torch.optim.Adam, no weight decay, no amsgrad)
 * The reference's values: epochs = 50, lr = 0.01, beta1 = 0.9, beta2 = 0.999, eps = 1e-8.  A parameter whose q is exactly 0
 * in every epoch (a hidden unit inactive on every trained row) keeps m = v = 0 and comes out bitwise as it went in.
 * esn_fnn_train   group g starts from the initial set (group_offset + g) % n_isets of W1_0 [n_isets][n_hidden][K],
 *                 b1_0 [n_isets][n_hidden], W2_0 [n_isets][n_out][n_hidden], b2_0 [n_isets][n_out] and writes
 *                 W1 [G][n_hidden][K], b1 [G][n_hidden], W2 [G][n_out][n_hidden], b2 [G][n_out]; loss [G][epochs], the
 *                 loss BEFORE each step, may be NULL.  U [G][T_in][n_in], D [G][T][n_out], scalings [G][n] or NULL.  One
 *                 workgroup per group and one launch for all epochs, the parameters resident in LDS, float64 plain FMA;
 *                 every sum in an order that depends on the shape alone and no atomics, so a group is bitwise the same
 *                 alone and inside any batch.  ESN_F64 only: every other precision returns -2.  workspace: device memory
 *                 of esn_fnn_workspace_bytes(...) bytes (Adam's moments of W1, which do not fit the owning lanes'
 *                 registers beside the gradient sums; 64 ceil(n_hidden / 4) ceil(K / 8) doubles per group), not
 *                 initialised by the caller and of no meaning afterwards.
 *                 Served: the ELM's 1 <= n_in, 1 <= window <= 16, K <= 256, n_out <= 8, T_in <= T, window <= T,
 *                 0 <= transient < T, and what residency of the parameters allows: n_hidden <= 512,
 *                 n_out n_hidden <= 1024, ceil(n_hidden / 4) ceil(K / 8) <= 512 (n_hidden K <= 16384 doubles of W1), and a
 *                 workgroup image 8 (n_hidden (K | 1) + 2 ceil(T n_in / 2) + n_out n_hidden + n_hidden + n_out +
 *                 32 (n_hidden | 1) + 256) bytes of at most 160 KB of LDS -- the reference's 100 units at K = 32 and at
 *                 K = 128 (T = 138, n_out = 8: 156 KB) fit, 64 units at K = 256 too; epochs >= 1, lr >= 0,
 *                 0 <= beta < 1, eps > 0.
 * esn_fnn_predict the ELM's prediction (the same kernels, instantiated with another activation) with three changes:
 *                 max(., 0) for tanh; bias_col = 1 with W_out[g] = [W2[g] | b2[g]]; one weight set per group, so W1, b1,
 *                 W2, b2 are [groups][...] with groups = ceil(n_frames / frames_per_group).  ESN_F64 and ESN_F16 with the
 *                 meaning they have for esn_elm_predict; the fp16 path rounds the ReLU outputs to fp16 -- unlike tanh
 *                 they are unbounded, so inputs are expected scaled to about unit variance.  Served: esn_elm_predict's
 *                 shapes (n_hidden <= 1024).
 * Anything outside the served shapes returns -1 before any HIP call, the limit in esn_last_error().  There is no float32
 * I/O variant and no _mem front end.  These are additions: the ABI version is unchanged. */
size_t esn_fnn_workspace_bytes(int n_in, int n_hidden, int window, int n_out, int n_groups, int T);
int esn_fnn_train(int precision, int n_in, int n_hidden, int window, int n_out, int n_isets,
                  const double* W1_0, const double* b1_0, const double* W2_0, const double* b2_0,
                  const double* in_scale, const double* in_shift, const double* t_scale, const double* t_shift,
                  const double* U, const double* D, int n_groups, int T_in, int T, int transient,
                  uint64_t group_offset, int epochs, double lr, double beta1, double beta2, double eps,
                  double* W1, double* b1, double* W2, double* b2, double* loss,
                  void* workspace, size_t workspace_bytes, void* stream);
int esn_fnn_predict(int precision, int n_in, int n_hidden, int window, int n_out,
                    const double* W1, const double* b1, const double* W2, const double* b2,
                    const double* in_scale, const double* in_shift, const double* t_scale, const double* t_shift,
                    const double* U, int n_frames, int frames_per_group, int T_in, int T, int transient,
                    double* Y, void* stream);

/* ---- Windowed CNN (the reference's third learned comparator: class CNNModel, system_model_2_all_comparision.py:14-27,
 * trained as trainMIMOModel('CNN') does, :93-113): three Conv1d layers over the whole pilot sequence, trained per group
 * by `epochs` full-batch Adam steps on the mean squared error.  Channels c0 = n_in, c1, c2, c3 = n_out; the kernel size k
 * is odd, p = (k - 1) / 2; parameters in torch's Conv1d layout W_l [c_l][c_{l-1}][k], b_l [c_l].  For group g:
 *   x_0[t][i] = u[t][i] in_scale[g][i] + in_shift[g][i]   0 <= t < T, u = 0 for T_in <= t < T (zero rows BEFORE scaling)
 *   z_l[t][o] = b_l[o] + sum_i sum_j W_l[o][i][j] x_{l-1}[t + j - p][i]     x_l = max(z_l, 0), l = 1, 2;   ys = z_3
 *   every x_l (l = 0, 1, 2) exactly 0 outside [0, T): torch's zero padding of each layer's input, not the scaled zero row
 *   loss = sum_{transient <= t < T, o} (ys[t][o] - (D[g][t][o] t_scale[g][o] + t_shift[g][o]))^2 / ((T - transient) n_out)
 *   Adam exactly as in the FNN block above (the gradient of ReLU at 0 is 0), epoch e = 1..epochs; loss[g][e] is the loss
 *   BEFORE step e.  The reference's values: k = 5, c1 = 32, c2 = 64, transient = 0, epochs = 50, lr = 0.01.
 *   predict: Y[f][t - transient][o] = (ys[t][o] - t_shift[g][o]) / t_scale[g][o], g = f / frames_per_group.
 * A parameter whose gradient is exactly 0 in every epoch (a channel that is never active, and the next layer's weights
 * that read it) comes out bitwise as it went in.
 * esn_cnn_train    group g starts from the initial set (group_offset + g) % n_isets of W1_0 .. b3_0 [n_isets][...] and
 *                  writes W1 .. b3 [G][...]; loss [G][epochs] may be NULL; U [G][T_in][n_in], D [G][T][n_out], scalings
 *                  [G][n] or NULL.  One workgroup per group and one launch for all epochs, float64; all three layers'
 *                  forward, input-gradient and weight-gradient products run on v_mfma_f64_16x16x4_f64.  Every sum in an
 *                  order that depends on the shape alone, no atomics, nothing shared between workgroups: a group is
 *                  bitwise the same alone and inside any batch.  ESN_F64 only: every other precision returns -2.
 *                  workspace: device memory of esn_cnn_workspace_bytes(..., n_groups, 0, T) bytes (per group the
 *                  parameters, Adam's moments, the padded activations and their gradients: nothing of this fits on
 *                  chip), not initialised by the caller and of no meaning afterwards.
 * esn_cnn_predict  the same forward functions, a workgroup per frame, the inner activations in that workgroup's part of
 *                  the workspace (esn_cnn_workspace_bytes(..., 0, n_frames, T) bytes: at most 512 parts).  A frame is
 *                  bitwise the same alone and inside any batch.  ESN_F64 only (-2 otherwise): there is no fp16 instance.
 * esn_cnn_workspace_bytes   the larger of what n_groups trainings and what a prediction of n_frames frames need (either
 *                  count may be 0); 0 for an unserved shape.
 * Served: 1 <= n_in <= 64, 1 <= c1, c2 <= 128, 1 <= n_out <= 8, k in {1, 3, 5, 7}, 1 <= T_in <= T <= 4096,
 * 0 <= transient < T (T may be below k), epochs >= 1, lr >= 0, 0 <= beta < 1, eps > 0.  Anything else returns -1 before
 * any HIP call, the limit in esn_last_error().  No float32 I/O variant, no _mem front end, one pilot per group.  These
 * are additions: the ABI version is unchanged. */
size_t esn_cnn_workspace_bytes(int n_in, int c1, int c2, int n_out, int kernel, int n_groups, int n_frames, int T);
int esn_cnn_train(int precision, int n_in, int c1, int c2, int n_out, int kernel, int n_isets,
                  const double* W1_0, const double* b1_0, const double* W2_0, const double* b2_0,
                  const double* W3_0, const double* b3_0,
                  const double* in_scale, const double* in_shift, const double* t_scale, const double* t_shift,
                  const double* U, const double* D, int n_groups, int T_in, int T, int transient,
                  uint64_t group_offset, int epochs, double lr, double beta1, double beta2, double eps,
                  double* W1, double* b1, double* W2, double* b2, double* W3, double* b3, double* loss,
                  void* workspace, size_t workspace_bytes, void* stream);
int esn_cnn_predict(int precision, int n_in, int c1, int c2, int n_out, int kernel,
                    const double* W1, const double* b1, const double* W2, const double* b2,
                    const double* W3, const double* b3,
                    const double* in_scale, const double* in_shift, const double* t_scale, const double* t_shift,
                    const double* U, int n_frames, int frames_per_group, int T_in, int T, int transient,
                    double* Y, void* workspace, size_t workspace_bytes, void* stream);

/* ---- LSTM comparator (the reference's fourth learned comparator, its curve BER_RNN: class RNNModel,
 * system_model_2_all_comparision.py:29-38, trained as trainMIMOModel('RNN') does, :93-113): nn.LSTM(n_in, H, batch_first)
 * followed by nn.Linear(H, n_out) over the whole pilot sequence, trained per group by `epochs` full-batch Adam steps on
 * the mean squared error.  H = n_hidden.  Parameters in torch's layout and gate order i, f, g, o: W_ih [4H][n_in],
 * W_hh [4H][H], b_ih [4H], b_hh [4H], W_fc [n_out][H], b_fc [n_out]; both bias vectors are kept, as the reference trains
 * both.  Rows q H .. q H + H - 1 of W_ih, W_hh, b_ih, b_hh belong to gate q = 0 (i), 1 (f), 2 (g), 3 (o).  For group g:
 *   x[t][i]  = u[t][i] in_scale[g][i] + in_shift[g][i]     0 <= t < T;  u = 0 for T_in <= t < T (zero rows BEFORE scaling)
 *   z[t]     = W_ih x[t] + b_ih + W_hh h[t-1] + b_hh       h[-1] = c[-1] = 0 for every sequence (training, each frame)
 *   i, f, o  = sigma(z_i), sigma(z_f), sigma(z_o)          sigma(a) = 1 / (1 + exp(-a))
 *   gg       = tanh(z_g)
 *   c[t]     = f c[t-1] + i gg
 *   h[t]     = o tanh(c[t])
 *   ys[t]    = W_fc h[t] + b_fc
 *   loss     = sum_{transient <= t < T, o} (ys[t][o] - (D[g][t][o] t_scale[g][o] + t_shift[g][o]))^2 / ((T - transient) n_out)
 *   Adam exactly as in the FNN block above, epoch e = 1..epochs; loss[g][e] is the loss BEFORE step e.  The reference's
 *   values: H = 100, transient = 0, epochs = 50, lr = 0.01.
 *   predict: Y[f][t - transient][o] = (ys[t][o] - t_shift[g][o]) / t_scale[g][o], g = f / frames_per_group.
 * The gradients are exact backpropagation through time of this loss.  With dys[t][o] = 2 (ys[t][o] - Ds[t][o]) /
 * ((T - transient) n_out) for t >= transient and 0 before, dz[T] = 0 and dc_next[T] = 0, for t = T-1 .. 0:
 *   dh[t]   = W_fc^T dys[t] + W_hh^T dz[t+1]
 *   d_o     = dh[t] tanh(c[t])                              dc[t] = dc_next[t+1] + dh[t] o (1 - tanh(c[t])^2)
 *   d_i     = dc[t] gg       d_g = dc[t] i       d_f = dc[t] c[t-1]       dc_next[t] = dc[t] f
 *   dz_i    = d_i i (1 - i)  dz_f = d_f f (1 - f)  dz_g = d_g (1 - gg^2)  dz_o = d_o o (1 - o)
 * and  dW_hh = sum_t dz[t] h[t-1]^T,  dW_ih = sum_t dz[t] x[t]^T,  db_ih = db_hh = sum_t dz[t],
 *      dW_fc = sum_t dys[t] h[t]^T,   db_fc = sum_t dys[t].
 * A parameter whose gradient is exactly 0 in every epoch keeps m = v = 0 and comes out bitwise as it went in: with T = 1
 * that is all of W_hh (h[-1] = 0) and the forget-gate rows of W_ih, b_ih, b_hh (c[-1] = 0).
 * esn_lstm_train    group g starts from the initial set (group_offset + g) % n_isets of W_ih_0 .. b_fc_0 [n_isets][...]
 *                   and writes W_ih .. b_fc [G][...]; loss [G][epochs] may be NULL; U [G][T_in][n_in], D [G][T][n_out],
 *                   scalings [G][n] or NULL.  One workgroup per group and one launch for all epochs, float64.  The
 *                   products over all T rows (the input projection, the read-out with the loss, the weight gradients)
 *                   run on v_mfma_f64_16x16x4_f64; the 2 T dependent steps of an epoch's two sweeps run against a copy
 *                   of W_hh that stays in registers and LDS from one Adam step to the next (H <= 104: all of it; above,
 *                   columns 96 .. H - 1 are read from the L2 each step).  Every sum in an order that depends on the
 *                   shape alone, no atomics, nothing shared between workgroups: a group is bitwise the same alone, in
 *                   any batch and in any chunking, with or without `loss`.  ESN_F64 only: every other precision
 *                   returns -2.  workspace: device memory of esn_lstm_workspace_bytes(..., n_groups, 0, T) bytes, per
 *                   group 8 (3 (4H (n_in + 1) + 4H (H + 1) + n_out (H + 1)) + T n_in + 8 H T + (3 T + 2) H + T n_out)
 *                   bytes (the parameters and Adam's moments, the scaled input, gates, dz, c, tanh c, h, dys), not
 *                   initialised by the caller and of no meaning afterwards.
 * esn_lstm_predict  forward only: a workgroup takes up to 16 frames of one group through all T steps, each step's
 *                   [16 x 4H] = [h | x | 1] . [W_hh | W_ih | b_ih + b_hh]^T on v_mfma_f64_16x16x4_f64 with the frames as
 *                   rows; W_hh's operand stays in registers and LDS across steps (H <= 104: all of it), hidden rows
 *                   never reach memory.  A frame is bitwise the same alone and inside any batch.  ESN_F64 only (-2
 *                   otherwise).  workspace: esn_lstm_workspace_bytes(..., 0, n_frames, T) bytes = min(n_frames, 1024)
 *                   parts of 2048 ceil(H / 16) (ceil((n_in + 1) / 4) + r) bytes, r the k-steps of four columns of W_hh
 *                   beyond the 16 in registers and the floor((163840 - 128 (4 ceil(H / 4) + 1)) / (2048 ceil(H / 16)))
 *                   in LDS (r = 0 for H <= 104).
 * esn_lstm_workspace_bytes   the larger of what n_groups trainings and what a prediction of n_frames frames need (either
 *                   count may be 0); 0 for an unserved shape.
 * Served: 1 <= n_in <= 64, 1 <= n_hidden <= 128, 1 <= n_out <= 8, 1 <= T_in <= T <= 4096, 0 <= transient < T,
 * epochs >= 1, lr >= 0, 0 <= beta < 1, eps > 0.  Anything else returns -1 before any HIP call, the limit in
 * esn_last_error(); a short workspace returns -1 too.  No float32 I/O variant, no _mem front end, one pilot per group,
 * one layer.  These are additions: the ABI version is unchanged. */
size_t esn_lstm_workspace_bytes(int n_in, int n_hidden, int n_out, int n_groups, int n_frames, int T);
int esn_lstm_train(int precision, int n_in, int n_hidden, int n_out, int n_isets,
                   const double* W_ih_0, const double* W_hh_0, const double* b_ih_0, const double* b_hh_0,
                   const double* W_fc_0, const double* b_fc_0,
                   const double* in_scale, const double* in_shift, const double* t_scale, const double* t_shift,
                   const double* U, const double* D, int n_groups, int T_in, int T, int transient,
                   uint64_t group_offset, int epochs, double lr, double beta1, double beta2, double eps,
                   double* W_ih, double* W_hh, double* b_ih, double* b_hh, double* W_fc, double* b_fc, double* loss,
                   void* workspace, size_t workspace_bytes, void* stream);
int esn_lstm_predict(int precision, int n_in, int n_hidden, int n_out,
                     const double* W_ih, const double* W_hh, const double* b_ih, const double* b_hh,
                     const double* W_fc, const double* b_fc,
                     const double* in_scale, const double* in_shift, const double* t_scale, const double* t_shift,
                     const double* U, int n_frames, int frames_per_group, int T_in, int T, int transient,
                     double* Y, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Channel record of the block-fading drivers (OFDM_MIMO_2-2_NBF_LDPC.py:369-385; the 4x8 ChannelRank driver is
 * named after it), float64.  H complex [G][N][n_r][n_t] in the layout of the function above, 16-byte aligned; p_i [G]
 * on the device as in the detectors; per subcarrier k the singular values s_1 >= ... of H_k by one-sided complex
 * Jacobi (no H^H H: its eigenvalues square the condition number), then
 *     rank [G][N]  = #{ s_i^2 >= max(1e-2 s_1^2, 10 No / Pi) }                                    (:379-380)
 *     cond [G][N]  = s_1 / max(s_min, 1e-12)                                                      (:381)
 *     cap  [G]     = mean over k of sum_i log2(1 + (Pi / No / n_t) s_i^2)                         (:372,382-383)
 *     S    [G][N][min(n_t, n_r)]  optional (NULL), descending                                     (:376)
 * min(n_t, n_r) <= 4 and max(n_t, n_r) <= 8, else -1 ("unsupported").  A zero matrix gives S = 0, rank 0, cond 0;
 * non-finite entries give NaN for that subcarrier; the iteration count is bounded for every input.  A block's outputs
 * are bitwise the same alone or inside any batch (cap is reduced in a fixed order).  The per-Eb/No aggregates of
 * :515-521 (mean, fraction of full rank, percentiles) are the caller's. */
int esn_channel_metrics(int n_blocks, int n_sub, int n_t, int n_r, const double* H, const double* p_i, double no,
                        double* S, double* cond, uint8_t* rank, double* cap, void* stream);

/* ---- Coded leg of the north-star driver, float64.  The reference delegates the code
 * to the un-vendored package pyldpc (requirements-sm2.txt:5); these entry points restate its
 * published algorithms at the reference's call sites (parity unpinned, see oracle/ldpc_oracle.py).
 * esn_ldpc_encode        c = [u ; P u mod 2] per (frame, tx) into TxBits [B][n][n_t], n = N*m
 *                        (Demo_MIMO_4x8_Sionna_CDL_ESN_v2.py:90-93, :399-404); P [n-k][k] bytes.
 * esn_qam_llr            X_hat complex [B][N][n_t] -> max-log LLRs [B][n_t][N*m] (positive = bit 0)
 *                        scaled by the decision-directed sigma^2 of the frame (:66-88, :108-112, :459-469).
 * esn_ldpc_decode_count  pyldpc.decode: flooding log-domain sum-product on y [n_cw][n] with
 *                        var = 10^(-snr_db/10), Lc = 2 y / var, at most maxiter sweeps, early stop on a
 *                        zero syndrome (:495-496); message = first k bits (get_message); info-bit
 *                        errors vs u_true accumulated per group of cw_per_group codewords (:508-511).
 *                        Graph in CSR form: chk_ptr [m+1], edge_var [E] (check-major), var_ptr [n+1],
 *                        var_edge [E]. */
int esn_ldpc_encode(int n_frames, int n_t, int k, int n, const uint8_t* P, const uint8_t* u,
                    uint8_t* bits, void* stream);
int esn_qam_llr(int n_frames, int n_sub, int n_t, int bits_per_sym, const double* X_hat,
                double* llr, double* sigma2, void* stream);
int esn_ldpc_decode_count(int n_cw, int n, int k, int m_checks, int n_edges,
                          const int* chk_ptr, const int* edge_var, const int* var_ptr, const int* var_edge,
                          const double* y, double snr_db, int maxiter, const uint8_t* u_true, int cw_per_group,
                          uint8_t* x_out, long long* err_count, long long* bit_count, void* stream);

/* ---- SINR-weighted soft outputs behind the LS-MMSE equaliser (extension: the reference gives every symbol of a frame
 * one decision-directed sigma^2), float64.  Plain additions: the ABI version stays.
 * esn_mmse_sinr          per block g, subcarrier k and stream i, with lam = no / p_i[g] and H_k = H[g][k] ([n_r][n_t]):
 *                          t = lam [(H_k^H H_k + lam I)^-1]_ii clamped to [1e-12, 1 - 1e-12]; the Gram matrix by the
 *                          operations of esn_mmse_detect_count
 *                          mu = 1 - t   the equaliser's bias,   gamma = (1 - t) / t   its SINR
 *                          w  = gamma / gamma_mean[g], gamma_mean[g] the mean of gamma over the block's N n_t entries,
 *                          summed in an order the shape alone decides (no atomics)
 *                        w, mu [G][N][n_t]; gamma_mean [G] optional (NULL).  One workgroup per block.
 * esn_qam_llr_weighted   sigma2[f] bitwise that of esn_qam_llr (taken on X_hat as it is), then, for frame f of group
 *                        g = f / frames_per_group,
 *                          llr[f][i][k m + b] = w[g][k][i] (d1 - d0)(X_hat[f][k][i] / mu[g][k][i]) / sigma2[f]
 *                        with the max-log distances, sign (positive = bit 0) and layout of esn_qam_llr.  w or mu NULL: 1;
 *                        both NULL: llr is bitwise that of esn_qam_llr.
 * esn_detect_llr[_f32]   the fused soft tail: esn_detect_count[_f32] on Y (err_count, bit_count and the optional X_hat
 *                        are bitwise that entry point's) and esn_qam_llr_weighted on its X_hat (llr and sigma2 bitwise),
 *                        one workgroup per frame, X_hat never in memory unless asked for.  tx_bits may be NULL: nothing is
 *                        counted.  Every element of llr is written; no atomics but the two counters.  One workgroup holds
 *                        esn_detect_llr_lds_bytes(N, n_t) = 16 (n_t (N + 1) + N/2) bytes of LDS; beyond 150 KiB the call
 *                        returns -2 and the caller takes esn_detect_count with X_hat, then esn_qam_llr_weighted.
 * Served: N a power of two in [2, 2048], 1 <= n_t <= 4, any n_r >= 1, bits_per_sym even in [2, 10]; anything else returns
 * -1 before any HIP call, the argument named in esn_last_error().  (All of that fits the LDS: 147 520 bytes at N = 2048,
 * n_t = 4.) */
int esn_mmse_sinr(int n_blocks, int n_sub, int n_t, int n_r, const double* p_i, double no, const double* H,
                  double* w, double* mu, double* gamma_mean, void* stream);
int esn_qam_llr_weighted(int n_frames, int frames_per_group, int n_sub, int n_t, int bits_per_sym,
                         const double* X_hat, const double* w, const double* mu, double* llr, double* sigma2,
                         void* stream);
size_t esn_detect_llr_lds_bytes(int n_sub, int n_t);
int esn_detect_llr(const double* Y, int n_frames, int frames_per_group, int n_sub, int n_t, int bits_per_sym,
                   const double* p_i, const uint8_t* tx_bits, long long* err_count, long long* bit_count,
                   const double* w, const double* mu, double* llr, double* sigma2, double* X_hat, void* stream);
int esn_detect_llr_f32(const float* Y, int n_frames, int frames_per_group, int n_sub, int n_t, int bits_per_sym,
                       const double* p_i, const uint8_t* tx_bits, long long* err_count, long long* bit_count,
                       const double* w, const double* mu, double* llr, double* sigma2, double* X_hat, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ESN_HIP_H */
