// Windowed ELM (include/esn_hip.h: esn_elm_features, esn_elm_predict): a random tanh layer over the last `window` rows of
// the scaled input, a bias column and a linear read-out.  With K = window n_in and the scaled rows us[t][i]:
//   pre[t][h] = b[h] + sum_{j<K} W_in[h][j] usflat[(t - (window-1)) n_in + j]       the window is a VIEW of the staged rows:
//   row[t]    = [ tanh(pre[t][:]) | 1 | 0 .. ]                                      sample k, input i sits at j = k n_in + i
//   Y[t][o]   = (sum_c W_out[o][c] row[t][c] - t_shift[o]) / t_scale[o]
// Two kernels.
//   elm_f64_kernel   float64, plain FMA: a workgroup owns 16 rows of one sequence, a thread one hidden unit of a chunk of
//                    256 and its 16 sums (j ascending, one chain per row: the order depends on nothing but K).  Features
//                    are written as they come; for the fused prediction a chunk's hidden rows go to LDS beside the chunk
//                    of W_out, a thread adds one of S contiguous ranges of the chunk into its (row, output) sum, chunk
//                    after chunk, and the S partial sums join pairwise (range s + h into range s).  S depends on n_out
//                    alone, so a sequence is bitwise the same alone or inside any batch.  Hidden rows never reach HBM.
//   elm_f16_kernel   v_mfma_f32_16x16x32_f16, fp16 operands, float32 accumulators, bias and tanh.  Persistent: W_in is
//                    converted to fp16 into LDS once per workgroup (per weight set), each of the four waves takes whole
//                    (sequence, row batch) items on its own.  A wave stages its scaled rows as fp16 in LDS, keeps their
//                    B operands (time on the lane) in registers, and walks the hidden units 32 at a time:
//                    pre^T = W_in us^T for two 16-unit tiles, tanh, and the two accumulator tiles ARE the B operand of
//                    the read-out product Y^T += W_out[:, 32 units] hid^T (the sum runs over the accumulators' row index),
//                    with the k order of that step permuted alike on the W_out side.  No barrier inside an item but the
//                    one after staging; no atomics.
// Both take the activation as a template parameter: RELU = true is the windowed FNN's prediction (esn_fnn_predict):
// max(., 0) for tanh, and the bias column's weights come from p.b_out beside W_out = W2.  The fp16 kernel rounds the
// ReLU outputs to fp16 like the tanh ones; they are unbounded, so inputs are expected at about unit variance.
#include <atomic>
#include "esn_common.h"
#include "esn_launch.h"
#include "esn_mfma_traits.h"

namespace esn {

constexpr int ELM_TR = 16;                     // rows of a float64 tile
constexpr int ELM_THREADS = 256;               // and hidden units of a chunk
constexpr int ELM_HS = ELM_THREADS + 1;        // LDS row stride of a chunk, in doubles
constexpr int ELM_MAX_OUT = 8;
constexpr size_t ELM_MAX_LDS = 160 * 1024;
constexpr int ELM16_WAVES = 4;

__device__ __forceinline__ int elm_wset(const ElmParams& p, int g) {
    return (int)((p.group_offset + (unsigned long long)g) % (unsigned long long)p.n_wsets);
}
// scaled input us[t][i] of sequence q (group g), 0 <= t < T: rows from T_in on are zero BEFORE scaling
__device__ __forceinline__ double elm_input(const ElmParams& p, int q, int g, int t, int i) {
    const double u = t < p.T_in ? p.U[((size_t)q * p.T_in + t) * p.n_in + i] : 0.0;
    const double sc = p.in_scale ? p.in_scale[(size_t)g * p.n_in + i] : 1.0;
    const double sh = p.in_shift ? p.in_shift[(size_t)g * p.n_in + i] : 0.0;
    return u * sc + sh;
}

// k ranges a (row, output) sum of the float64 read-out is split into: a power of two, 16 n_out S <= 256 threads
static inline int elm_segments(int n_out) {
    int s = 16;
    while (s > 1 && s * ELM_TR * n_out > ELM_THREADS) s >>= 1;
    return s;
}
static inline size_t elm_f64_lds_bytes(const ElmParams& p, bool predict) {
    size_t d = (size_t)round_up((ELM_TR + p.window - 1) * p.n_in, 2);
    if (predict) d += (size_t)ELM_TR * ELM_HS + (size_t)ELM_MAX_OUT * ELM_HS + (size_t)ELM_TR * ELM_MAX_OUT;
    return d * sizeof(double);
}

template <bool PREDICT, bool RELU = false>
__global__ __launch_bounds__(ELM_THREADS) void elm_f64_kernel(ElmParams p, int n_seg) {
    extern __shared__ __attribute__((aligned(16))) char esm[];
    const int n_in = p.n_in, w = p.window, K = w * n_in, nh = p.n_hidden, T = p.T, n_out = p.n_out;
    const int tid = threadIdx.x;
    const int n_tiles = (T + ELM_TR - 1) / ELM_TR;
    const int q = blockIdx.x / n_tiles, t0 = (blockIdx.x - q * n_tiles) * ELM_TR;
    if (PREDICT && t0 + ELM_TR <= p.transient) return;            // (the whole workgroup)
    const int g = q / p.seq_per_group, s = elm_wset(p, g);
    const int us_rows = ELM_TR + w - 1;
    double* us = reinterpret_cast<double*>(esm);                   // [us_rows][n_in]: rows t0 - (w-1) .. t0 + 15
    double* hid = us + round_up(us_rows * n_in, 2);                // [16][ELM_HS]   hidden rows of the chunk
    double* wo = hid + ELM_TR * ELM_HS;                            // [8][ELM_HS]    W_out of the chunk
    double* outb = wo + ELM_MAX_OUT * ELM_HS;                      // [16][n_out]
    for (int e = tid; e < us_rows * n_in; e += ELM_THREADS) {
        const int lr = e / n_in, i = e - lr * n_in, t = t0 - (w - 1) + lr;
        us[e] = (t >= 0 && t < T) ? elm_input(p, q, g, t, i) : 0.0;
    }
    __syncthreads();

    // the read-out sum this thread owns: (row r2, output o2), range seg of every chunk
    const int P = ELM_TR * n_out, len = ELM_THREADS / n_seg;
    const int seg = tid / (PREDICT ? P : ELM_THREADS), pair = tid - seg * P;
    const int r2 = pair / n_out, o2 = pair - r2 * n_out;
    const bool owner = PREDICT && seg < n_seg;
    double ysum = 0.0;

    const int ncol = PREDICT ? nh + p.bias_col : p.e_cols;
    for (int c0 = 0; c0 < ncol; c0 += ELM_THREADS) {
        const int c = c0 + tid;
        double v[ELM_TR];
        if (c < nh) {
            const double* wr = p.W_in + ((size_t)s * nh + c) * K;
            double acc[ELM_TR];
#pragma unroll
            for (int r = 0; r < ELM_TR; ++r) acc[r] = 0.0;
            int j = 0;
            for (; j + 8 <= K; j += 8) {
                double wv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) wv[u] = wr[j + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
#pragma unroll
                    for (int r = 0; r < ELM_TR; ++r) acc[r] = fma(wv[u], us[r * n_in + j + u], acc[r]);
                }
            }
            for (; j < K; ++j) {
                const double wv = wr[j];
#pragma unroll
                for (int r = 0; r < ELM_TR; ++r) acc[r] = fma(wv, us[r * n_in + j], acc[r]);
            }
            const double bb = p.b[(size_t)s * nh + c];
#pragma unroll
            for (int r = 0; r < ELM_TR; ++r) {
                if constexpr (RELU) v[r] = fmax(acc[r] + bb, 0.0);
                else v[r] = tanh(acc[r] + bb);
            }
        } else {
            const double one = (c == nh && p.bias_col) ? 1.0 : 0.0;
#pragma unroll
            for (int r = 0; r < ELM_TR; ++r) v[r] = one;
        }
        if constexpr (!PREDICT) {
            if (c < ncol) {
#pragma unroll
                for (int r = 0; r < ELM_TR; ++r) {
                    const int t = t0 + r;
                    if (t < T) {
                        const double x = t >= w - 1 ? v[r] : 0.0;
                        const size_t at = ((size_t)g * T + t) * p.e_cols + c;
                        if (p.e_f32) reinterpret_cast<float*>(p.E)[at] = (float)x;
                        else reinterpret_cast<double*>(p.E)[at] = x;
                    }
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < ELM_TR; ++r) hid[r * ELM_HS + tid] = v[r];      // (zero beyond the last column)
            for (int e = tid; e < n_out * ELM_THREADS; e += ELM_THREADS) {
                const int o = e / ELM_THREADS, cc = e - o * ELM_THREADS;
                if constexpr (RELU)                                     // W_out = W2 [n_out][nh], the bias column apart
                    wo[o * ELM_HS + cc] = c0 + cc < nh ? p.W_out[((size_t)g * n_out + o) * p.e_cols + c0 + cc]
                                                       : (c0 + cc == nh ? p.b_out[(size_t)g * n_out + o] : 0.0);
                else
                    wo[o * ELM_HS + cc] = c0 + cc < ncol ? p.W_out[((size_t)g * n_out + o) * p.e_cols + c0 + cc] : 0.0;
            }
            __syncthreads();
            if (owner) {
                const double* hr = hid + r2 * ELM_HS + seg * len;
                const double* wr = wo + o2 * ELM_HS + seg * len;
                for (int cc = 0; cc < len; ++cc) ysum = fma(hr[cc], wr[cc], ysum);
            }
            __syncthreads();
        }
    }
    if constexpr (PREDICT) {
        double* part = hid;                                         // [S/2][P]
        for (int h = n_seg >> 1; h >= 1; h >>= 1) {
            if (owner && seg >= h && seg < 2 * h) part[(seg - h) * P + pair] = ysum;
            __syncthreads();
            if (owner && seg < h) ysum += part[seg * P + pair];
            __syncthreads();
        }
        if (owner && seg == 0) {
            const double tsc = p.t_scale ? p.t_scale[(size_t)g * n_out + o2] : 1.0;
            const double tsh = p.t_shift ? p.t_shift[(size_t)g * n_out + o2] : 0.0;
            outb[pair] = t0 + r2 >= w - 1 ? (ysum - tsh) / tsc : 0.0;
        }
        __syncthreads();
        // rows lo .. hi - 1 of this tile are one contiguous run of Y
        const int lo = t0 > p.transient ? t0 : p.transient, hi = t0 + ELM_TR < T ? t0 + ELM_TR : T;
        const int n = (hi - lo) * n_out;
        double* dst = p.Y + ((size_t)q * (T - p.transient) + (lo - p.transient)) * n_out;
        const double* src = outb + (lo - t0) * n_out;
        if ((n_out & 1) == 0) {                                     // every row starts on 16 bytes
            for (int e = tid; e < n / 2; e += ELM_THREADS)
                reinterpret_cast<double2*>(dst)[e] = make_double2(src[2 * e], src[2 * e + 1]);
        } else {
            for (int e = tid; e < n; e += ELM_THREADS) dst[e] = src[e];
        }
    }
}

// ---- fp16 on the matrix pipe ------------------------------------------------------------------------------------
// NT row tiles of 16 per item, KK k-steps of 32 (window n_in <= 32 KK); W_LDS: the fp16 image of W_in fits LDS
template <int NT, int KK>
static inline int elm16_tile_halfs(const ElmParams& p) {          // a wave's staged rows, with slack for the last window
    return round_up((16 * NT + p.window - 1) * p.n_in + 32 * KK, 8);
}
template <int NT, int KK>
static inline size_t elm16_lds_bytes(const ElmParams& p, bool w_lds) {
    const int nhp = round_up(p.n_hidden, 32);
    return (w_lds ? (size_t)nhp * (32 * KK + 8) * 2 : 0) + (size_t)nhp * 4 + (size_t)ELM16_WAVES * elm16_tile_halfs<NT, KK>(p) * 2;
}

// the 8 read-out weights of output row `wrow` that meet hidden units h0 .. h0 + 31 in lane quarter qd: element j is unit
// h0 + 4 qd + j (j < 4) or h0 + 16 + 4 qd + j - 4, the rows the two accumulator tiles hold in that quarter
// (every load is unconditional, from a clamped column of a row that exists, and the select comes after: a load under a
// per-element condition is branched around and waited for one at a time)
__device__ __forceinline__ u32x4 elm16_wout_frag(const double* wrow, bool valid, int h0, int qd, int nh) {
    double v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = h0 + 4 * qd + (j < 4 ? j : 12 + j);
        v[j] = wrow[c < nh ? c : nh - 1];
    }
    h16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = h0 + 4 * qd + (j < 4 ? j : 12 + j);
        r[j] = (valid && c < nh) ? (_Float16)v[j] : (_Float16)0.0f;
    }
    return __builtin_bit_cast(u32x4, r);
}

template <int NT, int KK, bool W_LDS, bool RELU = false>
__global__ __launch_bounds__(64 * ELM16_WAVES) void elm_f16_kernel(ElmParams p, int n_batches, int ul) {
    extern __shared__ __attribute__((aligned(16))) char esm[];
    constexpr int ROWS = 16 * NT, KP = 32 * KK, WLD = KP + 8;      // (+ 8 halfs: rows 16 bytes apart in the banks)
    const int n_in = p.n_in, w = p.window, K = w * n_in, nh = p.n_hidden, T = p.T, n_out = p.n_out;
    const int nhp = round_up(nh, 32), tile_elems = (ROWS + w - 1) * n_in;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, qd = lane >> 4;
    _Float16* Wl = reinterpret_cast<_Float16*>(esm);                                   // [nhp][WLD]
    float* bsc = reinterpret_cast<float*>(esm + (W_LDS ? (size_t)nhp * WLD * 2 : 0)); // [nhp]  b 2 log2 e
    _Float16* ust = reinterpret_cast<_Float16*>(bsc + nhp) + (size_t)wave * ul;        // this wave's rows
    const float prescale = RELU ? 1.0f : (float)ACT_PRESCALE;     // (ReLU: the plain pre-activation)
    for (int e = tile_elems + lane; e < ul; e += 64) ust[e] = (_Float16)0.0f;         // (never written again)

    const bool by_group = p.n_wsets > 1;              // then a workgroup walks whole groups: one weight set at a time
    const int n_groups = (p.n_seq + p.seq_per_group - 1) / p.seq_per_group;
    const int n_units = by_group ? n_groups : (int)gridDim.x;
    int loaded = -1;
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        long long first, end, stride;                  // items: (sequence, batch) pairs, fewer than 2^31 in all
        int s = 0;
        if (by_group) {
            s = elm_wset(p, unit);
            const long long f0 = (long long)unit * p.seq_per_group;
            const long long f1 = f0 + p.seq_per_group < p.n_seq ? f0 + p.seq_per_group : p.n_seq;
            first = f0 * n_batches; end = f1 * n_batches; stride = ELM16_WAVES;
        } else {
            first = (long long)unit * ELM16_WAVES; end = (long long)p.n_seq * n_batches;
            stride = (long long)gridDim.x * ELM16_WAVES;
        }
        if (s != loaded) {
            __syncthreads();
            if constexpr (W_LDS) {
                for (int e = tid; e < nhp * (KP / 2); e += 64 * ELM16_WAVES) {
                    const int h = e / (KP / 2), k = 2 * (e - h * (KP / 2));
                    const double* src = p.W_in + ((size_t)s * nh + h) * K;
                    const float v0 = (h < nh && k < K) ? (float)src[k] : 0.0f;
                    const float v1 = (h < nh && k + 1 < K) ? (float)src[k + 1] : 0.0f;
                    *reinterpret_cast<uint32_t*>(Wl + (size_t)h * WLD + k) = TraitsF16::pack2(v0, v1);
                }
            }
            for (int h = tid; h < nhp; h += 64 * ELM16_WAVES)
                bsc[h] = h < nh ? (float)(p.b[(size_t)s * nh + h] * (RELU ? 1.0 : ACT_PRESCALE)) : 0.0f;
            loaded = s;
            __syncthreads();
        }
        for (long long base = first; base < end; base += stride) {
            const long long item = base + wave;
            int fr = 0, t0 = 0;
            if (item < end) { fr = (int)(item / n_batches); t0 = (int)(item - (long long)fr * n_batches) * ROWS; }
            const int g = fr / p.seq_per_group;
            const bool work = item < end && t0 + ROWS > p.transient;
            if (work) {
                // 8 elements per lane and pass, every load unconditional (row and element clamped, selected afterwards)
                const double* uf = p.U + (size_t)fr * p.T_in * n_in;
                for (int e0 = lane; e0 < tile_elems; e0 += 64 * 8) {
                    double u[8], sc[8], sh[8];
                    int at[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int e = e0 + 64 * j < tile_elems ? e0 + 64 * j : tile_elems - 1;
                        const int lr = e / n_in, t = t0 - (w - 1) + lr;
                        at[j] = e - lr * n_in;
                        const int tc = t < 0 ? 0 : (t < p.T_in ? t : p.T_in - 1);
                        u[j] = uf[(size_t)tc * n_in + at[j]];
                        if (t < 0 || t >= p.T_in) u[j] = 0.0;
                        sc[j] = 1.0; sh[j] = 0.0;
                        if (t < 0 || t >= T) at[j] = -1;                 // (outside the sequence: a zero row)
                    }
                    if (p.in_scale) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) sc[j] = p.in_scale[(size_t)g * n_in + (at[j] < 0 ? 0 : at[j])];
                    }
                    if (p.in_shift) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) sh[j] = p.in_shift[(size_t)g * n_in + (at[j] < 0 ? 0 : at[j])];
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (e0 + 64 * j < tile_elems) ust[e0 + 64 * j] = (_Float16)(at[j] < 0 ? 0.0 : u[j] * sc[j] + sh[j]);
                }
            }
            __syncthreads();
            if (!work) continue;                       // (no barrier below: the tile is this wave's own)

            // B operands of the first product: lane (col, qd) holds us window of row 16 nt + col, k = 32 kk + 8 qd ..
            u32x4 bf[NT][KK];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const int k0 = kk * 32 + 8 * qd;
                    const _Float16* src = ust + (nt * 16 + col) * n_in + k0;
                    if ((n_in & 7) == 0 && k0 + 8 <= K) {
                        bf[nt][kk] = *reinterpret_cast<const u32x4*>(src);
                    } else {
                        h16x8 r;
#pragma unroll
                        for (int j = 0; j < 8; ++j) r[j] = k0 + j < K ? src[j] : (_Float16)0.0f;
                        bf[nt][kk] = __builtin_bit_cast(u32x4, r);
                    }
                }
            }
            f32x4 ys[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) ys[nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            // what the epilogue needs of outputs o = 4 qd .. 4 qd + 3, loaded here (unconditionally, the index clamped)
            // so that the loads are long back when the hidden units are done
            double wb[4], tsc[4], tsf[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t go = (size_t)g * n_out + (4 * qd + j < n_out ? 4 * qd + j : 0);
                if constexpr (RELU) wb[j] = p.b_out[go];
                else wb[j] = p.W_out[go * p.e_cols + (p.bias_col ? nh : nh - 1)];
                tsc[j] = 1.0; tsf[j] = 0.0;
            }
            if (p.t_scale) {
#pragma unroll
                for (int j = 0; j < 4; ++j) tsc[j] = p.t_scale[(size_t)g * n_out + (4 * qd + j < n_out ? 4 * qd + j : 0)];
            }
            if (p.t_shift) {
#pragma unroll
                for (int j = 0; j < 4; ++j) tsf[j] = p.t_shift[(size_t)g * n_out + (4 * qd + j < n_out ? 4 * qd + j : 0)];
            }
            const bool has_row = col < n_out;
            const double* wrow = p.W_out + ((size_t)g * n_out + (has_row ? col : 0)) * p.e_cols;
            u32x4 wof = elm16_wout_frag(wrow, has_row, 0, qd, nh);
            u32x4 wof_1 = elm16_wout_frag(wrow, has_row, 32, qd, nh);
            for (int h0 = 0; h0 < nhp; h0 += 32) {
                const u32x4 wof_2 = elm16_wout_frag(wrow, has_row, h0 + 64, qd, nh);      // two steps ahead
                f32x4 acc[2][NT];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[0][nt] = acc[1][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    if (kk * 32 < K) {
                        u32x4 a[2];
#pragma unroll
                        for (int tl = 0; tl < 2; ++tl) {
                            const int h = h0 + 16 * tl + col, k0 = kk * 32 + 8 * qd;
                            if constexpr (W_LDS) {
                                a[tl] = *reinterpret_cast<const u32x4*>(Wl + (size_t)h * WLD + k0);
                            } else {
                                const double* src = p.W_in + ((size_t)s * nh + (h < nh ? h : 0)) * K;
                                h16x8 r;
#pragma unroll
                                for (int j = 0; j < 8; ++j)
                                    r[j] = (h < nh && k0 + j < K) ? (_Float16)src[k0 + j] : (_Float16)0.0f;
                                a[tl] = __builtin_bit_cast(u32x4, r);
                            }
                        }
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            TraitsF16::mma16(acc[0][nt], a[0], bf[nt][kk]);
                            TraitsF16::mma16(acc[1][nt], a[1], bf[nt][kk]);
                        }
                    }
                }
                const f32x4 bz0 = *reinterpret_cast<const f32x4*>(bsc + h0 + 4 * qd);
                const f32x4 bz1 = *reinterpret_cast<const f32x4*>(bsc + h0 + 16 + 4 * qd);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    float x[8];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if constexpr (RELU) {
                            x[j] = fmaxf(acc[0][nt][j] + bz0[j], 0.0f);
                            x[4 + j] = fmaxf(acc[1][nt][j] + bz1[j], 0.0f);
                        } else {
                            x[j] = tanh_prescaled(fmaf(acc[0][nt][j], prescale, bz0[j]));
                            x[4 + j] = tanh_prescaled(fmaf(acc[1][nt][j], prescale, bz1[j]));
                        }
                    }
                    const u32x4 hf = {TraitsF16::pack2(x[0], x[1]), TraitsF16::pack2(x[2], x[3]),
                                      TraitsF16::pack2(x[4], x[5]), TraitsF16::pack2(x[6], x[7])};
                    TraitsF16::mma16(ys[nt], wof, hf);
                }
                wof = wof_1;
                wof_1 = wof_2;
            }

            // lane (col, qd) holds outputs o = 4 qd .. 4 qd + 3 of row 16 nt + col
            float wob[4];
            double inv[4], tsh[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool valid = 4 * qd + j < n_out;
                wob[j] = (valid && p.bias_col) ? (float)(_Float16)wb[j] : 0.0f;
                inv[j] = 1.0 / (valid ? tsc[j] : 1.0);
                tsh[j] = valid ? tsf[j] : 0.0;
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int t = t0 + nt * 16 + col;
                if (t >= p.transient && t < T) {
                    double y[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        y[j] = t >= w - 1 ? ((double)(ys[nt][j] + wob[j]) - tsh[j]) * inv[j] : 0.0;
                    double* dst = p.Y + ((size_t)fr * (T - p.transient) + (t - p.transient)) * n_out + 4 * qd;
                    if ((n_out & 3) == 0) {
                        if (4 * qd < n_out) {
                            reinterpret_cast<double2*>(dst)[0] = make_double2(y[0], y[1]);
                            reinterpret_cast<double2*>(dst)[1] = make_double2(y[2], y[3]);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (4 * qd + j < n_out) dst[j] = y[j];
                    }
                }
            }
        }
    }
}

// the CU count of the current device, which sizes the persistent grid of the fp16 kernels
static int elm_cu_count(int* cu_count) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(cu_count, hipDeviceAttributeMultiprocessorCount, dev);
    return (int)e;
}

int launch_elm_features(const ElmParams& p, hipStream_t stream) {
    const int n_tiles = (p.T + ELM_TR - 1) / ELM_TR;
    hipLaunchKernelGGL(elm_f64_kernel<false>, dim3((unsigned)(p.n_seq * n_tiles)), dim3(ELM_THREADS),
                       elm_f64_lds_bytes(p, false), stream, p, 1);
    return (int)hipGetLastError();
}

template <int NT, int KK, bool W_LDS, bool RELU>
static int launch_elm16(const ElmParams& p, hipStream_t stream) {
    static std::atomic<unsigned long long> raised{0};
    int cus = 0;
    int e = elm_cu_count(&cus);
    if (!e)
        e = raise_dynamic_lds_once(reinterpret_cast<const void*>(elm_f16_kernel<NT, KK, W_LDS, RELU>), ELM_MAX_LDS,
                                   raised);
    if (e) return e;
    const size_t lds = elm16_lds_bytes<NT, KK>(p, W_LDS);
    const int n_batches = (p.T + 16 * NT - 1) / (16 * NT);
    const long long n_items = (long long)p.n_seq * n_batches;
    const int n_groups = (p.n_seq + p.seq_per_group - 1) / p.seq_per_group;
    const long long units = p.n_wsets > 1 ? n_groups : (n_items + ELM16_WAVES - 1) / ELM16_WAVES;
    const long long resident = (long long)cus * (lds <= ELM_MAX_LDS / 2 ? 2 : 1);
    hipLaunchKernelGGL((elm_f16_kernel<NT, KK, W_LDS, RELU>), dim3((unsigned)(units < resident ? units : resident)),
                       dim3(64 * ELM16_WAVES), lds, stream, p, n_batches, elm16_tile_halfs<NT, KK>(p));
    return (int)hipGetLastError();
}

template <bool RELU>
static int launch_predict(int precision, const ElmParams& p, hipStream_t stream) {
    if (precision == ESN_F64) {
        static std::atomic<unsigned long long> raised{0};
        const int e = raise_dynamic_lds_once(reinterpret_cast<const void*>((elm_f64_kernel<true, RELU>)), ELM_MAX_LDS,
                                             raised);
        if (e) return e;
        const int n_tiles = (p.T + ELM_TR - 1) / ELM_TR;
        hipLaunchKernelGGL((elm_f64_kernel<true, RELU>), dim3((unsigned)(p.n_seq * n_tiles)), dim3(ELM_THREADS),
                           elm_f64_lds_bytes(p, true), stream, p, elm_segments(p.n_out));
        return (int)hipGetLastError();
    }
    if (precision != ESN_F16) return -1;
    if (p.window * p.n_in <= 128) {
        if (elm16_lds_bytes<9, 4>(p, true) <= ELM_MAX_LDS) return launch_elm16<9, 4, true, RELU>(p, stream);
        return launch_elm16<9, 4, false, RELU>(p, stream);
    }
    if (elm16_lds_bytes<4, 8>(p, true) <= ELM_MAX_LDS) return launch_elm16<4, 8, true, RELU>(p, stream);
    return launch_elm16<4, 8, false, RELU>(p, stream);
}

int launch_elm_predict(int precision, const ElmParams& p, hipStream_t stream) {
    return launch_predict<false>(precision, p, stream);
}
int launch_fnn_predict(int precision, const ElmParams& p, hipStream_t stream) {
    return launch_predict<true>(precision, p, stream);
}

}  // namespace esn
