// Spectral radius on the fp16 matrix pipe: the recurrence and the ratio form of esn_reservoir.hip's
// specrad_*_kernel,
//     f_0 = |W|;  k = 1..K:  B_k = A_{k-1} A_{k-1},  f_k = |B_k|,  l_k = 2 l_{k-1} + ln f_k,  A_k = B_k / f_k
//     radius = exp((l_{K-1} + ln f_K) / 2^(K-1))
// with every squaring as three float16 products accumulated in float32 on v_mfma_f32_32x32x16_f16:
//     X = s B  (s = 2^(ceil(log2 padded n) - 2): |B| <= 1 gives s |b_ij| <= s <= 1024, inside fp16 by construction)
//     hi = fp16(X),  lo = fp16((X - hi) 2^11)
//     X X ~ hi hi + 2^-11 (hi lo + lo hi)          (hi lo and lo hi share an accumulator)
//
// An image holds s B_k, un-normalised by its own norm; 1 / (s f_k^2) multiplies the product in the NEXT launch's
// epilogue, which is where s A_k A_k = (s B_k)(s B_k) / (s f_k^2) comes out, so no pass normalises.  An image lies in
// the workspace in both orientations, each as a hi and a lo plane, zero-padded to a multiple of 64: the MFMA wants 8
// consecutive k per lane of both operands, which are rows of the image for A and rows of its transpose for B, so the
// epilogue stores its tile and the tile's transpose.  2 images x 2 orientations x 2 planes x 2 B = 16 n^2 bytes per
// matrix, what the float64 path's two images take.
//
// Norms stay in float64: |B_k|^2 leaves a launch as one partial per 64 x 64 tile (of the float32 values before they
// are split), and every workgroup of the next launch adds its matrix's partials in the same fixed order.  No
// floating-point atomics; the grid of a matrix depends on n alone, so its radius is bitwise the same alone and in
// any batch.  An unusable f_k (zero, infinite, NaN) zeroes the matrix's operands from then on: status 1, radius 0,
// neighbours untouched.  A matrix whose powers fall below the fp16 range (entries of s B_k under 6e-8 become zero) may
// be flagged where the float64 path would still measure it.
//
// Launches: the tile norms of W, the split image of s W / f_0, K squarings, the final ratio; no host read.
// Self-contained, as esn_reservoir.hip and esn_loo.hip are.
#include "esn_common.h"
#include "esn_launch.h"

namespace esn {

constexpr int SS_TILE = 64;                 // workgroup tile of B, and the padding unit of an image
constexpr int SS_KC = 64;                   // contraction steps staged per barrier pair
constexpr int SS_NT = 256;                  // threads: 4 waves, 2 x 2 over the tile, a 32 x 32 MFMA tile each
constexpr int SS_NW = SS_NT / 64;
constexpr int SS_LD = SS_KC + 8;            // staged row stride in halves (144 B): the 16-byte fragment reads of 16
                                            // consecutive rows start 36 banks apart and cover all 64 banks once
constexpr int SS_PLANE = SS_TILE * SS_LD;   // one staged plane [64 rows][SS_LD]: A hi | A lo | B^T hi | B^T lo
constexpr float SS_LO = 2048.0f;            // 2^11, the bits the hi piece holds
static_assert(4 * SS_PLANE * 2 + SS_NW * 8 <= 40 * 1024, "four workgroups per CU");

typedef _Float16 ss_half;
typedef _Float16 ss_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 ss_h4 __attribute__((ext_vector_type(4)));
typedef float ss_f16v __attribute__((ext_vector_type(16)));

__host__ __device__ inline int ss_padded(int n) { return (n + SS_TILE - 1) / SS_TILE * SS_TILE; }
__host__ __device__ inline double ss_scale(int np) {
    int e = 0;
    while ((1 << e) < np) ++e;              // ceil(log2 np), np >= 64
    return (double)(1 << (e - 2));
}

// workspace of one matrix: halves [image 2][orientation 2][plane 2][np * np], then doubles: partials 0 [nt] |
// partials 1 [nt] | l | (spare).  16 np^2 + 16 nt + 16 bytes, a multiple of 16.
struct SplitParams {
    const double* W; int n, np, nt, n_sets, K;
    double scale;
    char* work; size_t work_stride;         // bytes
    double* radius; int* status;
};
__host__ __device__ inline size_t ss_work_bytes(int n) {
    const size_t np = (size_t)ss_padded(n), tiles = (np / SS_TILE) * (np / SS_TILE);
    return 16 * np * np + 16 * tiles + 16;
}
// orientation 0: the image by rows; 1: its transpose by rows.  plane 0: hi, 1: lo.
__device__ __forceinline__ ss_half* ss_plane(const SplitParams& p, int s, int image, int orient, int plane) {
    return reinterpret_cast<ss_half*>(p.work + (size_t)s * p.work_stride) +
           (size_t)((image * 2 + orient) * 2 + plane) * p.np * p.np;
}
__device__ __forceinline__ double* ss_doubles(const SplitParams& p, int s) {
    return reinterpret_cast<double*>(p.work + (size_t)s * p.work_stride + (size_t)16 * p.np * p.np);
}
__device__ __forceinline__ double* ss_partials(const SplitParams& p, int s, int which) {
    return ss_doubles(p, s) + (size_t)which * p.nt;
}
__device__ __forceinline__ double* ss_state(const SplitParams& p, int s) { return ss_doubles(p, s) + (size_t)2 * p.nt; }

// sum over the workgroup in a fixed order (xor tree inside a wave, then the wave sums in ascending order)
__device__ __forceinline__ double ss_block_sum(double v, double* red, int tid) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < SS_NW; ++w) s += red[w];
    return s;
}
__device__ __forceinline__ double ss_norm2(const double* part, int nt, double* red, int tid) {
    double v = 0.0;
    for (int t = tid; t < nt; t += SS_NT) v += part[t];
    return ss_block_sum(v, red, tid);
}
__device__ __forceinline__ bool ss_usable(double f) { return f > 0.0 && f <= 1.7976931348623157e308; }

__device__ __forceinline__ void ss_split(float x, ss_half& hi, ss_half& lo) {
    hi = (ss_half)x;
    lo = (ss_half)((x - (float)hi) * SS_LO);
}

// launch 0a: |W|^2 per tile into partials 0
__global__ __launch_bounds__(SS_NT) void specrad_split_norm_kernel(SplitParams p) {
    __shared__ double red[SS_NW];
    const int s = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int tpr = p.np / SS_TILE, r0 = (tile / tpr) * SS_TILE, c0 = (tile % tpr) * SS_TILE;
    const double* W = p.W + (size_t)s * p.n * p.n;
    double acc = 0.0;
    for (int e = tid; e < SS_TILE * SS_TILE; e += SS_NT) {
        const int r = r0 + e / SS_TILE, c = c0 + e % SS_TILE;
        const double v = (r < p.n && c < p.n) ? W[(size_t)r * p.n + c] : 0.0;
        acc = fma(v, v, acc);
    }
    const double sum = ss_block_sum(acc, red, tid);
    if (tid == 0) ss_partials(p, s, 0)[tile] = sum;
}

// launch 0b: the split image of s W / f_0 (s A_0) into image 0, both orientations, padded with zeros; l_0 = ln f_0
__global__ __launch_bounds__(SS_NT) void specrad_split_init_kernel(SplitParams p) {
    __shared__ double red[SS_NW];
    const int s = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int np = p.np, tpr = np / SS_TILE, r0 = (tile / tpr) * SS_TILE, c0 = (tile % tpr) * SS_TILE;
    const double f = sqrt(ss_norm2(ss_partials(p, s, 0), p.nt, red, tid));
    const bool ok = ss_usable(f) && ss_usable(p.scale / f);
    const double c = ok ? p.scale / f : 0.0;
    if (tile == 0 && tid == 0) ss_state(p, s)[0] = ok ? log(f) : __builtin_nan("");
    const double* W = p.W + (size_t)s * p.n * p.n;
    ss_half* d_hi = ss_plane(p, s, 0, 0, 0);
    ss_half* d_lo = ss_plane(p, s, 0, 0, 1);
    ss_half* t_hi = ss_plane(p, s, 0, 1, 0);
    ss_half* t_lo = ss_plane(p, s, 0, 1, 1);
    for (int e = tid; e < SS_TILE * SS_TILE; e += SS_NT) {
        const int r = r0 + e / SS_TILE, col = c0 + e % SS_TILE;
        const double v = (r < p.n && col < p.n) ? W[(size_t)r * p.n + col] : 0.0;
        ss_half hi, lo;
        ss_split(ok ? (float)(v * c) : 0.0f, hi, lo);            // (0 * NaN must not reach the image)
        d_hi[(size_t)r * np + col] = hi; d_lo[(size_t)r * np + col] = lo;
        t_hi[(size_t)col * np + r] = hi; t_lo[(size_t)col * np + r] = lo;
    }
}

// launch k = 1..K: image (k-1)&1 -> image k&1.  v_mfma_f32_32x32x16_f16: lane l (r = l & 31, h = l >> 5) holds
// A[row r][k = 8h + j] and B[k = 8h + j][col r] in element j of its fragment; C register i is row
// (i & 3) + 8 (i >> 2) + 4h, column r.
__global__ __launch_bounds__(SS_NT) void specrad_split_square_kernel(SplitParams p, int k) {
    __shared__ __attribute__((aligned(16))) ss_half sm[4 * SS_PLANE];
    __shared__ double red[SS_NW];
    const int s = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6, lr = lane & 31, lh = lane >> 5;
    const int wr = wv >> 1, wc = wv & 1;
    const int np = p.np, tpr = np / SS_TILE, r0 = (tile / tpr) * SS_TILE, c0 = (tile % tpr) * SS_TILE;

    // 1 / (s f_{k-1}^2), the same bits in every workgroup of this matrix (image 0 holds s A_0: f = 1 there, and an
    // unusable f_0 has zeroed it); an unusable factor makes this image zero, hence every later f zero
    double n2 = 1.0;
    if (k > 1) n2 = ss_norm2(ss_partials(p, s, (k - 1) & 1), p.nt, red, tid);
    const double f = sqrt(n2), cinv = 1.0 / (p.scale * n2);
    const bool ok = ss_usable(f) && ss_usable(cinv);
    const double c = ok ? cinv : 0.0;
    if (k > 1 && tile == 0 && tid == 0) {
        double* st = ss_state(p, s);
        st[0] = 2.0 * st[0] + (ok ? log(f) : __builtin_nan(""));   // l_{k-1}
    }

    // staging: thread t brings 16-byte chunks (t & 3) and (t & 3) + 4 of row t >> 2 of each of the four planes
    const int srow = tid >> 2, sch = (tid & 3) * 8;
    const int src_img = (k - 1) & 1;
    const ss_half* g[4] = {ss_plane(p, s, src_img, 0, 0) + (size_t)(r0 + srow) * np + sch,
                           ss_plane(p, s, src_img, 0, 1) + (size_t)(r0 + srow) * np + sch,
                           ss_plane(p, s, src_img, 1, 0) + (size_t)(c0 + srow) * np + sch,
                           ss_plane(p, s, src_img, 1, 1) + (size_t)(c0 + srow) * np + sch};
    ss_half* st_at = sm + srow * SS_LD + sch;
    const ss_half* a_at = sm + (wr * 32 + lr) * SS_LD + 8 * lh;
    const ss_half* b_at = sm + 2 * SS_PLANE + (wc * 32 + lr) * SS_LD + 8 * lh;

    ss_f16v acc_hh, acc_x;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc_hh[i] = 0.0f; acc_x[i] = 0.0f; }

    ss_h8 stage[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        stage[q][0] = *reinterpret_cast<const ss_h8*>(g[q]);
        stage[q][1] = *reinterpret_cast<const ss_h8*>(g[q] + 32);
    }
    for (int k0 = 0; k0 < np; k0 += SS_KC) {
        __syncthreads();                                            // the previous chunk is read out
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            *reinterpret_cast<ss_h8*>(st_at + q * SS_PLANE) = stage[q][0];
            *reinterpret_cast<ss_h8*>(st_at + q * SS_PLANE + 32) = stage[q][1];
        }
        __syncthreads();
        if (k0 + SS_KC < np) {                                      // the next chunk travels while this one multiplies
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                stage[q][0] = *reinterpret_cast<const ss_h8*>(g[q] + k0 + SS_KC);
                stage[q][1] = *reinterpret_cast<const ss_h8*>(g[q] + k0 + SS_KC + 32);
            }
        }
#pragma unroll
        for (int kk = 0; kk < SS_KC; kk += 16) {
            const ss_h8 a_hi = *reinterpret_cast<const ss_h8*>(a_at + kk);
            const ss_h8 a_lo = *reinterpret_cast<const ss_h8*>(a_at + SS_PLANE + kk);
            const ss_h8 b_hi = *reinterpret_cast<const ss_h8*>(b_at + kk);
            const ss_h8 b_lo = *reinterpret_cast<const ss_h8*>(b_at + SS_PLANE + kk);
            acc_hh = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, acc_hh, 0, 0, 0);
            acc_x = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, acc_x, 0, 0, 0);
            acc_x = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, acc_x, 0, 0, 0);
        }
    }

    // epilogue: s B_k = [hi hi + 2^-11 (hi lo + lo hi)] / (s f_{k-1}^2), its norm partial, the split tile by rows and
    // by columns (registers 4g .. 4g + 3 are four consecutive rows: one 8-byte store into the transpose)
    ss_half* d_hi = ss_plane(p, s, k & 1, 0, 0);
    ss_half* d_lo = ss_plane(p, s, k & 1, 0, 1);
    ss_half* t_hi = ss_plane(p, s, k & 1, 1, 0);
    ss_half* t_lo = ss_plane(p, s, k & 1, 1, 1);
    const int col = c0 + wc * 32 + lr, rbase = r0 + wr * 32 + 4 * lh;
    const double inv_s = 1.0 / p.scale;
    double part = 0.0;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        ss_h4 th, tl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * gq + j;
            const float x = (float)((double)(acc_hh[i] + acc_x[i] * (1.0f / SS_LO)) * c);
            const double b = (double)x * inv_s;
            part = fma(b, b, part);
            ss_half hi, lo;
            ss_split(x, hi, lo);
            th[j] = hi; tl[j] = lo;
            const size_t at = (size_t)(rbase + 8 * gq + j) * np + col;
            d_hi[at] = hi; d_lo[at] = lo;
        }
        const size_t tat = (size_t)col * np + rbase + 8 * gq;
        *reinterpret_cast<ss_h4*>(t_hi + tat) = th;
        *reinterpret_cast<ss_h4*>(t_lo + tat) = tl;
    }
    const double sum = ss_block_sum(part, red, tid);
    if (tid == 0) ss_partials(p, s, k & 1)[tile] = sum;
}

// last launch: one workgroup per matrix
__global__ __launch_bounds__(SS_NT) void specrad_split_final_kernel(SplitParams p) {
    __shared__ double red[SS_NW];
    const int s = blockIdx.x, tid = threadIdx.x;
    const double f = sqrt(ss_norm2(ss_partials(p, s, p.K & 1), p.nt, red, tid));
    if (tid == 0) {
        const double l = ss_state(p, s)[0];                         // l_{K-1}
        const double r = exp((l + log(f)) / (double)(1ull << (p.K - 1)));
        const bool ok = ss_usable(f) && ss_usable(r);               // (a NaN l fails the second test)
        p.radius[s] = ok ? r : 0.0;
        p.status[s] = ok ? 0 : 1;
    }
}

size_t specrad_split_work_bytes(int n_res) { return ss_work_bytes(n_res); }

int launch_spectral_radius_split(const double* W, int n_sets, int n_res, int n_squarings, double* radius, int* status,
                                 void* workspace, hipStream_t stream) {
    SplitParams p;
    p.W = W; p.n = n_res; p.np = ss_padded(n_res); p.nt = (p.np / SS_TILE) * (p.np / SS_TILE);
    p.n_sets = n_sets; p.K = n_squarings; p.scale = ss_scale(p.np);
    p.work = reinterpret_cast<char*>(workspace); p.work_stride = ss_work_bytes(n_res);
    p.radius = radius; p.status = status;
    // blockIdx.y carries the matrix: at most 65 535 per launch
    for (int s0 = 0; s0 < n_sets; s0 += 65535) {
        const int ns = n_sets - s0 < 65535 ? n_sets - s0 : 65535;
        SplitParams q = p;
        q.W = W + (size_t)s0 * n_res * n_res;
        q.work = p.work + (size_t)s0 * p.work_stride;
        q.radius = radius + s0; q.status = status + s0;
        const dim3 grid(p.nt, ns);
        hipLaunchKernelGGL(specrad_split_norm_kernel, grid, dim3(SS_NT), 0, stream, q);
        hipLaunchKernelGGL(specrad_split_init_kernel, grid, dim3(SS_NT), 0, stream, q);
        for (int k = 1; k <= n_squarings; ++k)
            hipLaunchKernelGGL(specrad_split_square_kernel, grid, dim3(SS_NT), 0, stream, q, k);
        hipLaunchKernelGGL(specrad_split_final_kernel, dim3(ns), dim3(SS_NT), 0, stream, q);
    }
    return (int)hipGetLastError();
}

}  // namespace esn
