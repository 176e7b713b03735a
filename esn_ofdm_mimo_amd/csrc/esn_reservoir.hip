// Reservoirs drawn on the device: the uniform draw of pyESN.py:93-109, the spectral radius and the
// rescale, for a batch of S independent weight sets.
//
//   gen_reservoirs_kernel     W = u - 0.5, zeroed where a second uniform < sparsity; W_in = 2u - 1; W_fb = 2u - 1.
//                             The uniforms are Philox4x32-10 keyed by (seed, global set, purpose, element), or the
//                             caller's (the reference's draw order), which makes the result bit-comparable with NumPy.
//   specrad_*_kernel          the spectral radius by repeated squaring, no eigensolver (|.| the Frobenius norm):
//                                 f_0 = |W|, A_0 = W / f_0, l_0 = ln f_0
//                                 k = 1..K:  B = A_{k-1} A_{k-1};  f_k = |B|;  l_k = 2 l_{k-1} + ln f_k;  A_k = B / f_k
//                                 radius = exp((l_{K-1} + ln f_K) / 2^(K-1))
//   scale_reservoirs_kernel   W[s] *= rho / radius[s] where status[s] == 0
//
// One squaring is one launch of a batched tiled GEMM on v_mfma_f64_16x16x4_f64: a workgroup of four waves owns a
// 64 x 64 tile of B, a wave a 32 x 32 quarter of it (2 x 2 MFMA tiles), the operands of 32 contraction steps are
// staged in LDS.  The two images of a matrix ping-pong in the caller's workspace, zero-padded to a multiple of 64
// (zero rows and columns change neither products nor norms).  An image holds B un-normalised; 1 / f_k multiplies
// the operands when the NEXT launch stages them.  |B|^2 leaves a launch as one partial sum per tile, and every
// workgroup of the next launch adds the partials of its matrix in the same fixed order: no floating-point atomics,
// and a matrix's radius is bitwise the same alone and inside any batch (the grid of a matrix depends on n alone).
//
// Self-contained on purpose, as esn_loo.hip is: the Philox rounds and the MFMA operand layout repeat what esn_gen.hip
// and esn_recur_f64_mfma.hip do, and no existing kernel is routed through a shared header.
#include "esn_common.h"
#include "esn_launch.h"

namespace esn {

constexpr int SR_TILE = 64;                 // workgroup tile of B, and the padding unit of an image
constexpr int SR_KC = 32;                   // contraction steps staged per barrier pair
constexpr int SR_NT = 256;                  // threads: 4 waves, 2 x 2 over the tile
constexpr int SR_NW = SR_NT / 64;
constexpr int SR_LDA = SR_TILE + 1;         // A staging is k-major [SR_KC][SR_LDA]: odd stride, so the transposing store
                                            // of 16 consecutive k of one row lands in 16 different bank pairs
constexpr int SR_LDB = SR_TILE;             // B staging [SR_KC][SR_LDB], as it lies in memory
// LDS (doubles): A staging | B staging | reduction scratch [SR_NW]          33 056 B; the 160 VGPRs of the unrolled
// chunk, not LDS, hold the kernel to three workgroups per CU
constexpr int SR_OFF_B = SR_KC * SR_LDA;
constexpr int SR_OFF_R = SR_OFF_B + SR_KC * SR_LDB;
constexpr int SR_LDS_DOUBLES = SR_OFF_R + SR_NW;
static_assert(sizeof(double) * SR_LDS_DOUBLES <= 40 * 1024, "LDS must not be what limits the occupancy");

typedef double sr_f64x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int sr_padded(int n) { return (n + SR_TILE - 1) / SR_TILE * SR_TILE; }

// workspace of one matrix (doubles): image 0 | image 1 | partials 0 [nt] | partials 1 [nt] | l | (spare)
struct SpecradParams {
    const double* W; int n, np, nt, n_sets, K;
    double* work; size_t work_stride;
    double* radius; int* status;
};
__host__ __device__ inline size_t sr_work_doubles(int n) {
    const size_t np = (size_t)sr_padded(n), tiles = (np / SR_TILE) * (np / SR_TILE);
    return 2 * np * np + 2 * tiles + 2;
}
__device__ __forceinline__ double* sr_image(const SpecradParams& p, int s, int which) {
    return p.work + (size_t)s * p.work_stride + (size_t)which * p.np * p.np;
}
__device__ __forceinline__ double* sr_partials(const SpecradParams& p, int s, int which) {
    return p.work + (size_t)s * p.work_stride + (size_t)2 * p.np * p.np + (size_t)which * p.nt;
}
__device__ __forceinline__ double* sr_state(const SpecradParams& p, int s) {
    return p.work + (size_t)s * p.work_stride + (size_t)2 * p.np * p.np + (size_t)2 * p.nt;
}

// sum over the workgroup in a fixed order (xor tree inside a wave, then the wave sums in ascending order); every
// thread gets the sum.  red: SR_NW doubles nobody else uses until the next call.
__device__ __forceinline__ double sr_block_sum(double v, double* red, int tid) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < SR_NW; ++w) s += red[w];
    return s;
}

// |image|^2 from the per-tile partials: thread t adds partials t, t + 256, ... in ascending order, then the block sum
__device__ __forceinline__ double sr_norm2(const double* part, int nt, double* red, int tid) {
    double v = 0.0;
    for (int t = tid; t < nt; t += SR_NT) v += part[t];
    return sr_block_sum(v, red, tid);
}

__device__ __forceinline__ bool sr_usable(double f) { return f > 0.0 && f <= 1.7976931348623157e308; }

// launch 0: W into image 0 (padded with zeros), |W|^2 per tile into partials 0
__global__ __launch_bounds__(SR_NT) void specrad_init_kernel(SpecradParams p) {
    __shared__ double red[SR_NW];
    const int s = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int tpr = p.np / SR_TILE, r0 = (tile / tpr) * SR_TILE, c0 = (tile % tpr) * SR_TILE;
    const double* W = p.W + (size_t)s * p.n * p.n;
    double* img = sr_image(p, s, 0);
    double acc = 0.0;
    for (int e = tid; e < SR_TILE * SR_TILE; e += SR_NT) {
        const int r = r0 + e / SR_TILE, c = c0 + e % SR_TILE;
        const double v = (r < p.n && c < p.n) ? W[(size_t)r * p.n + c] : 0.0;
        img[(size_t)r * p.np + c] = v;
        acc = fma(v, v, acc);
    }
    const double sum = sr_block_sum(acc, red, tid);
    if (tid == 0) sr_partials(p, s, 0)[tile] = sum;
}

// launch k = 1..K: image (k-1)&1 -> image k&1.  v_mfma_f64_16x16x4_f64: lane l holds A[l%16][l/16] and B[l/16][l%16];
// C register i is row 4i + l/16, column l%16.
__global__ __launch_bounds__(SR_NT) void specrad_square_kernel(SpecradParams p, int k) {
    __shared__ __attribute__((aligned(16))) double sm[SR_LDS_DOUBLES];
    double* As = sm;
    double* Bs = sm + SR_OFF_B;
    double* red = sm + SR_OFF_R;
    const int s = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int wr = wv >> 1, wc = wv & 1;
    const int np = p.np, tpr = np / SR_TILE, r0 = (tile / tpr) * SR_TILE, c0 = (tile % tpr) * SR_TILE;
    const double* src = sr_image(p, s, (k - 1) & 1);
    double* dst = sr_image(p, s, k & 1);

    // f_{k-1}, the same bits in every workgroup of this matrix; an unusable one (zero, infinite, NaN) makes the
    // operands zero, hence every later f zero: the matrix stays flagged and never disturbs a neighbour
    const double f = sqrt(sr_norm2(sr_partials(p, s, (k - 1) & 1), p.nt, red, tid));
    const bool ok = sr_usable(f);
    const double inv = ok ? 1.0 / f : 0.0;
    if (tile == 0 && tid == 0) {
        double* st = sr_state(p, s);
        const double lf = ok ? log(f) : __builtin_nan("");
        st[0] = (k == 1) ? lf : 2.0 * st[0] + lf;                  // l_{k-1}
    }

    sr_f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = sr_f64x4{0.0, 0.0, 0.0, 0.0};

    for (int k0 = 0; k0 < np; k0 += SR_KC) {
        __syncthreads();                                            // the previous chunk is read out
#pragma unroll
        for (int q = 0; q < SR_TILE * SR_KC / SR_NT; ++q) {
            const int e = tid + SR_NT * q;
            const int ar = e / SR_KC, ak = e % SR_KC;               // 32 consecutive k of one row of the row tile
            As[ak * SR_LDA + ar] = src[(size_t)(r0 + ar) * np + k0 + ak] * inv;
            const int bk = e / SR_TILE, bc = e % SR_TILE;           // 64 consecutive columns of one k
            Bs[bk * SR_LDB + bc] = src[(size_t)(k0 + bk) * np + c0 + bc] * inv;
        }
        __syncthreads();
        const double* a0 = As + lq * SR_LDA + wr * 32 + lr;
        const double* b0 = Bs + lq * SR_LDB + wc * 32 + lr;
#pragma unroll
        for (int k4 = 0; k4 < SR_KC; k4 += 4) {
            const double a[2] = {a0[k4 * SR_LDA], a0[k4 * SR_LDA + 16]};
            const double b[2] = {b0[k4 * SR_LDB], b0[k4 * SR_LDB + 16]};
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }

    double part = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = acc[i][j][r];
                dst[(size_t)(r0 + wr * 32 + i * 16 + 4 * r + lq) * np + c0 + wc * 32 + j * 16 + lr] = v;
                part = fma(v, v, part);
            }
    const double sum = sr_block_sum(part, red, tid);
    if (tid == 0) sr_partials(p, s, k & 1)[tile] = sum;
}

// last launch: one workgroup per matrix
__global__ __launch_bounds__(SR_NT) void specrad_final_kernel(SpecradParams p) {
    __shared__ double red[SR_NW];
    const int s = blockIdx.x, tid = threadIdx.x;
    const double f = sqrt(sr_norm2(sr_partials(p, s, p.K & 1), p.nt, red, tid));
    if (tid == 0) {
        const double l = sr_state(p, s)[0];                         // l_{K-1}
        const double r = exp((l + log(f)) / (double)(1ull << (p.K - 1)));
        const bool ok = sr_usable(f) && sr_usable(r);               // (a NaN l fails the second test)
        p.radius[s] = ok ? r : 0.0;
        p.status[s] = ok ? 0 : 1;
    }
}

size_t specrad_work_doubles(int n_res) { return sr_work_doubles(n_res); }

int launch_spectral_radius(const double* W, int n_sets, int n_res, int n_squarings, double* radius, int* status,
                           void* workspace, hipStream_t stream) {
    SpecradParams p;
    p.W = W; p.n = n_res; p.np = sr_padded(n_res); p.nt = (p.np / SR_TILE) * (p.np / SR_TILE);
    p.n_sets = n_sets; p.K = n_squarings;
    p.work = reinterpret_cast<double*>(workspace); p.work_stride = sr_work_doubles(n_res);
    p.radius = radius; p.status = status;
    // blockIdx.y carries the matrix: at most 65 535 per launch
    for (int s0 = 0; s0 < n_sets; s0 += 65535) {
        const int ns = n_sets - s0 < 65535 ? n_sets - s0 : 65535;
        SpecradParams q = p;
        q.W = W + (size_t)s0 * n_res * n_res;
        q.work = p.work + (size_t)s0 * p.work_stride;
        q.radius = radius + s0; q.status = status + s0;
        const dim3 grid(p.nt, ns);
        hipLaunchKernelGGL(specrad_init_kernel, grid, dim3(SR_NT), 0, stream, q);
        for (int k = 1; k <= n_squarings; ++k)
            hipLaunchKernelGGL(specrad_square_kernel, grid, dim3(SR_NT), 0, stream, q, k);
        hipLaunchKernelGGL(specrad_final_kernel, dim3(ns), dim3(SR_NT), 0, stream, q);
    }
    return (int)hipGetLastError();
}

// ---- the draw ------------------------------------------------------------------------------------------------------
struct ResPhilox {
    uint32_t k0, k1;
    __device__ __forceinline__ void round(uint32_t (&c)[4], uint32_t ka, uint32_t kb) const {
        const uint64_t p0 = (uint64_t)0xD2511F53U * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57U * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ ka;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ kb;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
    }
    __device__ __forceinline__ void operator()(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                               uint32_t (&out)[4]) const {
        uint32_t c[4] = {c0, c1, c2, c3};
        uint32_t ka = k0, kb = k1;
#pragma unroll
        for (int i = 0; i < 10; ++i) { round(c, ka, kb); ka += 0x9E3779B9U; kb += 0xBB67AE85U; }
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = c[i];
    }
};

// 53-bit uniform in [0, 1) from two words, as NumPy's random_sample builds it
__device__ __forceinline__ double res_uniform(uint32_t a, uint32_t b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

// purposes 1-3 are esn_gen.hip's (bits, noise, taps): these keep clear of them
enum { RES_PURPOSE_W = 16, RES_PURPOSE_WIN = 17, RES_PURPOSE_WFB = 18 };

struct ResGenParams {
    int n, n_in, n_out, n_sets;
    double sparsity;
    uint64_t seed, first_set;
    const double* uniforms;
    double* W; double* W_in; double* W_fb;
};

// grid (blocks over the elements of one set, sets); element e of set i: W for e < n^2, then W_in, then W_fb
__global__ __launch_bounds__(256) void gen_reservoirs_kernel(ResGenParams p) {
    const int i = blockIdx.y;
    const uint64_t gs = p.first_set + (uint64_t)i;
    const size_t slot = (size_t)(gs % (uint64_t)p.n_sets);
    const size_t nn = (size_t)p.n * p.n, nin = (size_t)p.n * p.n_in, nout = (size_t)p.n * p.n_out;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nn + nin + nout) return;
    const ResPhilox ph{(uint32_t)p.seed, (uint32_t)(p.seed >> 32)};
    const double* u = p.uniforms ? p.uniforms + (size_t)i * (2 * nn + nin + nout) : nullptr;
    uint32_t w[4];
    if (e < nn) {
        double uv, um;
        if (u) { uv = u[e]; um = u[nn + e]; }
        else {
            ph((uint32_t)gs, (uint32_t)(gs >> 32), RES_PURPOSE_W, (uint32_t)e, w);
            uv = res_uniform(w[0], w[1]); um = res_uniform(w[2], w[3]);
        }
        p.W[slot * nn + e] = (um < p.sparsity) ? 0.0 : uv - 0.5;
    } else if (e < nn + nin) {
        const size_t j = e - nn;
        double uv;
        if (u) uv = u[2 * nn + j];
        else { ph((uint32_t)gs, (uint32_t)(gs >> 32), RES_PURPOSE_WIN, (uint32_t)j, w); uv = res_uniform(w[0], w[1]); }
        p.W_in[slot * nin + j] = uv * 2.0 - 1.0;
    } else {
        const size_t j = e - nn - nin;
        double uv;
        if (u) uv = u[2 * nn + nin + j];
        else { ph((uint32_t)gs, (uint32_t)(gs >> 32), RES_PURPOSE_WFB, (uint32_t)j, w); uv = res_uniform(w[0], w[1]); }
        p.W_fb[slot * nout + j] = uv * 2.0 - 1.0;
    }
}

int launch_gen_reservoirs(int n_res, int n_in, int n_out, double sparsity, uint64_t seed, uint64_t first_set,
                          int n_sets, const double* uniforms, double* W, double* W_in, double* W_fb,
                          hipStream_t stream) {
    ResGenParams p;
    p.n = n_res; p.n_in = n_in; p.n_out = n_out; p.n_sets = n_sets; p.sparsity = sparsity;
    p.seed = seed; p.first_set = first_set; p.uniforms = uniforms; p.W = W; p.W_in = W_in; p.W_fb = W_fb;
    const size_t per_set = (size_t)n_res * ((size_t)n_res + n_in + n_out);
    const unsigned bx = (unsigned)((per_set + 255) / 256);
    for (int s0 = 0; s0 < n_sets; s0 += 65535) {
        const int ns = n_sets - s0 < 65535 ? n_sets - s0 : 65535;
        ResGenParams q = p;
        q.first_set = first_set + (uint64_t)s0;
        if (uniforms) q.uniforms = uniforms + (size_t)s0 * (per_set + (size_t)n_res * n_res);
        hipLaunchKernelGGL(gen_reservoirs_kernel, dim3(bx, ns), dim3(256), 0, stream, q);
    }
    return (int)hipGetLastError();
}

// ---- the rescale ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scale_reservoirs_kernel(double* W, size_t nn, double rho, const double* radius,
                                                               const int* status) {
    const int s = blockIdx.y;
    if (status[s] != 0) return;                                     // a flagged set is left unscaled
    const double c = rho / radius[s];
    double* w = W + (size_t)s * nn;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nn; e += (size_t)gridDim.x * blockDim.x)
        w[e] *= c;
}

int launch_scale_reservoirs(double* W, int n_sets, int n_res, double rho, const double* radius, const int* status,
                            hipStream_t stream) {
    const size_t nn = (size_t)n_res * n_res;
    const unsigned bx = (unsigned)((nn + 255) / 256 < 1024 ? (nn + 255) / 256 : 1024);
    for (int s0 = 0; s0 < n_sets; s0 += 65535) {
        const int ns = n_sets - s0 < 65535 ? n_sets - s0 : 65535;
        hipLaunchKernelGGL(scale_reservoirs_kernel, dim3(bx, ns), dim3(256), 0, stream, W + (size_t)s0 * nn, nn, rho,
                           radius + s0, status + s0);
    }
    return (int)hipGetLastError();
}

}  // namespace esn
