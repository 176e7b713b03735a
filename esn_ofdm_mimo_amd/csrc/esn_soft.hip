// SINR-weighted soft outputs for the coded leg behind the LS-MMSE equaliser, float64:
//   mmse_sinr_kernel          per block g, subcarrier k, stream i, with lam = No / Pi[g]:
//                               t = lam [(H_k^H H_k + lam I)^-1]_ii clamped to [1e-12, 1 - 1e-12]  (mmse_sinr_point)
//                               mu = 1 - t (bias), gamma = (1 - t) / t (SINR), w = gamma / mean_g(gamma)
//   qam_llr_weighted_kernel   sigma^2_f of qam_llr_kernel (esn_coded.hip: same thread count, same element order, so the
//                             same bits), then LLR = w (d1 - d0)(x / mu) / sigma^2_f in the decoder's layout
//   detect_llr_kernel         the fused soft tail of the ESN leg: the transform, slicer and counters of
//                             detect_count_kernel (esn_detect.hip), then sigma^2_f and the weighted LLRs from the
//                             spectrum in LDS -- X_hat goes to memory only where it is asked for
// w and mu are 1 where their pointer is null: x / 1.0 and 1.0 * llr are exact, so the flat LLRs are those of qam_llr_kernel.
#include "esn_common.h"
#include "esn_launch.h"
#include "esn_mmse_solve.h"
#include "esn_ofdm_math.h"

namespace esn {

constexpr int kSoftThreads = 256;    // qam_llr_kernel's: the sigma^2 sums below are its sums, term for term

// One workgroup per block.  gamma is summed per thread over its subcarriers (k = tid, tid + 256, ..; streams in order),
// then over the wave by shuffles and over the four waves in order: the order depends on the shape alone.
__global__ __launch_bounds__(kSoftThreads) void mmse_sinr_kernel(SinrParams sp) {
    __shared__ double red[kSoftThreads / 64];
    __shared__ double s_mean;
    const int N = sp.n_sub, n_t = sp.n_t, n_r = sp.n_r, tid = threadIdx.x, nth = blockDim.x;
    const size_t blk = blockIdx.x;
    const double lam = sp.no / sp.p_i[blk];
    double part = 0.0;
    for (int k = tid; k < N; k += nth) {
        double t[MMSE_NT];
        mmse_sinr_point(sp.H + ((blk * N + k) * n_r) * n_t * 2, n_t, n_r, lam, t);
#pragma unroll
        for (int tx = 0; tx < MMSE_NT; ++tx) {
            if (tx >= n_t) continue;
            const double tc = fmin(fmax(t[tx], 1e-12), 1.0 - 1e-12);   // (a NaN leaves the lower clamp)
            const double mu = 1.0 - tc, gamma = mu / tc;
            sp.mu[(blk * N + k) * n_t + tx] = mu;
            sp.w[(blk * N + k) * n_t + tx] = gamma;
            part += gamma;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off);
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < (int)(nth >> 6); ++w) s += red[w];
        s_mean = s / (double)(N * n_t);
        if (sp.gamma_mean) sp.gamma_mean[blk] = s_mean;
    }
    __syncthreads();
    const double mean = s_mean;
    for (int k = tid; k < N; k += nth)                        // every thread re-reads what it wrote itself
        for (int tx = 0; tx < n_t; ++tx) sp.w[(blk * N + k) * n_t + tx] /= mean;
}

// |x - nearest grid point|^2, the term qam_llr_kernel sums; lev: the levels of qam_levels (LDS)
__device__ __forceinline__ double soft_dd_term(double re, double im, double norm, int side, const double* lev) {
    const double dr = re - lev[det_slice(re, norm, side)];
    const double di = im - lev[det_slice(im, norm, side)];
    return dr * dr + di * di;
}
// the per-thread sums `part` of a workgroup of kSoftThreads -> sigma^2 of the frame (to sigma2_out if given), by
// qam_llr_kernel's shuffles and wave order.  The whole workgroup calls it; it passes two barriers.
__device__ __forceinline__ double soft_sigma2(double part, int n_el, double* red, double* s_sigma2, double* sigma2_out) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off);
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
        *s_sigma2 = s / (double)n_el + 1e-12;
        if (sigma2_out) *sigma2_out = *s_sigma2;
    }
    __syncthreads();
    return *s_sigma2;
}
// the m LLRs of one point: bits [0, half) are those of the Im axis, [half, m) those of the Re axis (index = i side + j)
__device__ __forceinline__ void soft_llr_point(double re, double im, double wv, double muv, double inv, int m, int side,
                                               const double* lev, double* out) {
    const int half = m / 2;
    re = re / muv; im = im / muv;
    for (int b = 0; b < m; ++b) {
        const double t = (b < half) ? im : re;
        out[b] = wv * (qam_axis_llr(t, (b < half) ? b : b - half, side, lev) * inv);
    }
}

__global__ __launch_bounds__(kSoftThreads) void qam_llr_weighted_kernel(SoftLlrParams sp) {
    __shared__ double red[kSoftThreads / 64];
    __shared__ double s_sigma2;
    __shared__ double lev[32];
    const LlrParams& lp = sp.l;
    const int N = lp.n_sub, n_t = lp.n_t, m = lp.m, side = 1 << (m / 2);
    const double norm = det_norm(side);
    const int frame = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    const double* x = lp.X_hat + (size_t)frame * N * n_t * 2;
    const size_t wb = (size_t)(frame / sp.frames_per_group) * N * n_t;
    qam_levels(lev, side, norm);
    __syncthreads();
    double part = 0.0;
    for (int e = tid; e < N * n_t; e += nth) part += soft_dd_term(x[2 * e], x[2 * e + 1], norm, side, lev);
    const double s2 = soft_sigma2(part, N * n_t, red, &s_sigma2, lp.sigma2 ? lp.sigma2 + frame : nullptr);
    const double inv = 1.0 / fmax(s2, 1e-12);
    for (int e = tid; e < N * n_t; e += nth) {
        const int sc = e / n_t, tx = e % n_t;
        soft_llr_point(x[2 * e], x[2 * e + 1], sp.w ? sp.w[wb + e] : 1.0, sp.mu ? sp.mu[wb + e] : 1.0, inv, m, side, lev,
                       lp.llr + ((size_t)(frame * n_t + tx) * N + sc) * m);
    }
}

// One workgroup of kSoftThreads per frame holds all n_t antennas (sigma^2_f spans them): rows [n_t][N + 1] and the
// twiddle table in LDS as in detect_count_kernel, whose operations these are up to the counters -- the spectrum does not
// depend on which thread computes a butterfly, so X_hat, err and bits are that kernel's bit for bit.  The sigma^2 terms
// are taken in qam_llr_kernel's element order (subcarrier, antenna fastest) by as many threads; the LLRs go out antenna
// by antenna, subcarrier fastest: consecutive threads write consecutive runs of m doubles of the decoder's layout.
template <bool IO32>
__global__ __launch_bounds__(kSoftThreads) void detect_llr_kernel(DetectLlrParams lp) {
    extern __shared__ __attribute__((aligned(16))) char ssm[];
    const DetectParams& dp = lp.d;
    const int N = dp.n_sub, n_t = dp.n_t, m = dp.m, tid = threadIdx.x, nthr = blockDim.x, half = N >> 1;
    const int ld = N + 1;
    double2* buf = reinterpret_cast<double2*>(ssm);          // [n_t][ld]
    double2* tw = buf + (size_t)n_t * ld;                    // [N/2]
    __shared__ int red[kSoftThreads / 64];
    __shared__ double dred[kSoftThreads / 64];
    __shared__ double s_sigma2;
    __shared__ double lev[32];
    const int frame = blockIdx.x, group = frame / dp.frames_per_group;
    const double2* y = reinterpret_cast<const double2*>(dp.Y) + (size_t)frame * N * n_t;
    const float2* y32 = reinterpret_cast<const float2*>(dp.Y32) + (size_t)frame * N * n_t;
    const bool count = dp.tx_bits != nullptr;

    // the 16 tx bytes of the subcarriers this thread will slice, fetched before the transform (detect_count_kernel)
    constexpr int TXP = 2;
    const bool tx_pre = count && m * n_t == 16 && N * n_t <= TXP * nthr && ((uintptr_t)dp.tx_bits & 15) == 0;
    uint4 txw[TXP];
    if (tx_pre) {
#pragma unroll
        for (int q = 0; q < TXP; ++q) {
            const int e = tid + q * nthr, k = e / n_t;
            txw[q] = (e < N * n_t) ? *reinterpret_cast<const uint4*>(dp.tx_bits + ((size_t)frame * N + k) * 16) : uint4{0, 0, 0, 0};
        }
    }
    const double p_i_g = dp.p_i[group];
    const int side = 1 << (m / 2);
    const double norm = det_norm(side);
    qam_levels(lev, side, norm);
    ofdm_twiddles(tw, half, N, -1.0);
    for (int i = tid; i < N * n_t; i += nthr) {
        const int row = i / n_t, ant = i - row * n_t;
        const int rv = (int)(__brev((unsigned)row) >> (32 - dp.log2n));
        if constexpr (IO32) {
            const float2 v = y32[i];
            buf[ant * ld + rv] = make_double2((double)v.x, (double)v.y);
        } else {
            buf[ant * ld + rv] = y[i];
        }
    }
    __syncthreads();
    ofdm_fft_lds(buf, n_t, ld, tw, N, dp.log2n);

    const double scale = det_scale(N, p_i_g);
    int errs = 0;
    double part = 0.0;
    for (int e = tid; e < N * n_t; e += nthr) {               // element e = (subcarrier k, antenna), antenna fastest
        const int k = e / n_t, ant = e - k * n_t;
        const double2 v = buf[ant * ld + k];
        const double re = v.x * scale, im = v.y * scale;
        if (dp.X_hat) reinterpret_cast<double2*>(dp.X_hat)[(size_t)frame * N * n_t + e] = make_double2(re, im);
        part += soft_dd_term(re, im, norm, side, lev);
        if (!count) continue;
        const int idx = det_slice(re, norm, side) * side + det_slice(im, norm, side);
        if (tx_pre) {                                        // byte bb n_t + ant of the subcarrier's 16
            const uint4 w = (e - tid) / nthr == 0 ? txw[0] : txw[1];
            for (int bb = 0; bb < m; ++bb) {
                const int byte = bb * n_t + ant, q = byte >> 2;
                const uint32_t word = q == 0 ? w.x : q == 1 ? w.y : q == 2 ? w.z : w.w;
                errs += (int)(((uint32_t)(idx >> bb) & 1u) != ((word >> (8 * (byte & 3))) & 0xffu));
            }
        } else {
            errs += det_bit_errors(idx, dp.tx_bits + ((size_t)frame * N + k) * m * n_t + ant, n_t, m);
        }
    }
    det_count_tail(count, errs, red, dp.err + group, dp.bits + group, N * m * n_t);
    const double s2 = soft_sigma2(part, N * n_t, dred, &s_sigma2, lp.sigma2 ? lp.sigma2 + frame : nullptr);
    const double inv = 1.0 / fmax(s2, 1e-12);
    const size_t wb = (size_t)group * N * n_t;
    double* out = lp.llr + (size_t)frame * n_t * N * m;
    for (int e = tid; e < N * n_t; e += nthr) {               // element e = (antenna, subcarrier k), subcarrier fastest
        const int ant = e / N, k = e - ant * N;
        const double2 v = buf[ant * ld + k];
        const size_t wi = wb + (size_t)k * n_t + ant;
        soft_llr_point(v.x * scale, v.y * scale, lp.w ? lp.w[wi] : 1.0, lp.mu ? lp.mu[wi] : 1.0, inv, m, side, lev,
                       out + (size_t)e * m);
    }
}

int launch_mmse_sinr(const SinrParams& sp, hipStream_t stream) {
    if (sp.n_t > MMSE_NT) return -1;
    hipLaunchKernelGGL(mmse_sinr_kernel, dim3(sp.n_blocks), dim3(kSoftThreads), 0, stream, sp);
    return (int)hipGetLastError();
}

int launch_qam_llr_weighted(const SoftLlrParams& lp, hipStream_t stream) {
    hipLaunchKernelGGL(qam_llr_weighted_kernel, dim3(lp.l.n_frames), dim3(kSoftThreads), 0, stream, lp);
    return (int)hipGetLastError();
}

size_t detect_llr_lds_bytes(int n_sub, int n_t) {
    return sizeof(double2) * ((size_t)n_t * (n_sub + 1) + n_sub / 2);
}

int launch_detect_llr(const DetectLlrParams& lp, hipStream_t stream, bool io32) {
    const size_t lds = detect_llr_lds_bytes(lp.d.n_sub, lp.d.n_t);
    if (lds > MMSE_LDS_MAX) return -1;
    const void* kern = io32 ? reinterpret_cast<const void*>(detect_llr_kernel<true>)
                            : reinterpret_cast<const void*>(detect_llr_kernel<false>);
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    if (io32) hipLaunchKernelGGL(detect_llr_kernel<true>, dim3(lp.d.n_frames), dim3(kSoftThreads), lds, stream, lp);
    else hipLaunchKernelGGL(detect_llr_kernel<false>, dim3(lp.d.n_frames), dim3(kSoftThreads), lds, stream, lp);
    return (int)hipGetLastError();
}

}  // namespace esn
