// The arithmetic the OFDM kernels share, each piece written once:
//   * the radix-2 decimation-in-time transform in LDS on bit-reversed rows (twiddle table, the stage bodies, the driver):
//       esn_detect.hip   detect_count_kernel, X = FFT_N(y) / (N sqrt(Pi))   (the fixed-shape
//                        instances use det_bfly / det_twiddle on their own lane map)
//       esn_remod.hip    the forward pass of detect_remod_kernel (its decimation-in-frequency inverse takes the stage
//                        indices from here and keeps its own butterfly)
//       esn_chantrack.hip, esn_baseline.hip (channel_estimate_kernel, mmse_detect_kernel)
//       esn_equalize.hip mmse_equalize_rows_kernel: the spectrum of mmse_detect_kernel (esn_mmse_solve.h) and, on the
//                        conjugated solution with the same table, N IFFT_N(X) = conj(FFT_N(conj X))
//       esn_dcc.hip      mmse_dcc_kernel: that spectrum, and per cancellation pass the same pair of transforms on the
//                        decisions and on the amplifier's predicted distortion
//       esn_gen.hip      gen_frames_kernel, x = N IFFT_N(X): the conjugate table
//   * the unit-power square QAM grid (norm, slicer, level, bits <-> index): the above and qam_llr_kernel (esn_coded.hip);
//     the max-log distance of one axis (qam_axis_llr): the soft kernels of esn_soft.hip
//   * the error-counter tail of the generic kernels (detect, remod, mmse)
//   * H[k] = sum_j c[j] exp(-2 pi i jk / N): channel_estimate_kernel, taps_to_freq_kernel
// The library is built with -ffp-contract=off: every product and sum below is rounded on its own, so kernels that go
// through these functions compile the same operations on the same operands and their spectra, indices and counters are
// bit-identical -- whichever thread computes a butterfly, and whether the stages are taken one or two at a time.  The
// multiplications by the twiddles (1, -0) and (0, -1) stay: dropping them flips signed zeros.
#pragma once
#include "esn_common.h"

namespace esn {

__device__ __forceinline__ void det_bfly(double2& a, double2& c, const double2 w) {
    const double tr = c.x * w.x - c.y * w.y, ti = c.x * w.y + c.y * w.x;
    const double2 a0 = a;
    a = make_double2(a0.x + tr, a0.y + ti);
    c = make_double2(a0.x - tr, a0.y - ti);
}
// exp(sign 2 pi i k / N): sign -1.0 the forward transform, +1.0 its conjugate (same sincospi magnitude argument)
__device__ __forceinline__ double2 det_twiddle(int k, int N, double sign = -1.0) {
    double sn, cs;
    sincospi(sign * 2.0 * (double)k / (double)N, &sn, &cs);
    return make_double2(cs, sn);
}
// tw[0 .. count) = exp(sign 2 pi i k / N), by the whole workgroup; a barrier must follow before the table is read
__device__ __forceinline__ void ofdm_twiddles(double2* tw, int count, int N, double sign) {
    for (int k = threadIdx.x; k < count; k += blockDim.x) tw[k] = det_twiddle(k, N, sign);
}

// Stage s = 1 .. log2 N pairs position x with x + hm, hm = 2^(s-1), under the twiddle tw[(x mod hm) N / 2^s].
// Butterfly t < N/2 of stage s: positions base, base + hm, twiddle tw[k]
struct OfdmPair { int base, hm, k; };
__device__ __forceinline__ OfdmPair ofdm_pair(int t, int s, int N) {
    const int hm = 1 << (s - 1), j = t & (hm - 1);
    return {((t >> (s - 1)) << s) + j, hm, j * (N >> s)};
}
// Quad t < N/4 of stages s and s + 1: positions base + {0, 1, 2, 3} hm; stage s pairs (0, 1) and (2, 3) under tw[k1],
// stage s + 1 pairs (0, 2) under tw[k2] and (1, 3) under tw[k3]
struct OfdmQuad { int base, hm, k1, k2, k3; };
__device__ __forceinline__ OfdmQuad ofdm_quad(int t, int s, int N) {
    const int hm = 1 << (s - 1), j = t & (hm - 1), ts2 = N >> (s + 1);
    return {((t >> (s - 1)) << (s + 1)) + j, hm, j * (N >> s), j * ts2, (j + hm) * ts2};
}
__device__ __forceinline__ void ofdm_stage(double2* b, const double2* tw, int N, int s, int t) {
    const OfdmPair p = ofdm_pair(t, s, N);
    double2 a = b[p.base], c = b[p.base + p.hm];
    det_bfly(a, c, tw[p.k]);
    b[p.base] = a; b[p.base + p.hm] = c;
}
// the same butterflies in the same order as two single stages, on four points in registers: half the LDS round trips
__device__ __forceinline__ void ofdm_stage_pair(double2* b, const double2* tw, int N, int s, int t) {
    const OfdmQuad q = ofdm_quad(t, s, N);
    double2 p0 = b[q.base], p1 = b[q.base + q.hm], p2 = b[q.base + 2 * q.hm], p3 = b[q.base + 3 * q.hm];
    const double2 w1 = tw[q.k1];
    det_bfly(p0, p1, w1);
    det_bfly(p2, p3, w1);
    det_bfly(p0, p2, tw[q.k2]);
    det_bfly(p1, p3, tw[q.k3]);
    b[q.base] = p0; b[q.base + q.hm] = p1; b[q.base + 2 * q.hm] = p2; b[q.base + 3 * q.hm] = p3;
}
// In place, un-normalised: `rows` rows of N points, stride ld, already in bit-reversed order; tw[N/2] from
// ofdm_twiddles (sign -1.0: the DFT, +1.0: N times its inverse).  The whole workgroup calls it, after a barrier behind
// the writes of the rows and the table; it ends behind a barrier.  Work item e = (row, t) = (e / (N/4), e mod (N/4)),
// strided by the workgroup: at N = 128 that is 32 threads per row.
__device__ __forceinline__ void ofdm_fft_lds(double2* buf, int rows, int ld, const double2* tw, int N, int log2n) {
    int s = 1;
    for (; s + 1 <= log2n; s += 2) {
        for (int e = threadIdx.x; e < rows << (log2n - 2); e += blockDim.x)
            ofdm_stage_pair(buf + (size_t)(e >> (log2n - 2)) * ld, tw, N, s, e & ((N >> 2) - 1));
        __syncthreads();
    }
    if (s <= log2n) {                                        // odd number of stages: the last one alone
        for (int e = threadIdx.x; e < rows << (log2n - 1); e += blockDim.x)
            ofdm_stage(buf + (size_t)(e >> (log2n - 1)) * ld, tw, N, s, e & ((N >> 1) - 1));
        __syncthreads();
    }
}

// ---- the unit-power square QAM grid: side levels per axis, index = i side + j (Re level i, Im level j), natural
// binary, LSB first
__device__ __forceinline__ double det_norm(int side) { return sqrt(2.0 * (double)(side * side - 1) / 3.0); }
__device__ __forceinline__ double det_scale(int N, double p_i_g) { return 1.0 / ((double)N * sqrt(p_i_g)); }
__device__ __forceinline__ int det_slice(double v, double norm, int side) {   // index of the nearest grid level
    const int i = (int)rint((v * norm + (double)(side - 1)) * 0.5);
    return min(max(i, 0), side - 1);
}
__device__ __forceinline__ double det_level(int i, int side, double norm) {  // level i of the grid
    return (double)(2 * i - (side - 1)) / norm;
}
// lev[a] = det_level(a), a < side (side <= 32), by the whole workgroup; a barrier must follow before the table is read
__device__ __forceinline__ void qam_levels(double* lev, int side, double norm) {
    for (int a = threadIdx.x; a < side; a += blockDim.x) lev[a] = det_level(a, side, norm);
}
// max-log distance difference d1 - d0 of bit bb of one axis at coordinate t: d1 / d0 the smallest squared distance to a
// level whose index has bit bb set / clear (the operations of qam_llr_kernel on the levels of qam_levels -- the division
// by norm is taken once per workgroup, not once per level and bit; positive = bit 0 is nearer)
__device__ __forceinline__ double qam_axis_llr(double t, int bb, int side, const double* lev) {
    double d0 = 1e300, d1 = 1e300;
    for (int a = 0; a < side; ++a) {
        const double d = t - lev[a];
        const double dd = d * d;
        if ((a >> bb) & 1) d1 = fmin(d1, dd); else d0 = fmin(d0, dd);
    }
    return d1 - d0;
}
// index of the m bits b[0], b[stride], ..
__device__ __forceinline__ int det_bits_index(const uint8_t* b, size_t stride, int m) {
    int idx = 0;
    for (int bb = 0; bb < m; ++bb) idx |= (int)(b[bb * stride] & 1) << bb;
    return idx;
}
// how many of the m bits of idx differ from tb[0], tb[stride], ..
__device__ __forceinline__ int det_bit_errors(int idx, const uint8_t* tb, size_t stride, int m) {
    int errs = 0;
    for (int bb = 0; bb < m; ++bb) errs += (((idx >> bb) & 1) != (int)tb[bb * stride]);
    return errs;
}

// The workgroup's error count and its n_bits into the group's two counters: shuffle-reduce per wave, one slot of red[]
// (LDS, one int per wave) each, thread 0 adds.  The whole workgroup calls it; it passes one barrier, which is all it
// does where `count` (uniform) is false.
__device__ __forceinline__ void det_count_tail(bool count, int errs, int* red, long long* err, long long* bits, int n_bits) {
    if (count) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) errs += __shfl_down(errs, off);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = errs;
    }
    __syncthreads();
    if (count && threadIdx.x == 0) {
        int e = 0;
        for (int w = 0; w < (int)((blockDim.x + 63) >> 6); ++w) e += red[w];
        atomicAdd(reinterpret_cast<unsigned long long*>(err), (unsigned long long)e);
        atomicAdd(reinterpret_cast<unsigned long long*>(bits), (unsigned long long)n_bits);
    }
}

// sum_{j < n} c(j) exp(sign2 pi i jk / N), sign2 = -2.0 or +2.0, terms added in order of j; c(j) returns a double2
template <class Coef>
__device__ __forceinline__ double2 ofdm_dft_point(Coef c, int n, int k, int N, double sign2) {
    double hr = 0.0, hi = 0.0;
    for (int j = 0; j < n; ++j) {
        double sn, cs;
        sincospi(sign2 * (double)((j * k) % N) / (double)N, &sn, &cs);
        const double2 v = c(j);
        hr += v.x * cs - v.y * sn;
        hi += v.x * sn + v.y * cs;
    }
    return make_double2(hr, hi);
}

}  // namespace esn
