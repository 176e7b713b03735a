// The float64 matrix-pipe products that the per-group trainings share (esn_cnn.hip, esn_lstm.hip): a workgroup of
// CNN_THREADS threads, a wave per strip of CNN_NB tiles of v_mfma_f64_16x16x4_f64 (A[l % 16][l / 16], B[l / 16][l % 16],
// C register i: row 4 i + l / 16, column l % 16) that share the A operand, operands straight from memory.  Parameters of
// a layer are kept as P [c_out][K + 1] with the bias as one more column, fed by a constant 1.  Sums run over the inner
// index in ascending groups of four, whatever wave takes the strip: every sum's order depends on the shape alone.
#pragma once
#include "esn_common.h"

namespace esn {

typedef double cnn_f64x4 __attribute__((ext_vector_type(4)));
constexpr int CNN_THREADS = 512, CNN_WAVES = CNN_THREADS / 64;
constexpr int CNN_NB = 2;                      // tiles of a strip: they share the A operand

__device__ __forceinline__ cnn_f64x4 cnn_mfma(double a, double b, cnn_f64x4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// z [T x c_out] = [xp-view | 1] . P^T: epi(t, o, z) once for every t < T, o < c_out, by the lane that holds it
template <class Epi>
__device__ __forceinline__ void cnn_forward(const double* xp, const double* P, int T, int c_in, int c_out, int K, int wave,
                                            int lane, Epi epi) {
    const int lr = lane & 15, lq = lane >> 4, KS = K + 1;
    const int nrt = (T + 15) / 16, nct = (c_out + 15) / 16, ncs = (nct + CNN_NB - 1) / CNN_NB;
    for (int s = wave; s < nrt * ncs; s += CNN_WAVES) {
        const int rt = s / ncs, ct0 = (s - rt * ncs) * CNN_NB;
        const int t = 16 * rt + lr < T ? 16 * rt + lr : T - 1;             // rows and columns beyond the end read the
        const double* a = xp + (size_t)t * c_in + lq;                      // last one; their results are dropped
        const double* b[CNN_NB];
        cnn_f64x4 acc[CNN_NB];
#pragma unroll
        for (int q = 0; q < CNN_NB; ++q) {
            const int o = 16 * (ct0 + q) + lr < c_out ? 16 * (ct0 + q) + lr : c_out - 1;
            b[q] = P + (size_t)o * KS + lq;
            acc[q] = cnn_f64x4{0.0, 0.0, 0.0, 0.0};
        }
        int kk = 0;
        for (; kk + 4 <= K; kk += 4) {
            const double av = a[kk];
#pragma unroll
            for (int q = 0; q < CNN_NB; ++q)
                if (ct0 + q < nct) acc[q] = cnn_mfma(av, b[q][kk], acc[q]);
        }
        for (; kk < KS; kk += 4) {                                         // the last inputs, the bias column, zeros
            const int k1 = kk + lq;
            const double av = k1 < K ? a[kk] : (k1 == K ? 1.0 : 0.0);
#pragma unroll
            for (int q = 0; q < CNN_NB; ++q)
                if (ct0 + q < nct) acc[q] = cnn_mfma(av, k1 <= K ? b[q][kk] : 0.0, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < CNN_NB; ++q) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 16 * rt + 4 * i + lq, col = 16 * (ct0 + q) + lr;
                if (row < T && col < c_out) epi(row, col, acc[q][i]);
            }
        }
    }
}

struct CnnAdam { double beta1, beta2, step, rs2, eps; bool first; };

// strip s of the layer's weight gradient dP [c_out x (K + 1)] = dz^T . [xp-view | 1], rows t in ascending groups of four,
// and the Adam step of its elements by the lanes that hold them
__device__ __forceinline__ void cnn_weight_grad_strip(int s, const double* dzp, const double* xp, double* P, double* M,
                                                      double* V, int T, int c_in, int c_out, int kernel, int lane,
                                                      const CnnAdam& ad) {
    const int lr = lane & 15, lq = lane >> 4, K = kernel * c_in, KS = K + 1, pad = (kernel - 1) / 2;
    const int nct = (KS + 15) / 16, ncs = (nct + CNN_NB - 1) / CNN_NB;
    const int rt = s / ncs, ct0 = (s - rt * ncs) * CNN_NB;
    const int o = 16 * rt + lr < c_out ? 16 * rt + lr : c_out - 1;
    const double* a = dzp + (size_t)pad * c_out + o;
    int kc[CNN_NB];
    cnn_f64x4 acc[CNN_NB];
#pragma unroll
    for (int q = 0; q < CNN_NB; ++q) {
        kc[q] = 16 * (ct0 + q) + lr < KS ? 16 * (ct0 + q) + lr : K;
        acc[q] = cnn_f64x4{0.0, 0.0, 0.0, 0.0};
    }
    for (int t0 = 0; t0 < T; t0 += 4) {
        const int t = t0 + lq;
        const bool in = t < T;
        const double av = in ? a[(size_t)t * c_out] : 0.0;
#pragma unroll
        for (int q = 0; q < CNN_NB; ++q) {
            if (ct0 + q < nct) {
                const double bv = in ? (kc[q] < K ? xp[(size_t)t * c_in + kc[q]] : 1.0) : 0.0;
                acc[q] = cnn_mfma(av, bv, acc[q]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < CNN_NB; ++q) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = 16 * rt + 4 * i + lq, col = 16 * (ct0 + q) + lr;
            if (row < c_out && col < KS) {
                const size_t at = (size_t)row * KS + col;
                double prm = P[at], m = ad.first ? 0.0 : M[at], v = ad.first ? 0.0 : V[at];
                fnn_adam(prm, m, v, acc[q][i], ad.beta1, ad.beta2, ad.step, ad.rs2, ad.eps);
                P[at] = prm;
                M[at] = m;
                V[at] = v;
            }
        }
    }
}

// the strips of a layer's weight gradient: wave w of the workgroup takes those whose place in the list is w mod 8
__host__ __device__ inline int cnn_weight_grad_strips(int c_in, int c_out, int kernel) {
    const int nct = (kernel * c_in + 1 + 15) / 16;
    return ((c_out + 15) / 16) * ((nct + CNN_NB - 1) / CNN_NB);
}

}  // namespace esn
