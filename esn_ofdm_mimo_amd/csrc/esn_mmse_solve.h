// The per-subcarrier linear solve of the baseline equaliser, written once for the kernels that need X on the chip:
//   esn_baseline.hip   mmse_detect_kernel (slices X and counts), channel_estimate_kernel (cdiv)
//   esn_equalize.hip   mmse_equalize_rows_kernel (turns X back into time-domain rows)
//   esn_soft.hip       mmse_sinr_kernel (mmse_sinr_point: the solve's bias and SINR per stream, no Y)
//   esn_dcc.hip        mmse_dcc_kernel (X0, and once per cancellation pass on H D in place of Y)
// Those with a Y go through mmse_spectrum and mmse_solve_point, and the library is built with -ffp-contract=off, so they compile
// the same operations on the same operands: their X_hat is bit-identical.
#pragma once
#include "esn_common.h"
#include "esn_ofdm_math.h"

namespace esn {

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cdiv(double2 a, double2 b) {
    const double d = b.x * b.x + b.y * b.y;
    return make_double2((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}

constexpr int MMSE_NT = 4;     // transmit antennas handled in registers

// Y[rx][k] = (1/N) sum_i y[i][rx] e^{-2 pi i ik/N}: y complex [N][n_r] (the frame behind its prefix), Y [n_r][N] and
// tw [N/2] in LDS.  The whole workgroup calls it; it ends behind a barrier.
__device__ __forceinline__ void mmse_spectrum(double2* Y, double2* tw, const double* y, int N, int log2n, int n_r) {
    const int tid = threadIdx.x, nth = blockDim.x;
    ofdm_twiddles(tw, N >> 1, N, -1.0);
    for (int e = tid; e < N * n_r; e += nth) {
        const int i = e / n_r, rx = e % n_r;
        const int rv = (int)(__brev((unsigned)i) >> (32 - log2n));
        Y[(size_t)rx * N + rv] = make_double2(y[(size_t)e * 2] / N, y[(size_t)e * 2 + 1] / N);
    }
    __syncthreads();
    ofdm_fft_lds(Y, n_r, N, tw, N, log2n);
}

// x = (H_k^H H_k + lam I)^-1 H_k^H Y_k: hk complex [n_r][n_t] (global), Y [n_r][N] (LDS), n_t <= MMSE_NT; x[tx] for
// tx >= n_t is zero
__device__ __forceinline__ void mmse_solve_point(const double* hk, const double2* Y, int N, int k, int n_t, int n_r,
                                                 double lam, double2 (&x)[MMSE_NT]) {
    // G = H^H H + lam I (Hermitian, n_t x n_t), r = H^H Y
    double2 G[MMSE_NT][MMSE_NT], rhs[MMSE_NT];
#pragma unroll
    for (int a = 0; a < MMSE_NT; ++a) {
        rhs[a] = make_double2(0.0, 0.0);
#pragma unroll
        for (int b = 0; b < MMSE_NT; ++b) G[a][b] = make_double2(a == b ? lam : 0.0, 0.0);
    }
    for (int rx = 0; rx < n_r; ++rx) {
        double2 h[MMSE_NT];
#pragma unroll
        for (int a = 0; a < MMSE_NT; ++a)
            h[a] = (a < n_t) ? make_double2(hk[((size_t)rx * n_t + a) * 2], hk[((size_t)rx * n_t + a) * 2 + 1])
                             : make_double2(0.0, 0.0);
        const double2 yv = Y[(size_t)rx * N + k];
#pragma unroll
        for (int a = 0; a < MMSE_NT; ++a) {
            const double2 hc = make_double2(h[a].x, -h[a].y);
            const double2 t = cmul(hc, yv);
            rhs[a].x += t.x; rhs[a].y += t.y;
#pragma unroll
            for (int b = 0; b < MMSE_NT; ++b) {
                const double2 u = cmul(hc, h[b]);
                G[a][b].x += u.x; G[a][b].y += u.y;
            }
        }
    }
#pragma unroll
    for (int a = 0; a < MMSE_NT; ++a)
        if (a >= n_t) G[a][a] = make_double2(1.0, 0.0);       // padding antennas: identity rows
    // Gaussian elimination (G is Hermitian positive definite: no pivoting needed)
#pragma unroll
    for (int c = 0; c < MMSE_NT; ++c) {
        const double2 piv = G[c][c];
#pragma unroll
        for (int rr = c + 1; rr < MMSE_NT; ++rr) {
            const double2 f = cdiv(G[rr][c], piv);
#pragma unroll
            for (int cc = c; cc < MMSE_NT; ++cc) {
                const double2 t = cmul(f, G[c][cc]);
                G[rr][cc].x -= t.x; G[rr][cc].y -= t.y;
            }
            const double2 t = cmul(f, rhs[c]);
            rhs[rr].x -= t.x; rhs[rr].y -= t.y;
        }
    }
#pragma unroll
    for (int c = MMSE_NT - 1; c >= 0; --c) {
        double2 acc = rhs[c];
#pragma unroll
        for (int cc = c + 1; cc < MMSE_NT; ++cc) {
            const double2 t = cmul(G[c][cc], x[cc]);
            acc.x -= t.x; acc.y -= t.y;
        }
        x[c] = cdiv(acc, G[c][c]);
    }
}

// t[tx] = lam [(H_k^H H_k + lam I)^-1]_{tx tx}, the error share of stream tx behind the solve above (bias 1 - t, SINR
// (1 - t) / t): the same Gram matrix by the same operations, eliminated against the identity, one back substitution per
// column.  t[tx] for tx >= n_t is lam (their rows are the identity); the caller clamps
__device__ __forceinline__ void mmse_sinr_point(const double* hk, int n_t, int n_r, double lam, double (&t)[MMSE_NT]) {
    double2 G[MMSE_NT][MMSE_NT], B[MMSE_NT][MMSE_NT];
#pragma unroll
    for (int a = 0; a < MMSE_NT; ++a)
#pragma unroll
        for (int b = 0; b < MMSE_NT; ++b) {
            G[a][b] = make_double2(a == b ? lam : 0.0, 0.0);
            B[a][b] = make_double2(a == b ? 1.0 : 0.0, 0.0);
        }
    for (int rx = 0; rx < n_r; ++rx) {
        double2 h[MMSE_NT];
#pragma unroll
        for (int a = 0; a < MMSE_NT; ++a)
            h[a] = (a < n_t) ? make_double2(hk[((size_t)rx * n_t + a) * 2], hk[((size_t)rx * n_t + a) * 2 + 1])
                             : make_double2(0.0, 0.0);
#pragma unroll
        for (int a = 0; a < MMSE_NT; ++a) {
            const double2 hc = make_double2(h[a].x, -h[a].y);
#pragma unroll
            for (int b = 0; b < MMSE_NT; ++b) {
                const double2 u = cmul(hc, h[b]);
                G[a][b].x += u.x; G[a][b].y += u.y;
            }
        }
    }
#pragma unroll
    for (int a = 0; a < MMSE_NT; ++a)
        if (a >= n_t) G[a][a] = make_double2(1.0, 0.0);
#pragma unroll
    for (int c = 0; c < MMSE_NT; ++c) {
        const double2 piv = G[c][c];
#pragma unroll
        for (int rr = c + 1; rr < MMSE_NT; ++rr) {
            const double2 f = cdiv(G[rr][c], piv);
#pragma unroll
            for (int cc = c; cc < MMSE_NT; ++cc) {
                const double2 u = cmul(f, G[c][cc]);
                G[rr][cc].x -= u.x; G[rr][cc].y -= u.y;
            }
#pragma unroll
            for (int j = 0; j <= c; ++j) {                    // B stays lower triangular
                const double2 u = cmul(f, B[c][j]);
                B[rr][j].x -= u.x; B[rr][j].y -= u.y;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MMSE_NT; ++j) {                       // column j of the inverse, down to its row j
        double2 z[MMSE_NT];
#pragma unroll
        for (int c = MMSE_NT - 1; c >= j; --c) {
            double2 acc = B[c][j];
#pragma unroll
            for (int cc = c + 1; cc < MMSE_NT; ++cc) {
                const double2 u = cmul(G[c][cc], z[cc]);
                acc.x -= u.x; acc.y -= u.y;
            }
            z[c] = cdiv(acc, G[c][c]);
        }
        t[j] = lam * z[j].x;
    }
}

}  // namespace esn
