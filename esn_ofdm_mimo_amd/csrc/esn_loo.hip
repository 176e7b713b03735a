// Leave-one-out choice of the ridge parameter: one workgroup per pilot, one Gram pass, then for each
// of the L candidates a Cholesky factorisation, the inverse of the factor, the LOO residuals and their score, the
// argmin, and W_out for the chosen lambda only.
//
//   wide (rows <= cols):  K = E E^T + lambda I,  A = K^-1 D_s,            loo[i][o] = A[i][o] / (K^-1)[i][i]
//   tall (rows >  cols):  G = E^T E + lambda I,  W^T = G^-1 E^T D_s,      loo[i][o] = (D_s - E W^T)[i][o] / (1 - h_i),
//                         h_i = e_i^T G^-1 e_i = |L^-1 e_i|^2
//
// The un-factored Gram matrix (lower triangle, packed by rows) and the right-hand side stay in the caller's workspace
// between candidates; LDS holds the packed factor, which the in-place inversion turns into X = L^-1.  With X both
// K^-1 D_s = X^T (X D_s) and diag(K^-1)[i] = sum_k X[k][i]^2 are plain products.  Every sum runs in an order fixed by
// the shape alone, so a group's score, choice and W_out do not depend on the batch it is solved in.
//
// Self-contained on purpose: the Gram staging and the MFMA operand layout repeat what readout_chol_kernel
// (esn_solve_chol.hip) does, but sharing them through a header would change how the eight instances of that kernel
// compile.  Only the host-side argument struct (esn_launch.h: ReadoutArgs) is common.
#include <stdlib.h>
#include "esn_common.h"
#include "esn_launch.h"

namespace esn {

constexpr int LO_NP = 128;                  // largest Gram dimension
constexpr int LO_NT = 512;                  // threads: 8 waves
constexpr int LO_NW = LO_NT / 64;
constexpr int LO_RHS = 8;                   // n_out <= 8
constexpr int LO_KC = 32;                   // k-chunk of the Gram pass
constexpr int LO_LD = LO_NP + 1;            // staging row stride (doubles): odd, so a transposing store hits 32 banks
constexpr int LO_TRI = LO_NP * (LO_NP + 1) / 2;             // packed lower triangle, 8256 doubles
constexpr int LO_TILES = 36;                // lower 16x16 tiles of a 128 x 128 Gram matrix
// LDS (doubles): packed factor | z / solution [LO_NP][LO_RHS] | column vector [LO_NP] | reduction scratch [2 LO_NW]
// | 1 / L[j][j] [LO_NP]
constexpr int LO_OFF_Z = LO_TRI;
constexpr int LO_OFF_V = LO_OFF_Z + LO_NP * LO_RHS;
constexpr int LO_OFF_R = LO_OFF_V + LO_NP;
constexpr int LO_OFF_D = LO_OFF_R + 2 * LO_NW;
constexpr size_t LO_LDS = sizeof(double) * (size_t)(LO_OFF_D + LO_NP);          // 76 416 B: two workgroups per CU
static_assert(LO_KC * LO_LD <= LO_TRI, "the Gram staging aliases the factor");
static_assert(LO_LDS <= 80 * 1024, "two workgroups per CU");

typedef double lo_f64x4 __attribute__((ext_vector_type(4)));

struct LooParams {
    const double* E; const float* E32; const double* D;
    int T, transient, cols, n_out;
    const double* t_scale; const double* t_shift;
    const double* ridge; int n_ridge;
    double* W_out; double* score; int* choice; int* status;
    double* work; size_t work_stride;       // doubles per group: Gram [LO_TRI] | rhs [LO_NP][LO_RHS] | best [LO_NP][LO_RHS]
};

__device__ __forceinline__ int lo_idx(int r, int c) { return r * (r + 1) / 2 + c; }   // r >= c
__device__ __forceinline__ const float* lo_src(const LooParams& p, float*) { return p.E32; }
__device__ __forceinline__ const double* lo_src(const LooParams& p, double*) { return p.E; }

// sum over the workgroup in a fixed order (xor tree inside a wave, then the LO_NW wave sums in ascending order);
// every thread gets the sum.  red: LO_NW doubles nobody else uses until the next call.
__device__ __forceinline__ double lo_block_sum(double v, double* red, int tid) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < LO_NW; ++w) s += red[w];
    return s;
}

template <typename TE, bool wide>
__global__ __launch_bounds__(LO_NT) void ridge_loo_kernel(LooParams sp) {
    extern __shared__ __attribute__((aligned(16))) char loo_smem[];
    double* Ls = reinterpret_cast<double*>(loo_smem);               // packed factor, then X = L^-1
    double* As = Ls;                                                // [LO_KC][LO_LD] staging of the Gram pass
    double* Zs = Ls + LO_OFF_Z;                                     // [LO_NP][LO_RHS]
    double* Vs = Ls + LO_OFF_V;                                     // [LO_NP]
    double* Rs = Ls + LO_OFF_R;                                     // [2 LO_NW]
    double* Ds = Ls + LO_OFF_D;                                     // [LO_NP] 1 / L[j][j]
    const int g = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int rows = sp.T - sp.transient, cols = sp.cols, nrhs = sp.n_out, L = sp.n_ridge;
    const int n = wide ? rows : cols;       // Gram dimension (<= LO_NP)
    const int m = wide ? cols : rows;       // contraction length
    const TE* A = lo_src(sp, (TE*)nullptr) + ((size_t)g * sp.T + sp.transient) * cols;     // [rows][cols]
    const double* Dg = sp.D + ((size_t)g * sp.T + sp.transient) * nrhs;
    double* Gw = sp.work + (size_t)g * sp.work_stride;              // packed lower Gram matrix, un-factored
    double* Bw = Gw + LO_TRI;                                       // rhs [n][LO_RHS]: D_s (wide) or E^T D_s (tall)
    double* Best = Bw + LO_NP * LO_RHS;                             // solution of the best candidate so far
    double sc[LO_RHS], sh[LO_RHS];
#pragma unroll
    for (int o = 0; o < LO_RHS; ++o) {
        sc[o] = (o < nrhs && sp.t_scale) ? sp.t_scale[(size_t)g * nrhs + o] : 1.0;
        sh[o] = (o < nrhs && sp.t_shift) ? sp.t_shift[(size_t)g * nrhs + o] : 0.0;
    }

    // ---- phase 1: the Gram matrix, once, on the float64 matrix pipe --------------------------------------------
    // v_mfma_f64_16x16x4_f64: A[l%16][l/16], B[l/16][l%16], C reg i: row 4i + l/16, col l%16.  Lower tile t goes to
    // wave t % 8; a chunk of LO_KC contraction steps is staged in LDS as doubles, k-major.
    {
        int g_ti[5], g_tj[5];
        const int ntile = (n + 15) / 16, ntl = ntile * (ntile + 1) / 2;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int t = wv + LO_NW * q < LO_TILES ? wv + LO_NW * q : 0;
            int ti = 0;
            while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
            g_ti[q] = ti;
            g_tj[q] = t - ti * (ti + 1) / 2;
        }
        lo_f64x4 acc[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[q] = lo_f64x4{0.0, 0.0, 0.0, 0.0};
        double atb[2] = {0.0, 0.0};         // tall: (E^T D_s)[i][o], thread (o, i) = (e / 128, e % 128), e = tid + 512 p
        for (int k0 = 0; k0 < m; k0 += LO_KC) {
            __syncthreads();                                        // the previous chunk is read out
            for (int e = tid; e < LO_KC * LO_NP; e += LO_NT) {
                int i, kk;
                if (wide) { i = e / LO_KC; kk = e % LO_KC; }        // 32 consecutive k of one E row
                else      { kk = e / LO_NP; i = e % LO_NP; }        // 128 consecutive columns of one E row
                const int k = k0 + kk;
                double v = 0.0;
                if (i < n && k < m) v = (double)A[wide ? (size_t)i * cols + k : (size_t)k * cols + i];
                As[kk * LO_LD + i] = v;
            }
            __syncthreads();
            const int kmax = (m - k0 < LO_KC) ? m - k0 : LO_KC;     // (rows past m of the chunk are zero)
            const double* slab0 = As + lq * LO_LD + lr;
            for (int k4 = 0; k4 < kmax; k4 += 4) {
                const double* slab = slab0 + k4 * LO_LD;
#pragma unroll
                for (int q = 0; q < 5; ++q)
                    if (wv + LO_NW * q < ntl)
                        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(slab[g_ti[q] * 16], slab[g_tj[q] * 16], acc[q], 0, 0, 0);
            }
            if constexpr (!wide) {
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const int e = tid + LO_NT * p, o = e / LO_NP, i = e % LO_NP;
                    if (o < nrhs && i < n) {
                        for (int kk = 0; kk < kmax; ++kk)
                            atb[p] = fma(As[kk * LO_LD + i], Dg[(size_t)(k0 + kk) * nrhs + o] * sc[o] + sh[o], atb[p]);
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 5; ++q)
            if (wv + LO_NW * q < ntl) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = 16 * g_ti[q] + 4 * i + lq, c = 16 * g_tj[q] + lr;
                    if (r < n && c <= r) Gw[lo_idx(r, c)] = acc[q][i];
                }
            }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int e = tid + LO_NT * p;
            if (wide) {
                const int i = e / LO_RHS, o = e % LO_RHS;
                Bw[e] = (i < n && o < nrhs) ? Dg[(size_t)i * nrhs + o] * sc[o] + sh[o] : 0.0;
            } else {
                const int o = e / LO_NP, i = e % LO_NP;
                Bw[i * LO_RHS + o] = (o < nrhs && i < n) ? atb[p] : 0.0;
            }
        }
        __threadfence_block();
        __syncthreads();
    }

    // ---- phase 2: the candidates -------------------------------------------------------------------------------
    const int ntri = n * (n + 1) / 2;
    double best = __builtin_inf();
    int best_l = -1;
    for (int l = 0; l < L; ++l) {
        const double lam = sp.ridge[(size_t)g * L + l];
        if (!(lam >= 0.0 && lam <= 1.7976931348623157e308)) {      // negative or non-finite: never a candidate
            if (tid == 0) { sp.status[(size_t)g * L + l] = 2; sp.score[(size_t)g * L + l] = __builtin_inf(); }
            continue;
        }
        __syncthreads();
        for (int e = tid; e < ntri; e += LO_NT) Ls[e] = Gw[e];
        __syncthreads();
        // lambda on the diagonal before the pivot threshold is taken, as the ridge Cholesky solve does
        for (int i = tid; i < n; i += LO_NT) Ls[lo_idx(i, i)] += lam;
        __syncthreads();
        double dmax = 0.0;
        for (int i = lane; i < n; i += 64) dmax = fmax(dmax, Ls[lo_idx(i, i)]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, off));
        const double piv_tol = dmax * 1e-14;

        // (a) right-looking Cholesky by columns; every thread reads the same pivot, so the verdict is uniform.  The
        // diagonal entry itself is never overwritten (no barrier between its read and the column scaling): what the
        // inversion needs of it, 1 / L[j][j], goes to Ds.  Two barriers per column.
        bool failed = false;
        for (int j = 0; j < n; ++j) {
            const double v = Ls[lo_idx(j, j)];
            if (!(v > piv_tol)) { failed = true; break; }
            const double d = sqrt(v), inv = 1.0 / d;
            if (tid == 0) Ds[j] = inv;
            for (int i = j + 1 + tid; i < n; i += LO_NT) {
                const double x = Ls[lo_idx(i, j)] * inv;
                Ls[lo_idx(i, j)] = x;
                Vs[i] = x;
            }
            __syncthreads();
            // A22[r][c] -= L[r][j] L[c][j], j < c <= r: 16 rows x 32 columns of threads
            for (int r = j + 1 + (tid >> 5); r < n; r += LO_NT / 32) {
                const double lrj = Vs[r];
                double* row = Ls + lo_idx(r, 0);
                for (int c = j + 1 + (tid & 31); c <= r; c += 32) row[c] = fma(-lrj, Vs[c], row[c]);
            }
            __syncthreads();
        }
        if (failed) {
            if (tid == 0) { sp.status[(size_t)g * L + l] = 1; sp.score[(size_t)g * L + l] = __builtin_inf(); }
            continue;
        }

        // (b) X = L^-1 in place, last column first: X[j][j] = 1 / L[j][j], X[i][j] = -X[j][j] sum_{k=j+1..i} X[i][k] L[k][j].
        // Four threads per row split k by k % 4 and meet in a fixed xor tree.
        {
            const int i = tid >> 2, s = tid & 3;
            for (int j = n - 1; j >= 0; --j) {
                for (int k = j + 1 + tid; k < n; k += LO_NT) Vs[k] = Ls[lo_idx(k, j)];
                __syncthreads();
                const double xjj = Ds[j];
                double part = 0.0;
                if (i > j && i < n) {
                    const double* row = Ls + lo_idx(i, 0);
                    for (int k = j + 1 + s; k <= i; k += 4) part = fma(row[k], Vs[k], part);
                }
                part += __shfl_xor(part, 1);
                part += __shfl_xor(part, 2);
                if (s == 0 && i >= j && i < n) Ls[lo_idx(i, j)] = (i == j) ? xjj : -xjj * part;
                __syncthreads();
            }
        }

        // (c) z = X B, then sol = X^T z and dg[i] = sum_k X[k][i]^2 = diag((Gram + lambda I)^-1); thread (i, o)
        double z[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int e = tid + LO_NT * p, i = e / LO_RHS, o = e % LO_RHS;
            double a = 0.0;
            if (i < n && o < nrhs) {
                const double* row = Ls + lo_idx(i, 0);
                for (int k = 0; k <= i; ++k) a = fma(row[k], Bw[k * LO_RHS + o], a);
            }
            z[p] = a;
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) Zs[tid + LO_NT * p] = z[p];
        __syncthreads();
        double sol[2], dg[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int e = tid + LO_NT * p, i = e / LO_RHS, o = e % LO_RHS;
            double a = 0.0, q = 0.0;
            if (i < n) {
                for (int k = i; k < n; ++k) {
                    const double x = Ls[lo_idx(k, i)];
                    a = fma(x, Zs[k * LO_RHS + o], a);
                    q = fma(x, x, q);
                }
            }
            sol[p] = a;
            dg[p] = q;
        }

        // (d) the score
        double part = 0.0;
        if constexpr (wide) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int e = tid + LO_NT * p, i = e / LO_RHS, o = e % LO_RHS;
                if (i < n && o < nrhs) {
                    const double q = sol[p] / dg[p];
                    part = fma(q, q, part);
                }
            }
        } else {
            // W^T into LDS; then four threads per fit row: y = X e_i by rows j % 4 (h_i = |y|^2) and the residual by
            // k % 4, both met in a fixed xor tree.  E comes from L2 here: it was streamed from HBM by the Gram pass.
            __syncthreads();
#pragma unroll
            for (int p = 0; p < 2; ++p) Zs[tid + LO_NT * p] = sol[p];
            __syncthreads();
            for (int base = 0; base < 4 * rows; base += LO_NT) {
                const int idx = base + tid, i = idx >> 2, s = idx & 3;
                const bool live = i < rows;
                double h = 0.0, r[LO_RHS];
#pragma unroll
                for (int o = 0; o < LO_RHS; ++o) r[o] = 0.0;
                if (live) {
                    const TE* e_i = A + (size_t)i * cols;
                    for (int j = s; j < n; j += 4) {
                        const double* row = Ls + lo_idx(j, 0);
                        double y = 0.0;
                        for (int k = 0; k <= j; ++k) y = fma(row[k], (double)e_i[k], y);
                        h = fma(y, y, h);
                    }
                    for (int k = s; k < n; k += 4) {
                        const double ek = (double)e_i[k];
#pragma unroll
                        for (int o = 0; o < LO_RHS; ++o) r[o] = fma(ek, Zs[k * LO_RHS + o], r[o]);
                    }
                }
                h += __shfl_xor(h, 1);
                h += __shfl_xor(h, 2);
#pragma unroll
                for (int o = 0; o < LO_RHS; ++o) {
                    r[o] += __shfl_xor(r[o], 1);
                    r[o] += __shfl_xor(r[o], 2);
                }
                if (live && s == 0) {
                    const double den = 1.0 - h;
#pragma unroll
                    for (int o = 0; o < LO_RHS; ++o)
                        if (o < nrhs) {
                            const double q = (Dg[(size_t)i * nrhs + o] * sc[o] + sh[o] - r[o]) / den;
                            part = fma(q, q, part);
                        }
                }
            }
        }
        const double score = lo_block_sum(part, Rs + (l & 1) * LO_NW, tid);
        if (tid == 0) { sp.status[(size_t)g * L + l] = 0; sp.score[(size_t)g * L + l] = score; }
        if (score < best) {                 // strict: the lowest index wins a tie; inf and NaN never win
            best = score;
            best_l = l;
#pragma unroll
            for (int p = 0; p < 2; ++p) Best[tid + LO_NT * p] = sol[p];
        }
    }

    // ---- phase 3: W_out for the chosen lambda ------------------------------------------------------------------
    if (tid == 0) sp.choice[g] = best_l;
    double* wo = sp.W_out + (size_t)g * nrhs * cols;
    if (best_l < 0) {
        for (int e = tid; e < nrhs * cols; e += LO_NT) wo[e] = 0.0;
        return;
    }
    __threadfence_block();
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p) Zs[tid + LO_NT * p] = Best[tid + LO_NT * p];
    __syncthreads();
    if constexpr (wide) {
        // W_out[o][c] = sum_i E[i][c] alpha[i][o], i ascending; a thread per column, coalesced across the workgroup
        for (int c = tid; c < cols; c += LO_NT) {
            double w[LO_RHS];
#pragma unroll
            for (int o = 0; o < LO_RHS; ++o) w[o] = 0.0;
            for (int i = 0; i < n; ++i) {
                const double a = (double)A[(size_t)i * cols + c];
#pragma unroll
                for (int o = 0; o < LO_RHS; ++o) w[o] = fma(a, Zs[i * LO_RHS + o], w[o]);
            }
#pragma unroll
            for (int o = 0; o < LO_RHS; ++o)
                if (o < nrhs) wo[(size_t)o * cols + c] = w[o];
        }
    } else {
        for (int e = tid; e < nrhs * cols; e += LO_NT) {
            const int o = e / cols, c = e % cols;
            wo[e] = Zs[c * LO_RHS + o];
        }
    }
}

size_t ridge_loo_work_doubles() { return (size_t)LO_TRI + 2 * LO_NP * LO_RHS; }

int launch_ridge_loo(const ReadoutArgs& a) {
    const int rows = a.T - a.transient, cols = a.cols;
    const int n = rows <= cols ? rows : cols;
    if (n > LO_NP || a.n_out > LO_RHS) return -1;
    const LooParams sp = {a.E, a.E32, a.D, a.T, a.transient, cols, a.n_out, a.t_scale, a.t_shift, a.ridge, a.n_ridge,
                          a.W_out, a.score, a.choice, a.status,
                          reinterpret_cast<double*>(a.workspace), ridge_loo_work_doubles()};
    const bool wide = rows <= cols;
    void (*fn)(LooParams) = a.E32 ? (wide ? ridge_loo_kernel<float, true> : ridge_loo_kernel<float, false>)
                                  : (wide ? ridge_loo_kernel<double, true> : ridge_loo_kernel<double, false>);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)LO_LDS);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fn, dim3(a.n_groups), dim3(LO_NT), LO_LDS, a.stream, sp);
    return (int)hipGetLastError();
}

}  // namespace esn
