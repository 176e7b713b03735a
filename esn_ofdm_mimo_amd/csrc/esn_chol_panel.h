// The blocked Cholesky over a factor in the caller's workspace, for the two kernels that solve normal equations too
// large for LDS: readout_chol_big_kernel (esn_solve_chol_big.hip) and gram_solve_kernel (esn_gram.hip).  One workgroup
// of CP_NT threads per system; the factor L is column-major [np][np] (ld = np, lower part) in global memory, L2 /
// Infinity Cache resident.
//   chol_diag_max       the block maximum of the diagonal, from which the callers take the pivot tolerance
//   chol_panel_factor   one 16-column panel of the left-looking factorisation: panel tile (rt, j) = tile0(rt, j) -
//                       L(rt, :16j) L(j, :16j)^T with both operands read straight from the workspace in MFMA layout
//                       (column-major storage makes a lane group's 16 rows one 128-byte segment), the 16x16 diagonal
//                       factorisation / inversion in registers on wave 0 (ch_diag_regs, as in the LDS kernel), the
//                       panel solve by MFMA from that inverse; the finished panel goes back to the workspace
// Pivot rule (v <= piv_tol: direction dropped, *bad set) and arithmetic order per tile are those of the LDS kernel, so
// all three agree to round-off where more than one applies.  The kernels declare the LDS and hand it in.  The
// substitutions that follow are NOT here: the same source, once a function, compiled to a slower substitution in
// readout_chol_big_kernel (profiles/chol_panel_time.txt), so each kernel keeps its copy -- the two differ in the rows
// per lane (8 / 9) and in how a wave takes its right-hand sides (n_out <= 8: one; <= 16: a loop).
#pragma once
#include "esn_solve.h"

namespace esn {

constexpr int CP_NT = 512;        // threads: 8 waves, two per SIMD
constexpr int CP_NW = CP_NT / 64;
constexpr int CP_PLD = 17;        // LDS row stride of the panel (doubles)

typedef double cp_f64x4 __attribute__((ext_vector_type(4)));

struct CholPanelLds {
    double* P;                    // [np][CP_PLD] panel
    double* invd;                 // [np] 1 / L[i][i] (0 for a dropped direction), for the substitutions
    double (*linv)[17];           // [16][17] inverse of the diagonal block
    int* bad;                     // set when a pivot is rejected
};

// max over i < n of diag(i) and 0; one barrier inside, every thread gets the result
template <typename Diag>
__device__ __forceinline__ double chol_diag_max(Diag diag, int n, double* red) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double dmax = 0.0;
    for (int i = tid; i < n; i += CP_NT) dmax = fmax(dmax, diag(i));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dmax = fmax(dmax, __shfl_down(dmax, off));
    if (lane == 0) red[wv] = dmax;
    __syncthreads();
    dmax = 0.0;
    for (int w = 0; w < CP_NW; ++w) dmax = fmax(dmax, red[w]);
    return dmax;
}

// Panel j (columns j0 = 16 j ..), called for j = 0 .. np / 16 - 1 in order by the whole block.  tile0(rt, j0, i): element
// (16 rt + 4 i + lane / 16, j0 + lane % 16) of the matrix to factorise -- register i of this lane's C operand.  wvu: the
// wave index as a scalar.  Ends behind a barrier, the panel visible to the whole block.
template <typename Tile0>
__device__ __forceinline__ void chol_panel_factor(double* Lw, int ld, int n, int np, double piv_tol,
                                                  const CholPanelLds& s, int wvu, int j, Tile0 tile0) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int ntile = np / 16, j0 = 16 * j;
    double* P = s.P;
    // (1) panel tiles: tile0(rt, j) - L(rt, :j0) L(j, :j0)^T
    for (int rt = j + wvu; rt < ntile; rt += CP_NW) {
        cp_f64x4 c;
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = tile0(rt, j0, i);
        const double* la = Lw + (size_t)lq * ld + rt * 16 + lr;       // L[rt*16 + lr][k + lq]
        const double* lb = Lw + (size_t)lq * ld + j0 + lr;            // L[j0 + lr][k + lq]
#pragma unroll 4
        for (int k = 0; k < j0; k += 4)
            c = __builtin_amdgcn_mfma_f64_16x16x4f64(-la[(size_t)k * ld], lb[(size_t)k * ld], c, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) P[(rt * 16 + 4 * i + lq) * CP_PLD + lr] = c[i];
    }
    __syncthreads();
    // (2) diagonal block: factorise and invert in registers (wave 0), as in the LDS kernel
    if (wv == 0) {
        const int r = lane & 15;
        double a[16], x[16], my_invd;
#pragma unroll
        for (int c = 0; c < 16; ++c) a[c] = P[(j0 + r) * CP_PLD + c];
        const unsigned rejected = ch_diag_regs<false, true>(a, x, my_invd, j0, n, piv_tol, r);
        if (lane < 16) {
#pragma unroll
            for (int c = 0; c < 16; ++c) P[(j0 + r) * CP_PLD + c] = a[c];
            s.invd[j0 + r] = my_invd;
        }
        if (rejected && lane == 0) *s.bad = 1;
        if (lane < 16) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s.linv[i][r] = x[i];
        }
    }
    __syncthreads();
    // (3) panel solve: L(rt, j) = P(rt) L11^-T
    for (int rt = j + 1 + wvu; rt < ntile; rt += CP_NW) {
        cp_f64x4 c = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k0 = 0; k0 < 16; k0 += 4)
            c = __builtin_amdgcn_mfma_f64_16x16x4f64(P[(rt * 16 + lr) * CP_PLD + k0 + lq], s.linv[lr][k0 + lq], c, 0, 0, 0);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 4; ++i) P[(rt * 16 + 4 * i + lq) * CP_PLD + lr] = c[i];
    }
    __syncthreads();
    // (4) the finished panel (rows j0 .. np-1, 16 columns) back to the workspace, column-major
    for (int e = tid; e < (np - j0) * 16; e += CP_NT) {
        const int c = e / (np - j0), rr = j0 + e % (np - j0);
        Lw[(size_t)(j0 + c) * ld + rr] = P[rr * CP_PLD + c];
    }
    __threadfence_block();
    __syncthreads();
}

}  // namespace esn
