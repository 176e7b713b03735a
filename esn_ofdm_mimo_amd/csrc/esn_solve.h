// What the three read-out solve kernels share: their parameter block and how the host fills it, the rejection of a
// bad lambda, the wave sum, and the register form of the 16x16 diagonal-tile factorisation both Cholesky kernels
// call.  esn_solve_qr.hip (Householder QR), esn_solve_chol.hip (Gram matrix and factor in LDS, Gram dimension <= 128)
// and esn_solve_chol_big.hip (in the caller's workspace, <= 512) hold one kernel and its launcher each.
//
// Ridge (an extension, the reference has none): W_out = argmin |E W^T - D_s|^2 + lambda |W|^2, lambda >= 0 absolute.
// The <true> instances of the three kernels run one workgroup per (group, lambda): workgroup `slot` reads E of group
// slot / n_ridge and lambda = ridge[slot], and writes W_out[slot], status[slot].  The QR kernel solves the augmented
// problem (tall: [A ; sqrt(lambda) I] w = [B ; 0]; wide: minimum norm of [A  sqrt(lambda) I] [w ; z] = B, first
// `cols` entries kept); the Cholesky kernels add lambda to the live Gram diagonal.  lambda = 0 takes the pinv path
// instruction for instruction; a negative or non-finite lambda gives status 2 and a zero W_out.
#pragma once
#include <stdlib.h>
#include <type_traits>
#include "esn_common.h"
#include "esn_launch.h"

namespace esn {

struct SolveParams {
    const double* E; const double* D;
    const float* E32;       // Cholesky path: extended states as float32 (E unused) -- esn_harvest_batch_f32
    int n_groups, T, transient, cols, n_out;
    const double* t_scale; const double* t_shift;
    double* W_out; int* status;
    double* work; size_t work_stride;   // doubles per group
    int m, n, wide;
    int skip;   // diagnostic only (ESN_CHOL_SKIP env): bit0 Gram, bit1 Cholesky, bit2 solves, bit3 W_out
    int part_ok;   // big kernel: the three-partial-sums W_out pass fits the LDS the launcher allocated
    int vec;       // LDS Cholesky kernel: E rows start 16-byte aligned and hold whole 16-byte runs (vector loads)
    int dma;       // LDS Cholesky kernel, wide float32 E: Gram and W_out passes fed by LDS-DMA rings (knob chol_dma)
    unsigned long long* stamps;   // diagnostic build (-DESN_STAMPS) only: [wave][8] cycle sums of workgroup 0
    const double* ridge; int n_ridge;   // ridge instances only: lambda [n_groups][n_ridge]
};

// The part of the parameter block every launcher fills alike, the rest zero: the launchers add work, work_stride,
// skip, dma, vec and part_ok as their kernel reads them.
inline SolveParams solve_params(const ReadoutArgs& a) {
    SolveParams sp{};
    const int rows = a.T - a.transient;
    sp.E = a.E; sp.E32 = a.E32; sp.D = a.D; sp.n_groups = a.n_groups; sp.T = a.T; sp.transient = a.transient;
    sp.cols = a.cols; sp.n_out = a.n_out; sp.t_scale = a.t_scale; sp.t_shift = a.t_shift;
    sp.W_out = a.W_out; sp.status = a.status;
    sp.wide = rows < a.cols; sp.m = sp.wide ? a.cols : rows; sp.n = sp.wide ? rows : a.cols;
    sp.ridge = a.ridge; sp.n_ridge = a.n_ridge;
    ESN_STAMPS_ONLY(sp.stamps = stamp_buffer();)
    return sp;
}
// workgroups of a launch: one per group, or per (group, lambda) in the ridge instances
inline int solve_grid(const ReadoutArgs& a) { return a.ridge ? a.n_groups * a.n_ridge : a.n_groups; }

// doubles of workspace per workgroup: the QR kernel, its ridge instance (the augmented matrix), the workspace Cholesky
inline size_t solve_work_doubles(int rows, int cols, int n_out) {
    const bool wide = rows < cols;
    const size_t m = wide ? cols : rows, n = wide ? rows : cols;
    // matrix (+ rhs columns when tall) + rhs block + rdiag + beta, rounded to 16 B
    size_t d = (n + (wide ? 0 : n_out)) * m + (size_t)n_out * m + 2 * n;
    return (d + 1) & ~(size_t)1;
}
inline size_t solve_ridge_work_doubles(int rows, int cols, int n_out) {
    const bool wide = rows < cols;
    const size_t m = (size_t)rows + cols, n = wide ? rows : cols;      // the augmented matrix has rows + cols rows
    size_t d = (n + (wide ? 0 : n_out)) * m + (size_t)n_out * m + 2 * n;
    return (d + 1) & ~(size_t)1;
}
inline size_t chol_big_work_doubles(int n) {
    const size_t np = (size_t)round_up(n, 16);
    return np * np;
}

// ridge instances: workgroup `slot` with a negative or non-finite lambda writes status 2 and a zero W_out
__device__ __forceinline__ bool ridge_rejects(const SolveParams& sp, int slot) {
    const double lam = sp.ridge[slot];
    if (lam >= 0.0 && lam <= 1.7976931348623157e308) return false;
    double* wo = sp.W_out + (size_t)slot * sp.n_out * sp.cols;
    for (int i = threadIdx.x; i < sp.n_out * sp.cols; i += blockDim.x) wo[i] = 0.0;
    if (threadIdx.x == 0) sp.status[slot] = 2;
    return true;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return __shfl(v, 0);
}

// element (r, c) of a tile: row-major, the column XORed with the row pair.  MFMA operand reads by row
// (r = lane % 16, c = k + lane / 16) and by column (r = k + lane / 16, c = lane % 16), the 16-lane row
// reads of the diagonal factorisation and the accumulator stores all hit 32 distinct 8-byte banks.
__device__ __forceinline__ int ch_el(int r, int c) { return r * 16 + (c ^ (r & ~1)); }

// copy of lane SRC of this lane's 16-lane row, by DPP: the value stays in the vector pipe (a v_readlane would take
// it through an SGPR pair, and what is decided from it through the scalar unit and a branch).  The wait states of
// a DPP read behind a VALU write of its source or of EXEC open the string, as in ch_dpp_fmac.
template <int SRC>
__device__ __forceinline__ double ch_row_bcast(double x) {
    double v;
    asm("s_nop 4\n\tv_mov_b64_dpp %0, %1 row_newbcast:%c2 row_mask:0xf bank_mask:0xf" : "=v"(v) : "v"(x), "i"(SRC));
    return v;
}

// acc[t] = fma(-(d of lane L0 + t of this lane's 16-lane row), o, acc[t]) for t < N, N = 8, 4, 2 or 1: the
// double-precision DPP form v_fmac_f64_dpp with row_newbcast takes the cross-lane factor as src0, so no value
// travels through SGPRs.  One statement per group: the compiler sees neither the broadcasts (it cannot keep the
// 120 of the factorisation alive for the inversion, which needs the same values) nor the DPP reads, so the wait
// states a DPP read needs after a VALU write of its source (2) or of EXEC (5) open the string.
#define CH_DPP_FMAC(t) "v_fmac_f64_dpp %" #t ", -%[d], %[o] row_newbcast:%c[l" #t "] row_mask:0xf bank_mask:0xf\n\t"
template <int L0, int N>
__device__ __forceinline__ void ch_dpp_fmac(double* acc, double d, double o) {
    static_assert(N == 8 || N == 4 || N == 2 || N == 1, "group sizes");
    static_assert(L0 >= 0 && L0 + N <= 16, "lanes of one row");
    if constexpr (N == 8) {
        asm("s_nop 4\n\t" CH_DPP_FMAC(0) CH_DPP_FMAC(1) CH_DPP_FMAC(2) CH_DPP_FMAC(3)
            CH_DPP_FMAC(4) CH_DPP_FMAC(5) CH_DPP_FMAC(6) CH_DPP_FMAC(7)
            : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]), "+v"(acc[7])
            : [d] "v"(d), [o] "v"(o), [l0] "i"(L0), [l1] "i"(L0 + 1), [l2] "i"(L0 + 2), [l3] "i"(L0 + 3),
              [l4] "i"(L0 + 4), [l5] "i"(L0 + 5), [l6] "i"(L0 + 6), [l7] "i"(L0 + 7));
    } else if constexpr (N == 4) {
        asm("s_nop 4\n\t" CH_DPP_FMAC(0) CH_DPP_FMAC(1) CH_DPP_FMAC(2) CH_DPP_FMAC(3)
            : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3])
            : [d] "v"(d), [o] "v"(o), [l0] "i"(L0), [l1] "i"(L0 + 1), [l2] "i"(L0 + 2), [l3] "i"(L0 + 3));
    } else if constexpr (N == 2) {
        asm("s_nop 4\n\t" CH_DPP_FMAC(0) CH_DPP_FMAC(1)
            : "+v"(acc[0]), "+v"(acc[1]) : [d] "v"(d), [o] "v"(o), [l0] "i"(L0), [l1] "i"(L0 + 1));
    } else {
        asm("s_nop 4\n\t" CH_DPP_FMAC(0) : "+v"(acc[0]) : [d] "v"(d), [o] "v"(o), [l0] "i"(L0));
    }
}
#undef CH_DPP_FMAC
// acc[i] = fma(-(d of lane i), o, acc[i]) for FROM <= i < 16, in groups of 8, 4, 2 and 1
template <int FROM>
__device__ __forceinline__ void ch_dpp_fmac_from(double (&acc)[16], double d, double o) {
    constexpr int cnt = 16 - FROM;
    if constexpr (cnt & 8) ch_dpp_fmac<FROM, 8>(acc + FROM, d, o);
    if constexpr (cnt & 4) ch_dpp_fmac<FROM + (cnt & 8), 4>(acc + FROM + (cnt & 8), d, o);
    if constexpr (cnt & 2) ch_dpp_fmac<FROM + (cnt & 12), 2>(acc + FROM + (cnt & 12), d, o);
    if constexpr (cnt & 1) ch_dpp_fmac<15, 1>(acc + 15, d, o);
}

// One wave, every lane active, lanes 16..63 mirroring lanes 0..15 (r = lane % 16): the 16x16 diagonal tile whose
// row r lane r holds in a[] is factorised in place (a[k] of lane i > k becomes L11[i][k]) and x[] of lane c
// receives column c of L11^-1 by forward substitution.  Nothing travels through SGPRs: the pivot is a DPP row
// broadcast (every lane takes the same accept / reject decision), the 120 updates a[k] -= a[j] L11[k][j] and
// the 120 of the inversion take their cross-lane factor by DPP.  The updates run on every lane: rows r < k of
// column k hold no tile entry and nothing reads them.  FULL_L: the caller stores L11, so a finalised column
// gets its diagonal and 0.0 above it; otherwise only the rows below the diagonal are meaningful afterwards.
// The inversion shares the column loop: once column j and x[j] are final, every x[i], i > j, takes its term;
// each x[i] still sums in ascending k.
// A rejected pivot (v <= tol) drops its direction, as pinv would: unit diagonal and zero column in L11, zero
// row in L11^-1, so the panel column and the solution component vanish too; a padding pivot (past n) is not
// a rejection, and DROP_PAD says whether its row of L11^-1 is zeroed as well.  my_invd (FULL_L only):
// 1 / L11[r][r], 1.0 for a pivot that was not taken.  Returns the mask of rejected live pivots.
template <bool DROP_PAD, bool FULL_L>
__device__ __forceinline__ unsigned ch_diag_regs(double (&a)[16], double (&x)[16], double& my_invd, int j0, int n,
                                                 double piv_tol, int r) {
    my_invd = 1.0;
    unsigned rejected = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = (i == r) ? 1.0 : 0.0;           // x[] holds the running sums until final
    double v = ch_row_bcast<0>(a[0]);                                   // the pivot of the column to come
    auto column = [&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const bool live = j0 + j < n;
        const bool ok = live && v > piv_tol;
        if (live && !ok) rejected |= 1u << j;
        // (selects around the square root and the quotient, not a branch over them: sqrt(1.0) and 1.0 / 1.0 are
        // exact, and the 16 columns stay one block the scheduler can overlap)
        const double d = sqrt(ok ? v : 1.0), inv_1 = 1.0 / d, inv_d = ok ? inv_1 : 0.0;
        if constexpr (FULL_L) {
            if (r == j) my_invd = inv_1;
            a[j] = (r == j) ? d : ((r > j) ? a[j] * inv_d : 0.0);      // column j of L11
        } else {
            a[j] *= inv_d;                                              // rows > j of column j of L11
        }
        // a[k] = fma(-a[j], L11[k][j], a[k]), k > j: the next column first, its pivot is what the chain waits for
        if constexpr (j < 15) {
            ch_dpp_fmac<j + 1, 1>(a + j + 1, a[j], a[j]);
            v = ch_row_bcast<j + 1>(a[j + 1]);
        }
        if constexpr (j < 14) ch_dpp_fmac_from<j + 2>(a, a[j], a[j]);
        const bool zero = DROP_PAD ? !ok : live && !ok;
        x[j] = (j >= r && !zero) ? x[j] * inv_1 : 0.0;                  // row j of L11^-1
        if constexpr (j < 15) ch_dpp_fmac_from<j + 1>(x, a[j], x[j]);   // x[i] = fma(-L11[i][j], x[j], x[i]), i > j
    };
    column(std::integral_constant<int, 0>()); column(std::integral_constant<int, 1>());
    column(std::integral_constant<int, 2>()); column(std::integral_constant<int, 3>());
    column(std::integral_constant<int, 4>()); column(std::integral_constant<int, 5>());
    column(std::integral_constant<int, 6>()); column(std::integral_constant<int, 7>());
    column(std::integral_constant<int, 8>()); column(std::integral_constant<int, 9>());
    column(std::integral_constant<int, 10>()); column(std::integral_constant<int, 11>());
    column(std::integral_constant<int, 12>()); column(std::integral_constant<int, 13>());
    column(std::integral_constant<int, 14>()); column(std::integral_constant<int, 15>());
    return rejected;
}

// One wave: factorise the 16x16 diagonal tile at D in registers and overwrite it with L11^-1 (ch_diag_regs).
// Returns 1 if a live pivot was rejected.
__device__ __forceinline__ int ch_factor_diag(double* D, int j0, int n, double piv_tol, int lane) {
    int r = lane & 15;                              // lanes 16..63 mirror lanes 0..15 (no divergence)
    // opaque per call: what depends on r alone (the 16 swizzled tile addresses, the row predicates of every
    // column) would be hoisted out of the block loop and held in registers this kernel does not have
    asm volatile("" : "+v"(r));
    double a[16], x[16], my_invd;
#pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = D[ch_el(r, c)];
    const unsigned rejected = ch_diag_regs<true, false>(a, x, my_invd, j0, n, piv_tol, r);
    if (lane < 16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) D[ch_el(i, r)] = x[i];
    }
    return rejected ? 1 : 0;
}

}  // namespace esn
