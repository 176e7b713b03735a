// Readout training: W_out = (pinv(E[transient:]) @ teacher[transient:]).T  (pyESN.py:191-192)
// as a float64 Householder QR, one workgroup per trained ESN.
//
//   rows <  cols (4x8, N=128: 128 x 528): QR of A^T, minimum-norm solution
//                X = Q R^-T B   -- what pinv returns for an under-determined system
//   rows >= cols (SISO / 2x2: 512 x 104):           QR of [A | B], X = R^-1 (Q^T B)
//
// The working matrix is column-major in the caller's workspace (L2 resident);
// reflector j is applied to the trailing columns one wave per column.
//
// Ridge (an extension, the reference has none): W_out = argmin |E W^T - D_s|^2 + lambda |W|^2, lambda >= 0 absolute.
// The <true> instances of the three kernels run one workgroup per (group, lambda): workgroup `slot` reads E of group
// slot / n_ridge and lambda = ridge[slot], and writes W_out[slot], status[slot].  The QR kernel solves the augmented
// problem (tall: [A ; sqrt(lambda) I] w = [B ; 0]; wide: minimum norm of [A  sqrt(lambda) I] [w ; z] = B, first
// `cols` entries kept); the Cholesky kernels add lambda to the live Gram diagonal.  lambda = 0 takes the pinv path
// instruction for instruction; a negative or non-finite lambda gives status 2 and a zero W_out.
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

template <bool RG>
__global__ __launch_bounds__(1024) void readout_qr_kernel(SolveParams sp) {
    __shared__ double red[16];
    __shared__ double bc[4];
    const int slot = blockIdx.x;                            // RG: one workgroup per (group, lambda)
    const int g = RG ? slot / sp.n_ridge : slot;
    const int tid = threadIdx.x, nth = blockDim.x;
    const int lane = tid & 63, wv = tid >> 6, nwv = nth >> 6;
    const int n = sp.n, nrhs = sp.n_out;
    const int rows = sp.T - sp.transient, cols = sp.cols;
    int m = sp.m;
    double sq = 0.0;                                        // sqrt(lambda) > 0: the augmented problem, m grows by n
    if constexpr (RG) {
        if (ridge_rejects(sp, slot)) return;
        const double lam = sp.ridge[slot];
        if (lam > 0.0) { sq = sqrt(lam); m = sp.m + n; }
    }
    const bool aug = RG && sq > 0.0;
    double* M = sp.work + (size_t)slot * sp.work_stride;    // [n + (wide?0:nrhs)][m] column-major
    const int ncol_tot = sp.wide ? n : n + nrhs;
    double* R = M + (size_t)ncol_tot * m;                    // rhs / solution block [nrhs][m]
    double* rdiag = R + (size_t)nrhs * m;                    // [n]
    double* beta = rdiag + n;                                // [n]
    const double* Eg = sp.E + ((size_t)g * sp.T + sp.transient) * cols;
    const double* Dg = sp.D + ((size_t)g * sp.T + sp.transient) * nrhs;

    // ---- load -----------------------------------------------------------------
    if (sp.wide) {
        // M = A^T: column j = row j of A (contiguous in E); augmented: [A  sq I]^T
        if (aug) {
            for (size_t i = tid; i < (size_t)n * m; i += nth) {
                const int c = (int)(i / m), rr = (int)(i % m);
                M[i] = rr < cols ? Eg[(size_t)c * cols + rr] : (rr - cols == c ? sq : 0.0);
            }
        } else {
            for (size_t i = tid; i < (size_t)n * m; i += nth) M[i] = Eg[i];
        }
        for (int i = tid; i < nrhs * m; i += nth) {
            int o = i / m, j = i % m;
            double v = 0.0;
            if (j < n) {
                double sc = sp.t_scale ? sp.t_scale[(size_t)g * nrhs + o] : 1.0;
                double sh = sp.t_shift ? sp.t_shift[(size_t)g * nrhs + o] : 0.0;
                v = Dg[(size_t)j * nrhs + o] * sc + sh;
            }
            R[i] = v;
        }
    } else {
        // M = [A | B]: column c of A is strided in E; augmented: [A ; sq I | B ; 0]
        for (size_t i = tid; i < (size_t)n * m; i += nth) {
            int c = (int)(i / m), rr = (int)(i % m);
            if (aug && rr >= rows) M[i] = (rr - rows == c) ? sq : 0.0;
            else M[i] = Eg[(size_t)rr * cols + c];
        }
        for (int i = tid; i < nrhs * m; i += nth) {
            int o = i / m, rr = i % m;
            double sc = sp.t_scale ? sp.t_scale[(size_t)g * nrhs + o] : 1.0;
            double sh = sp.t_shift ? sp.t_shift[(size_t)g * nrhs + o] : 0.0;
            if (aug && rr >= rows) M[(size_t)(n + o) * m + rr] = 0.0;
            else M[(size_t)(n + o) * m + rr] = Dg[(size_t)rr * nrhs + o] * sc + sh;
        }
    }
    __syncthreads();

    // ---- Householder QR of the first n columns ----------------------------------
    for (int j = 0; j < n; ++j) {
        double* cj = M + (size_t)j * m;
        double part = 0.0;
        for (int i = j + tid; i < m; i += nth) { double x = cj[i]; part = fma(x, x, part); }
        part = wave_sum(part);
        if (lane == 0) red[wv] = part;
        __syncthreads();
        if (tid == 0) {
            double sigma = 0.0;
            for (int w = 0; w < nwv; ++w) sigma += red[w];
            double x0 = cj[j];
            double nx = sqrt(sigma);
            double alpha = (x0 >= 0.0) ? -nx : nx;
            double v0 = x0 - alpha;
            double vtv = sigma - x0 * x0 + v0 * v0;
            double b = (vtv > 0.0) ? 2.0 / vtv : 0.0;
            cj[j] = v0;
            rdiag[j] = alpha;
            beta[j] = b;
            bc[0] = b;
        }
        __syncthreads();
        const double b = bc[0];
        if (b != 0.0) {
            for (int c = j + 1 + wv; c < ncol_tot; c += nwv) {
                double* cc = M + (size_t)c * m;
                double dot = 0.0;
                for (int i = j + lane; i < m; i += 64) dot = fma(cj[i], cc[i], dot);
                dot = wave_sum(dot) * b;
                for (int i = j + lane; i < m; i += 64) cc[i] = fma(-dot, cj[i], cc[i]);
            }
        }
        __syncthreads();
    }

    // ---- rank check ---------------------------------------------------------------
    double rmax = 0.0;
    for (int j = tid; j < n; j += nth) rmax = fmax(rmax, fabs(rdiag[j]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) rmax = fmax(rmax, __shfl_down(rmax, off));
    if (lane == 0) red[wv] = rmax;
    __syncthreads();
    if (tid == 0) {
        double r = 0.0;
        for (int w = 0; w < nwv; ++w) r = fmax(r, red[w]);
        bc[1] = r * 1e-13;
        int bad = 0;
        for (int j = 0; j < n; ++j) bad |= (fabs(rdiag[j]) <= r * 1e-13);
        sp.status[slot] = bad ? 1 : 0;
    }
    __syncthreads();
    const double tol = bc[1];

    if (sp.wide) {
        // forward substitution R^T z = b, one wave per right-hand side (z overwrites b)
        for (int o = wv; o < nrhs; o += nwv) {
            double* z = R + (size_t)o * m;
            for (int j = 0; j < n; ++j) {
                const double* cj = M + (size_t)j * m;    // R[k][j], k<j, is cj[k]
                double acc = 0.0;
                for (int k = lane; k < j; k += 64) acc = fma(cj[k], z[k], acc);
                acc = wave_sum(acc);
                if (lane == 0) {
                    double d = rdiag[j];
                    z[j] = (fabs(d) > tol) ? (z[j] - acc) / d : 0.0;
                }
                __builtin_amdgcn_s_waitcnt(0);  // z[j] visible to this wave's later loads
                __builtin_amdgcn_wave_barrier();
            }
            // x = H_0 ... H_{n-1} [z; 0]
            for (int j = n - 1; j >= 0; --j) {
                const double* cj = M + (size_t)j * m;
                const double b = beta[j];
                if (b == 0.0) continue;
                double dot = 0.0;
                for (int i = j + lane; i < m; i += 64) dot = fma(cj[i], z[i], dot);
                dot = wave_sum(dot) * b;
                for (int i = j + lane; i < m; i += 64) z[i] = fma(-dot, cj[i], z[i]);
                __builtin_amdgcn_s_waitcnt(0);
                __builtin_amdgcn_wave_barrier();
            }
            double* wo = sp.W_out + ((size_t)slot * nrhs + o) * cols;
            for (int i = lane; i < cols; i += 64) wo[i] = z[i];
        }
    } else {
        // back substitution R x = (Q^T b)[0:n], one wave per right-hand side
        for (int o = wv; o < nrhs; o += nwv) {
            double* c = M + (size_t)(n + o) * m;     // transformed rhs; x overwrites c[0:n]
            for (int j = n - 1; j >= 0; --j) {
                double acc = 0.0;
                for (int k = j + 1 + lane; k < n; k += 64) acc = fma(M[(size_t)k * m + j], c[k], acc);
                acc = wave_sum(acc);
                if (lane == 0) {
                    double d = rdiag[j];
                    c[j] = (fabs(d) > tol) ? (c[j] - acc) / d : 0.0;
                }
                __builtin_amdgcn_s_waitcnt(0);
                __builtin_amdgcn_wave_barrier();
            }
            double* wo = sp.W_out + ((size_t)slot * nrhs + o) * cols;
            for (int i = lane; i < n; i += 64) wo[i] = c[i];
        }
    }
}

size_t solve_work_doubles(int rows, int cols, int n_out) {
    const bool wide = rows < cols;
    const size_t m = wide ? cols : rows, n = wide ? rows : cols;
    // matrix (+ rhs columns when tall) + rhs block + rdiag + beta, rounded to 16 B
    size_t d = (n + (wide ? 0 : n_out)) * m + (size_t)n_out * m + 2 * n;
    return (d + 1) & ~(size_t)1;
}

size_t solve_ridge_work_doubles(int rows, int cols, int n_out) {
    const bool wide = rows < cols;
    const size_t m = (size_t)rows + cols, n = wide ? rows : cols;      // the augmented matrix has rows + cols rows
    size_t d = (n + (wide ? 0 : n_out)) * m + (size_t)n_out * m + 2 * n;
    return (d + 1) & ~(size_t)1;
}

int launch_readout_solve(const double* E, const double* D, int n_groups, int T, int transient,
                         int cols, int n_out, const double* t_scale, const double* t_shift,
                         double* W_out, int* status, void* workspace, hipStream_t stream,
                         const double* ridge, int n_ridge) {
    SolveParams sp;
    const int rows = T - transient;
    sp.ridge = ridge; sp.n_ridge = n_ridge;
    sp.E = E; sp.E32 = nullptr; sp.D = D; sp.n_groups = n_groups; sp.T = T; sp.transient = transient;
    sp.cols = cols; sp.n_out = n_out; sp.t_scale = t_scale; sp.t_shift = t_shift;
    sp.W_out = W_out; sp.status = status;
    sp.work = reinterpret_cast<double*>(workspace);
    sp.work_stride = ridge ? solve_ridge_work_doubles(rows, cols, n_out) : solve_work_doubles(rows, cols, n_out);
    sp.wide = rows < cols;
    sp.m = sp.wide ? cols : rows;
    sp.n = sp.wide ? rows : cols;
    if (ridge) hipLaunchKernelGGL(readout_qr_kernel<true>, dim3(n_groups * n_ridge), dim3(1024), 0, stream, sp);
    else hipLaunchKernelGGL(readout_qr_kernel<false>, dim3(n_groups), dim3(1024), 0, stream, sp);
    return (int)hipGetLastError();
}

}  // namespace esn

// ---------------------------------------------------------------------------------
// Fast path for well-conditioned batched fits: normal equations in float64 with the
// Gram matrix (<= 128 x 128) and its Cholesky factor resident in LDS.
//   rows <  cols:  G = A A^T,  G alpha = B,      W_out^T = A^T alpha   (minimum norm)
//   rows >= cols:  G = A^T A,  G W_out^T = A^T B
// Error ~ cond(A)^2 eps: with the model's state noise cond(A) ~ 1e3, i.e.
// ~1e-10 -- far below the float32 harvest.  A non-positive / tiny pivot sets status=1 and
// the caller re-solves that group with the QR kernel.
//
// Two systems per CU: 512 threads and 80 KiB of LDS per workgroup, so that one system's
// serial phases (diagonal blocks, substitutions) run beside the other's Gram and E stream.
// LDS holds only the 36 lower 16x16 tiles of the Gram matrix, packed (72 KiB), and the
// right-hand sides (8 KiB).  A diagonal tile holds L11^-1 once factorised (L11 itself is not
// needed again); the E staging of the Gram phase and the W_out partial sums alias the tiles.
// ---------------------------------------------------------------------------------
namespace esn {

constexpr int CH_NP = 128;                  // padded Gram dimension
constexpr int CH_NT = 512;                  // threads: 8 waves, two per SIMD
constexpr int CH_NW = CH_NT / 64;
constexpr int CH_TILES = 36;                // lower 16x16 tiles of the Gram matrix
constexpr int CH_KC = 32;                   // k-chunk staged per pass
constexpr int CH_AS_LD = CH_NP + 16;        // staging row stride (doubles): rows k and k+1 of an operand read
                                            // fall on opposite halves of the 64 banks (no conflicts)
constexpr int CH_RHS = 8;                   // right-hand side columns (n_out <= 8), Bs[i][CH_RHS]
constexpr size_t CH_LDS = sizeof(double) * ((size_t)CH_TILES * 256 + (size_t)CH_NP * CH_RHS);   // 81 920 B
static_assert(2 * CH_KC * CH_AS_LD <= CH_TILES * 256, "E staging aliases the Gram tiles");

typedef double f64x4 __attribute__((ext_vector_type(4)));

// LDS-DMA rings of the wide float32 instance (sp.dma): E goes global -> LDS by buffer_load ... lds, 16 B per
// lane, with no register staging.  Both rings live in the tile area, which is dead in phases 1 and 5.
constexpr int CH_RING = 4;                  // Gram: 4 buffers of one 32-k chunk (3 chunks in flight)
constexpr int CH_RBUF = CH_KC * CH_NP * 4;  // 16 KB: 128 rows x 32 k as float32
constexpr int CH_WRING = 3;                 // W_out: 3 buffers (2 chunks in flight) of three part segments
constexpr int CH_WSEG = 8192;               // rows of one part per chunk, padded to whole 1 KB DMA pieces
constexpr int CH_WROWS = 4;                 // at most 4 rows of a part per chunk (the row loop is unrolled)
static_assert(CH_RING * CH_RBUF <= CH_TILES * 256 * 8, "Gram ring aliases the Gram tiles");
static_assert(CH_WRING * 3 * CH_WSEG <= CH_TILES * 256 * 8, "W_out ring aliases the Gram tiles");

__device__ __forceinline__ __amdgpu_buffer_rsrc_t ch_rsrc(const void* ptr, int bytes) {
    const uint64_t a = (uint64_t)reinterpret_cast<uintptr_t>(ptr);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>((uintptr_t)(((uint64_t)hi << 32) | lo)), 0,
                                             __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
// 16 bytes per lane from E at byte offset voff (>= num_records: zeros, no traffic) to the 1 KB at dst
__device__ __forceinline__ void ch_dma16(__amdgpu_buffer_rsrc_t rs, char* dst, int voff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, voff, 0, 0, 0);
}
constexpr int CH_OOR = 0x7ffffff0;          // byte offset past any E a launch accepts
// this wave's DMA pieces, except the last `pending` issued, have landed in LDS; its LDS reads have returned
__device__ __forceinline__ void ch_wait_dma(int pending) {
    switch (pending) {
        case 4: asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); break;
    }
}

// W_out ring: a thread's 16 B of one E row and the row's CH_RHS alpha values.  hipcc guards every LDS read it can
// see with vmcnt(0) while an LDS-DMA is pending, which would drain the ring on each row; these reads are ordered
// after the DMA by the ring's counted vmcnt and barrier instead, and waited for here.
__device__ __forceinline__ void ch_wrow(const char* e, const double* al, float (&a)[4], double (&b)[8]) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    const uint32_t ea = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)e;
    const uint32_t ba = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) double*)al;
    f32x4 ev;
    f64x2 b0, b1, b2, b3;
    asm volatile("ds_read_b128 %0, %5\n\tds_read_b128 %1, %6\n\tds_read_b128 %2, %6 offset:16\n\t"
                 "ds_read_b128 %3, %6 offset:32\n\tds_read_b128 %4, %6 offset:48\n\ts_waitcnt lgkmcnt(0)"
                 : "=v"(ev), "=v"(b0), "=v"(b1), "=v"(b2), "=v"(b3) : "v"(ea), "v"(ba) : "memory");
    a[0] = ev.x; a[1] = ev.y; a[2] = ev.z; a[3] = ev.w;
    b[0] = b0.x; b[1] = b0.y; b[2] = b1.x; b[3] = b1.y; b[4] = b2.x; b[5] = b2.y; b[6] = b3.x; b[7] = b3.y;
}

// first double of lower tile (ti, tj), ti >= tj
__device__ __forceinline__ int ch_tile(int ti, int tj) { return (ti * (ti + 1) / 2 + tj) * 256; }
// element (r, c) of a tile: row-major, the column XORed with the row pair.  MFMA operand reads by row
// (r = lane % 16, c = k + lane / 16) and by column (r = k + lane / 16, c = lane % 16), the 16-lane row
// reads of the diagonal factorisation and the accumulator stores all hit 32 distinct 8-byte banks.
__device__ __forceinline__ int ch_el(int r, int c) { return r * 16 + (c ^ (r & ~1)); }

__device__ __forceinline__ void ch_load4(const float* p, float (&v)[4]) {
    const float4 x = *reinterpret_cast<const float4*>(p);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
}
__device__ __forceinline__ void ch_load4(const double* p, double (&v)[4]) {
    const double2 x = *reinterpret_cast<const double2*>(p), y = *reinterpret_cast<const double2*>(p + 2);
    v[0] = x.x; v[1] = x.y; v[2] = y.x; v[3] = y.y;
}
__device__ __forceinline__ const float* ch_src(const SolveParams& sp, float*) { return sp.E32; }
__device__ __forceinline__ const double* ch_src(const SolveParams& sp, double*) { return sp.E; }

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

template <typename TE, bool wide, bool RG>
__global__ __launch_bounds__(CH_NT) __attribute__((amdgpu_waves_per_eu(4))) void readout_chol_kernel(SolveParams sp) {
    extern __shared__ __attribute__((aligned(16))) char chol_smem[];
    double* Gs = reinterpret_cast<double*>(chol_smem);             // 36 packed tiles            (phase 2-4)
    double* As = Gs;                                                // [2][CH_KC][CH_AS_LD] staging (phase 1)
    double* Bs = Gs + CH_TILES * 256;                               // [CH_NP][CH_RHS] rhs / solution
    const int slot = blockIdx.x, tid = threadIdx.x;                 // RG: one workgroup per (group, lambda)
    const int g = RG ? slot / sp.n_ridge : slot;
    if constexpr (RG) {
        if (ridge_rejects(sp, slot)) return;
    }
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int rows = sp.T - sp.transient, cols = sp.cols, nrhs = sp.n_out;
    const int n = wide ? rows : cols;      // Gram dimension (<= CH_NP)
    const int m = wide ? cols : rows;      // contraction length
    const int ntile = (n + 15) / 16;
    const TE* A = ch_src(sp, (TE*)nullptr) + ((size_t)g * sp.T + sp.transient) * cols;    // [rows][cols]
    const double* Dg = sp.D + ((size_t)g * sp.T + sp.transient) * nrhs;

    // ---- phase 1: G = sum_k a_k a_k^T on the float64 matrix pipe ------------------------------
    // v_mfma_f64_16x16x4_f64 (A[l%16][l/16], B[l/16][l%16], C reg i: row 4i + l/16, col l%16) runs at
    // the vector-FMA rate on gfx950 (64 cycles, probe in tools/mfma_layout_probe.hip).  Only the 36 lower
    // 16x16 tiles are formed: tile t goes to wave t % 8, so waves w and w + 4 (one SIMD) carry 9 between them.
    int g_ti[5], g_tj[5];
    const int g_cnt = wv < 4 ? 5 : 4;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int t = wv + CH_NW * q < CH_TILES ? wv + CH_NW * q : 0;
        int ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
        g_ti[q] = ti;
        g_tj[q] = t - ti * (ti + 1) / 2;
    }
    f64x4 acc[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) acc[q] = f64x4{0.0, 0.0, 0.0, 0.0};
    // tall case also needs A^T B: thread (o, i) = (e / 128, e % 128), e = tid + 512 p
    double atb[2] = {0.0, 0.0};
    // A chunk is 32 k x 128 i; each thread moves two runs of 4 elements that are contiguous in E (16-byte
    // loads when sp.vec): 4 consecutive k of one Gram row (wide) or 4 consecutive Gram rows of one k (tall).
    // Wide: a 16-lane group takes 16 rows, so the 8-byte LDS stores of a group hit 32 distinct banks.
    auto run_of = [&](int p, int& i, int& kk) {
        const int e = tid + CH_NT * p;
        if (wide) { i = (e & 15) + 16 * ((e >> 7) & 7); kk = 4 * ((e >> 4) & 7); }
        else      { kk = e >> 5; i = 4 * (e & 31); }
    };
    TE stg[2][4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            int i, kk;
            run_of(p, i, kk);
            const int k = k0 + kk;
            int nv = wide ? (i < n ? m - k : 0) : (k < m ? n - i : 0);
            nv = nv < 0 ? 0 : (nv > 4 ? 4 : nv);
            const TE* src = A + (wide ? (size_t)i * cols + k : (size_t)k * cols + i);
            if (nv == 4 && sp.vec) {
                ch_load4(src, stg[p]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) stg[p][j] = j < nv ? src[j] : (TE)0;
            }
        }
    };
    auto commit = [&](double* dst) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            int i, kk;
            run_of(p, i, kk);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (wide) dst[(kk + j) * CH_AS_LD + i] = (double)stg[p][j];
                else      dst[kk * CH_AS_LD + i + j] = (double)stg[p][j];
            }
        }
    };
    double* Abuf[2] = {As, As + CH_KC * CH_AS_LD};
    const int m_run = (sp.skip & 1) ? CH_KC : m;
    constexpr bool can_dma = wide && sizeof(TE) == 4;
    const bool dma = can_dma && sp.dma && sp.vec;
#ifdef ESN_STAMPS
    unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_ph[4] = {0, 0, 0, 0};
    ESN_STAMP(st_k0);
#endif
    if constexpr (can_dma) {
        if (dma) {
            // Float32 chunks of 32 k x 128 rows through a ring of CH_RING buffers, CH_RING - 1 in flight.  DMA
            // piece j of wave w covers rows 8 d .. 8 d + 7 (d = 2 w + j) and all eight k-quads of the chunk: lane l
            // fetches the 16 B of row 8 d + (l & 7), k-quad l >> 3.  Byte (r, k) of a buffer is therefore
            // 1024 (r >> 3) + 128 (k >> 2) + 16 (r & 7) + 4 (k & 3): an operand read (16 rows x 4 k) takes two LDS
            // cycles per lane group, the least a 4-byte read of 16-byte runs allows, and steps k4 apart by a
            // constant offset.  Rows >= n are past num_records, k-quads >= m get an out-of-range offset: both land
            // as zeros.  The MFMA sequence and k order are those of the register-staged pass (bitwise the same G).
            char* ring = chol_smem;
            const __amdgpu_buffer_rsrc_t ers = ch_rsrc(A, n * cols * 4);
            const int kq = lane >> 3;
            int roff[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) roff[j] = ((16 * wv + 8 * j + (lane & 7)) * cols + 4 * kq) * 4;
            const int nch = (m_run + CH_KC - 1) / CH_KC;
            auto issue = [&](int c, int b) {
                const int k0 = c * CH_KC;
                const bool ok = k0 + 4 * kq < m;
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    ch_dma16(ers, ring + b * CH_RBUF + (2 * wv + j) * 1024, ok ? roff[j] + 4 * k0 : CH_OOR);
            };
#pragma unroll
            for (int c = 0; c < CH_RING - 1; ++c)
                if (c < nch) issue(c, c);
            const int lbase = 1024 * (lr >> 3) + 16 * (lr & 7) + 4 * lq;
            for (int c = 0, b = 0; c < nch; ++c, b = (b + 1 == CH_RING ? 0 : b + 1)) {
#ifdef ESN_STAMPS
                ESN_STAMP(s0);
#endif
                const int later = nch - 1 - c < CH_RING - 2 ? nch - 1 - c : CH_RING - 2;
                ch_wait_dma(2 * later);
#ifdef ESN_STAMPS
                ESN_STAMP(s1);
#endif
                __builtin_amdgcn_s_barrier();                       // chunk c landed for all; chunk c-1 read by all
                if (c + CH_RING - 1 < nch) issue(c + CH_RING - 1, b == 0 ? CH_RING - 1 : b - 1);
                const char* buf = ring + b * CH_RBUF + lbase;
                const float* pa[5];
                const float* pb[5];
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    pa[q] = reinterpret_cast<const float*>(buf + 2048 * g_ti[q]);
                    pb[q] = reinterpret_cast<const float*>(buf + 2048 * g_tj[q]);
                }
#ifdef ESN_STAMPS
                ESN_STAMP(s2);
                {   // operand-read latency: one read of the chunk, waited for (the stamp waits lgkmcnt(0))
                    float x = pa[0][0];
                    asm volatile("" :: "v"(x));
                }
                ESN_STAMP(s3);
#endif
                // the tile count is hoisted out of the k4 steps: a full chunk is one straight block, so its
                // operand reads run ahead of the MFMAs across steps
                auto step = [&](int s, auto cnt) {
#pragma unroll
                    for (int q = 0; q < decltype(cnt)::value; ++q)
                        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)pa[q][32 * s], (double)pb[q][32 * s], acc[q], 0, 0, 0);
                };
                const int kmax = (m - c * CH_KC < CH_KC) ? m - c * CH_KC : CH_KC;
                if (kmax == CH_KC && g_cnt == 5) {
#pragma unroll
                    for (int s = 0; s < CH_KC / 4; ++s) step(s, std::integral_constant<int, 5>());
                } else if (kmax == CH_KC) {
#pragma unroll
                    for (int s = 0; s < CH_KC / 4; ++s) step(s, std::integral_constant<int, 4>());
                } else if (g_cnt == 5) {
                    for (int s = 0; s < kmax / 4; ++s) step(s, std::integral_constant<int, 5>());
                } else {
                    for (int s = 0; s < kmax / 4; ++s) step(s, std::integral_constant<int, 4>());
                }
#ifdef ESN_STAMPS
                ESN_STAMP(s4);
                st_acc[0] += s1 - s0; st_acc[1] += s2 - s1; st_acc[2] += s3 - s2; st_acc[3] += s4 - s3;
#endif
            }
            __syncthreads();                                        // every DMA waited for; the ring is read out
        }
    }
    // chunk c is multiplied out of Abuf[c & 1] while chunk c+1 is in flight to registers (with two workgroups
    // per CU, the partner's work covers what one chunk of MFMAs does not)
    for (int k0 = 0, cur = 0; k0 < (dma ? 0 : m_run); k0 += CH_KC, cur ^= 1) {
        if (k0 == 0) {
            fetch(0);
            commit(Abuf[0]);
            __syncthreads();
        }
#ifdef ESN_STAMPS
        ESN_STAMP(s0);
#endif
        if (k0 + CH_KC < m_run) fetch(k0 + CH_KC);
        const double* Ac = Abuf[cur];
        const int kmax = (m - k0 < CH_KC) ? m - k0 : CH_KC;
        // (rows past m and columns past n of the chunk are zero-filled by fetch)
        const double* slab0 = Ac + lq * CH_AS_LD + lr;
        for (int k4 = 0; k4 < kmax; k4 += 4) {
            const double* slab = slab0 + k4 * CH_AS_LD;
#pragma unroll
            for (int q = 0; q < 5; ++q)
                if (q < g_cnt)
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(slab[g_ti[q] * 16], slab[g_tj[q] * 16], acc[q], 0, 0, 0);
        }
        if constexpr (!wide) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int e = tid + CH_NT * p, o = e / CH_NP, i = e % CH_NP;
                if (o < nrhs) {
                    const double sc = sp.t_scale ? sp.t_scale[(size_t)g * nrhs + o] : 1.0;
                    const double sh = sp.t_shift ? sp.t_shift[(size_t)g * nrhs + o] : 0.0;
                    for (int kk = 0; kk < kmax; ++kk)
                        atb[p] = fma(Ac[kk * CH_AS_LD + i], Dg[(size_t)(k0 + kk) * nrhs + o] * sc + sh, atb[p]);
                }
            }
        }
#ifdef ESN_STAMPS
        ESN_STAMP(s1);
#endif
        if (k0 + CH_KC < m_run) commit(Abuf[cur ^ 1]);
#ifdef ESN_STAMPS
        ESN_STAMP(s2);
#endif
        __syncthreads();
#ifdef ESN_STAMPS
        ESN_STAMP(s3);
        st_acc[3] += s1 - s0; st_acc[0] += s2 - s1; st_acc[1] += s3 - s2;    // MFMA issue | load wait + commit | barrier
#endif
    }
#ifdef ESN_STAMPS
    ESN_STAMP(st_k1);
#endif

    // ---- phase 2: G and the right-hand sides into LDS ----------------------------------------
#pragma unroll
    for (int q = 0; q < 5; ++q)
        if (q < g_cnt) {
            double* T = Gs + ch_tile(g_ti[q], g_tj[q]);
#pragma unroll
            for (int i = 0; i < 4; ++i) T[ch_el(4 * i + lq, lr)] = acc[q][i];
        }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int e = tid + CH_NT * p;
        if (wide) {
            const int i = e / CH_RHS, o = e % CH_RHS;
            double v = 0.0;
            if (i < n && o < nrhs) {
                const double sc = sp.t_scale ? sp.t_scale[(size_t)g * nrhs + o] : 1.0;
                const double sh = sp.t_shift ? sp.t_shift[(size_t)g * nrhs + o] : 0.0;
                v = Dg[(size_t)i * nrhs + o] * sc + sh;
            }
            Bs[e] = v;
        } else {
            const int o = e / CH_NP, i = e % CH_NP;
            Bs[i * CH_RHS + o] = (o < nrhs && i < n) ? atb[p] : 0.0;
        }
    }
    __syncthreads();
    if constexpr (RG) {
        // ridge: lambda on the live diagonal only (the padding rows of a ragged last tile stay as they are), before
        // dmax / piv_tol are taken; + 0.0 leaves a non-negative diagonal bitwise as it is
        const double lam = sp.ridge[slot];
        for (int i = tid; i < n; i += CH_NT) Gs[ch_tile(i >> 4, i >> 4) + ch_el(i & 15, i & 15)] += lam;
        __syncthreads();
    }

    // ---- phase 3: blocked right-looking Cholesky, 16-column blocks ----------------------------
    // per block kb: (b) panel L21 = A21 L11^-T, one tile per wave; (c) trailing update A22 -= L21 L21^T of
    // the lower tiles, where wave 0 takes the next diagonal tile and goes on to factorise and invert it (a)
    // while waves 1-7 update the rest.  Two barriers per 16 columns; all products are 16x16x4 float64
    // MFMAs out of / into the packed tiles.
    int bad = 0;                                                    // wave 0: a live pivot was rejected
    const int nblk = (sp.skip & 2) ? 1 : ntile;
    double piv_tol = 0.0;
    if (wv == 0) {
        double dmax = 0.0;                                          // largest diagonal entry
        for (int i = lane; i < n; i += 64) dmax = fmax(dmax, Gs[ch_tile(i >> 4, i >> 4) + ch_el(i & 15, i & 15)]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, off));
        piv_tol = dmax * 1e-14;
    }
    for (int kb = -1; kb < nblk; ++kb) {                            // kb = -1: the first diagonal block only
#ifdef ESN_STAMPS
        ESN_STAMP(f0);
        unsigned long long f1 = f0, f2 = f0;
#endif
        if (kb >= 0) {   // (b) panel: row tile rt of L21 = A21[rt] * L11^-T  (B operand [k][n] = L11^-1[n][k])
            const int rt = kb + 1 + wv;
            if (rt < ntile) {
                const double* Li = Gs + ch_tile(kb, kb);

                double* T = Gs + ch_tile(rt, kb);
                f64x4 c = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k0 = 0; k0 < 16; k0 += 4)
                    c = __builtin_amdgcn_mfma_f64_16x16x4f64(T[ch_el(lr, k0 + lq)], Li[ch_el(lr, k0 + lq)], c, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) T[ch_el(4 * i + lq, lr)] = c[i];
            }
        }
        if (kb >= 0) {   // (c) trailing update of the lower tiles (ti >= tj > kb): A22[ti][tj] -= L21[ti] L21[tj]^T;
            // t = 0 is the next diagonal tile (wave 0), waves 1..7 take t = 1, 2, ...
#ifdef ESN_STAMPS
            ESN_STAMP_SET(f1);
#endif
            __syncthreads();
#ifdef ESN_STAMPS
            ESN_STAMP_SET(f2);
#endif
            const int mt = ntile - kb - 1, cnt = mt * (mt + 1) / 2;
            for (int t = wv; t < cnt; t += (wv == 0 ? cnt : CH_NW - 1)) {
                int di = 0;
                while ((di + 1) * (di + 2) / 2 <= t) ++di;
                const int ti = kb + 1 + di, tj = kb + 1 + t - di * (di + 1) / 2;
                double* C = Gs + ch_tile(ti, tj);
                const double* La = Gs + ch_tile(ti, kb);
                const double* Lb = Gs + ch_tile(tj, kb);
                f64x4 c;
#pragma unroll
                for (int i = 0; i < 4; ++i) c[i] = C[ch_el(4 * i + lq, lr)];
#pragma unroll
                for (int k0 = 0; k0 < 16; k0 += 4)
                    c = __builtin_amdgcn_mfma_f64_16x16x4f64(-La[ch_el(lr, k0 + lq)], Lb[ch_el(lr, k0 + lq)], c, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) C[ch_el(4 * i + lq, lr)] = c[i];
            }
        }
#ifdef ESN_STAMPS
        ESN_STAMP(f3);
#endif
        if (wv == 0 && kb + 1 < nblk) bad |= ch_factor_diag(Gs + ch_tile(kb + 1, kb + 1), 16 * (kb + 1), n, piv_tol, lane);
#ifdef ESN_STAMPS
        ESN_STAMP(f4);
#endif
        __syncthreads();
#ifdef ESN_STAMPS
        ESN_STAMP(f5);
        // panel + trailing update | the two barrier waits | the diagonal tile (wave 0)
        st_ph[0] += (f1 - f0) + (f3 - f2); st_ph[1] += (f2 - f1) + (f5 - f4); st_ph[2] += f4 - f3;
#endif
    }

#ifdef ESN_STAMPS
    ESN_STAMP(st_k2);
#endif
    // ---- phase 4: L L^T alpha = B by 16-row tiles ---------------------------------------------
    // Forward, step I: z_I = L_II^-1 b_I, then b_J -= L_JI z_I for J > I (wave J - I - 1).  Backward, step I:
    // x_I = L_II^-T z_I, then z_J -= L_IJ^T x_I for J < I (wave J).  Each product is four 16x16x4 MFMAs
    // (columns = right-hand sides, lanes with lr >= 8 carry zeros); the accumulator layout of z_I is the B
    // operand layout of the update, so every updating wave forms z_I itself.  Wave 7 forms it as well and
    // stores it one step later, when no wave reads those rows any more.  One barrier per tile step.
    if (!(sp.skip & 4)) {
        const bool bl = lr < CH_RHS;
        f64x4 keep = {0.0, 0.0, 0.0, 0.0};
        int keep_t = -1;
        auto rhs_tile = [&](int I) -> f64x4 {                       // rows 16 I + 4 i + lq, column lr
            f64x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = bl ? Bs[(16 * I + 4 * i + lq) * CH_RHS + lr] : 0.0;
            return v;
        };
        auto put_tile = [&](int I, const f64x4& v) {
            if (bl) {
#pragma unroll
                for (int i = 0; i < 4; ++i) Bs[(16 * I + 4 * i + lq) * CH_RHS + lr] = v[i];
            }
        };
        auto flush = [&]() {
            if (wv == CH_NW - 1 && keep_t >= 0) put_tile(keep_t, keep);
            keep_t = -1;
        };
        for (int I = 0; I < ntile; ++I) {                           // forward: L z = b
            flush();
            const int J = I + 1 + wv;
            const bool upd = J < ntile;
            if (upd || wv == CH_NW - 1) {
                const double* Li = Gs + ch_tile(I, I);
                const f64x4 b = rhs_tile(I);
                f64x4 z = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    z = __builtin_amdgcn_mfma_f64_16x16x4f64(Li[ch_el(lr, 4 * s + lq)], b[s], z, 0, 0, 0);
                if (upd) {
                    const double* L = Gs + ch_tile(J, I);
                    f64x4 c = rhs_tile(J);
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        c = __builtin_amdgcn_mfma_f64_16x16x4f64(-L[ch_el(lr, 4 * s + lq)], z[s], c, 0, 0, 0);
                    put_tile(J, c);
                } else {
                    keep = z;
                    keep_t = I;
                }
            }
            __syncthreads();
        }
        flush();
        __syncthreads();
        for (int I = ntile - 1; I >= 0; --I) {                      // backward: L^T x = z
            flush();
            const int J = wv;
            const bool upd = J < I;
            if (upd || wv == CH_NW - 1) {
                const double* Li = Gs + ch_tile(I, I);
                const f64x4 zi = rhs_tile(I);
                f64x4 x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    x = __builtin_amdgcn_mfma_f64_16x16x4f64(Li[ch_el(4 * s + lq, lr)], zi[s], x, 0, 0, 0);
                if (upd) {
                    const double* L = Gs + ch_tile(I, J);
                    f64x4 c = rhs_tile(J);
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        c = __builtin_amdgcn_mfma_f64_16x16x4f64(-L[ch_el(4 * s + lq, lr)], x[s], c, 0, 0, 0);
                    put_tile(J, c);
                } else {
                    keep = x;
                    keep_t = I;
                }
            }
            __syncthreads();
        }
        flush();
        __syncthreads();
    }

#ifdef ESN_STAMPS
    ESN_STAMP(st_k3);
#endif
    // ---- phase 5: W_out ---------------------------------------------------------------------
    if constexpr (wide) {
        // W_out[o][c] = sum_i A[i][c] alpha[i][o].  Every element of A is fetched once, by 16-byte loads:
        // thread (part, unit) sums a third of the rows for the unit's CPT columns and all nrhs outputs;
        // parts 1 and 2 leave their sums in LDS (the factor is no longer needed), part 0 adds them.
        constexpr int CPT = 16 / sizeof(TE);
        const int nunit = cols / CPT;
        int parts = nunit > 0 ? CH_NT / nunit : 0;
        parts = parts > 3 ? 3 : parts;
        if (sp.vec && cols % CPT == 0 && parts > 0 && (parts - 1) * CH_RHS * cols <= CH_TILES * 256 && !(sp.skip & 8)) {
            double* part = Gs;                               // [parts - 1][CH_RHS][cols]
            const int pt = tid / nunit, un = tid - pt * nunit;
            double w[CPT][CH_RHS];
#pragma unroll
            for (int c = 0; c < CPT; ++c)
#pragma unroll
                for (int o = 0; o < CH_RHS; ++o) w[c][o] = 0.0;
            const int per = (n + parts - 1) / parts;
            int rw = CH_WSEG / (cols * 4);                   // rows of each part per W_out chunk
            rw = rw > CH_WROWS ? CH_WROWS : rw;
            bool wdma = false;
            if constexpr (can_dma) {
              wdma = dma && rw > 0;
              if (wdma) {
                // The same sums, E streamed through a ring of CH_WRING buffers: chunk c holds rows
                // i0 + rw c .. i0 + rw c + rw - 1 of each part in that part's CH_WSEG segment (row-major as in E),
                // so each thread reads its 16 B of a row with one conflict-free LDS read.  Wave w fetches 1 KB piece
                // w of every segment; bytes past a segment's rows get an out-of-range offset and land as zeros.
                // Row order per thread and the combine order of the parts are unchanged (bitwise the same W_out).
                char* ring = chol_smem;
                const __amdgpu_buffer_rsrc_t ers = ch_rsrc(A, n * cols * 4);
                const int rowb = cols * 4;
                const int nch = (per + rw - 1) / rw;
                auto issue = [&](int c, int b) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const int r0 = j * per + c * rw;
                        int nr = (j < parts) ? ((j + 1) * per < n ? (j + 1) * per : n) - r0 : 0;
                        nr = nr < 0 ? 0 : (nr > rw ? rw : nr);
                        const int off = 1024 * wv + 16 * lane;
                        ch_dma16(ers, ring + (b * 3 + j) * CH_WSEG + 1024 * wv, off < nr * rowb ? r0 * rowb + off : CH_OOR);
                    }
                };
#pragma unroll
                for (int c = 0; c < CH_WRING - 1; ++c)
                    if (c < nch) issue(c, c);
                const int i0 = pt * per, i1 = (i0 + per < n) ? i0 + per : n;
                for (int c = 0, b = 0; c < nch; ++c, b = (b + 1 == CH_WRING ? 0 : b + 1)) {
#ifdef ESN_STAMPS
                    ESN_STAMP(s0);
#endif
                    ch_wait_dma(nch - 1 - c < CH_WRING - 2 ? 3 * (nch - 1 - c) : 3 * (CH_WRING - 2));
#ifdef ESN_STAMPS
                    ESN_STAMP(s1);
#endif
                    __builtin_amdgcn_s_barrier();
                    if (c + CH_WRING - 1 < nch) issue(c + CH_WRING - 1, b == 0 ? CH_WRING - 1 : b - 1);
#ifdef ESN_STAMPS
                    ESN_STAMP(s2);
#endif
                    if (pt < parts) {
                        const char* seg = ring + (b * 3 + pt) * CH_WSEG + CPT * sizeof(TE) * un;
                        const int ib = i0 + c * rw;
                        const int nr = ((ib + rw < i1) ? ib + rw : i1) - ib;
#pragma unroll
                        for (int rr = 0; rr < CH_WROWS; ++rr) {
                            if (rr >= nr) break;
                            const int i = ib + rr;
                            float a[4];
                            double al[CH_RHS];
                            ch_wrow(seg + rr * rowb, Bs + i * CH_RHS, a, al);
#pragma unroll
                            for (int o = 0; o < CH_RHS; ++o)
                                if (o < nrhs) {
#pragma unroll
                                    for (int cc = 0; cc < CPT; ++cc) w[cc][o] = fma((double)a[cc], al[o], w[cc][o]);
                                }
                        }
                    }
#ifdef ESN_STAMPS
                    ESN_STAMP(s3);
                    st_acc[4] += s1 - s0; st_acc[5] += s2 - s1; st_acc[6] += s3 - s2;
#endif
                }
                __syncthreads();                             // the ring is read out: the part sums alias it
                if (pt > 0 && pt < parts) {
#pragma unroll
                    for (int o = 0; o < CH_RHS; ++o)
                        if (o < nrhs) {
#pragma unroll
                            for (int c = 0; c < CPT; ++c) part[((pt - 1) * CH_RHS + o) * cols + CPT * un + c] = w[c][o];
                        }
                }
              }
            }
            if (!wdma && pt < parts) {
                const int i0 = pt * per, i1 = (i0 + per < n) ? i0 + per : n;
                const TE* ac = A + (size_t)CPT * un;
#pragma unroll 4
                for (int i = i0; i < i1; ++i) {
                    TE a[CPT];
                    if constexpr (CPT == 4) {
                        ch_load4(ac + (size_t)i * cols, a);
                    } else {
                        const double2 ad = *reinterpret_cast<const double2*>(ac + (size_t)i * cols);
                        a[0] = ad.x; a[1] = ad.y;
                    }
#pragma unroll
                    for (int o = 0; o < CH_RHS; ++o)
                        if (o < nrhs) {
                            const double al = Bs[i * CH_RHS + o];
#pragma unroll
                            for (int c = 0; c < CPT; ++c) w[c][o] = fma((double)a[c], al, w[c][o]);
                        }
                }
                if (pt > 0) {
#pragma unroll
                    for (int o = 0; o < CH_RHS; ++o)
                        if (o < nrhs) {
#pragma unroll
                            for (int c = 0; c < CPT; ++c) part[((pt - 1) * CH_RHS + o) * cols + CPT * un + c] = w[c][o];
                        }
                }
            }
            __syncthreads();
            if (pt == 0) {
#pragma unroll
                for (int o = 0; o < CH_RHS; ++o)
                    if (o < nrhs) {
#pragma unroll
                        for (int c = 0; c < CPT; ++c) {
                            double v = w[c][o];
                            for (int q = 1; q < parts; ++q) v += part[((q - 1) * CH_RHS + o) * cols + CPT * un + c];
                            sp.W_out[((size_t)slot * nrhs + o) * cols + CPT * un + c] = v;
                        }
                    }
            }
        } else {
            for (int c = tid; c < ((sp.skip & 8) ? 0 : cols); c += CH_NT) {
                double w[CH_RHS];
#pragma unroll
                for (int o = 0; o < CH_RHS; ++o) w[o] = 0.0;
#pragma unroll 8
                for (int i = 0; i < n; ++i) {
                    const double a = (double)A[(size_t)i * cols + c];
#pragma unroll
                    for (int o = 0; o < CH_RHS; ++o)
                        if (o < nrhs) w[o] = fma(a, Bs[i * CH_RHS + o], w[o]);
                }
#pragma unroll
                for (int o = 0; o < CH_RHS; ++o)
                    if (o < nrhs) sp.W_out[((size_t)slot * nrhs + o) * cols + c] = w[o];
            }
        }
    } else {
        for (int e = tid; e < nrhs * cols; e += CH_NT) {
            const int o = e / cols, c = e % cols;
            sp.W_out[((size_t)slot * nrhs + o) * cols + c] = Bs[c * CH_RHS + o];
        }
    }
    if (tid == 0) sp.status[slot] = bad;
#ifdef ESN_STAMPS
    ESN_STAMP(st_k4);
    // row wv: Gram wait | barrier | operand read | MFMA issue, W_out wait | barrier | rows; row 8 + wv: phase totals
    if (sp.stamps && slot == 0 && lane == 0) {
        for (int i = 0; i < 7; ++i) sp.stamps[wv * 8 + i] = st_acc[i];
        sp.stamps[(8 + wv) * 8 + 0] = st_k1 - st_k0;
        sp.stamps[(8 + wv) * 8 + 1] = st_k2 - st_k1;
        sp.stamps[(8 + wv) * 8 + 2] = st_k3 - st_k2;
        sp.stamps[(8 + wv) * 8 + 3] = st_k4 - st_k3;
        sp.stamps[(8 + wv) * 8 + 4] = st_k4 - st_k0;
        for (int i = 0; i < 3; ++i) sp.stamps[(8 + wv) * 8 + 5 + i] = st_ph[i];      // the factor phase, split
    }
#endif
}

int launch_readout_chol(const double* E, const float* E32, const double* D, int n_groups, int T, int transient,
                        int cols, int n_out, const double* t_scale, const double* t_shift,
                        double* W_out, int* status, hipStream_t stream, const double* ridge, int n_ridge) {
    SolveParams sp;
    sp.E32 = E32;
    sp.ridge = ridge; sp.n_ridge = n_ridge;
    const int rows = T - transient;
    const int n = rows < cols ? rows : cols;
    if (n > CH_NP || n_out > CH_RHS) return -1;
    sp.E = E; sp.D = D; sp.n_groups = n_groups; sp.T = T; sp.transient = transient;
    sp.cols = cols; sp.n_out = n_out; sp.t_scale = t_scale; sp.t_shift = t_shift;
    sp.W_out = W_out; sp.status = status; sp.work = nullptr; sp.work_stride = 0;
    sp.wide = rows < cols; sp.m = sp.wide ? cols : rows; sp.n = n;
    sp.skip = knobs().chol_skip;
    sp.dma = knobs().chol_dma;
    sp.part_ok = 0;
#ifdef ESN_STAMPS
    sp.stamps = stamp_buffer();
#else
    sp.stamps = nullptr;
#endif
    // 16-byte loads of 4 consecutive elements: every row of every group starts 16-byte aligned
    const uintptr_t base = E32 ? (uintptr_t)E32 : (uintptr_t)E;
    sp.vec = (base % 16 == 0) && (cols % (E32 ? 4 : 2) == 0);
    void (*fn)(SolveParams);
    if (ridge)
        fn = E32 ? (sp.wide ? readout_chol_kernel<float, true, true> : readout_chol_kernel<float, false, true>)
                 : (sp.wide ? readout_chol_kernel<double, true, true> : readout_chol_kernel<double, false, true>);
    else
        fn = E32 ? (sp.wide ? readout_chol_kernel<float, true, false> : readout_chol_kernel<float, false, false>)
                 : (sp.wide ? readout_chol_kernel<double, true, false> : readout_chol_kernel<double, false, false>);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)CH_LDS);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fn, dim3(ridge ? n_groups * n_ridge : n_groups), dim3(CH_NT), CH_LDS, stream, sp);
    return (int)hipGetLastError();
}

}  // namespace esn

// ---------------------------------------------------------------------------------
// The same normal-equations solve for Gram dimensions 129..512 (4x8 at N = 512: 512 x 528;
// N_res = 300 at N = 512: 512 x 316), where neither the Gram matrix (2 MB) nor its factor fits LDS.
// One workgroup per trained ESN, the Gram matrix / factor column-major in a caller workspace
// (L2 / Infinity Cache resident), every O(n^3) part on the float64 matrix pipe:
//   phase 1  G (lower 16x16 tiles) in passes of four tile columns: the k-chunks of A stream through
//            LDS once per pass (double-buffered, register-prefetched), <= 8 accumulator tiles per wave
//   phase 3  left-looking Cholesky by 16-column panels: panel tile (rt, j) = G(rt, j) - L(rt, :16j) L(j, :16j)^T
//            with both operands read straight from the workspace in MFMA layout (column-major storage makes a
//            lane group's 16 rows one 128-byte segment), then the 16x16 diagonal factorisation / inversion in
//            registers and the panel solve by MFMA exactly as in the LDS kernel; the finished panel goes back
//            to the workspace
//   phase 4  column-oriented substitutions, one wave per right-hand side, the next column prefetched
//   phase 5  W_out^T = A^T alpha (wide) -- the LDS kernel's pass over A
// Same pivot rule (v <= 1e-14 max diag: direction dropped, group flagged) and the same arithmetic order per
// tile as the LDS kernel, so the two agree to round-off where both apply.
// ---------------------------------------------------------------------------------
namespace esn {

constexpr int CB_NMAX = 512;      // largest Gram dimension
constexpr int CB_KC = 8;          // k-chunk staged per pass
constexpr int CB_PLD = 17;        // LDS row stride of the panel (doubles)
constexpr int CB_NT = 512;        // threads: 8 waves, two per SIMD -> 256 registers per lane (16 accumulator tiles)
constexpr int CB_NW = CB_NT / 64;
constexpr int CB_EPT = CB_NMAX * CB_KC / CB_NT;     // staged elements per thread
constexpr int CB_TPW = 16;        // Gram tiles per wave and pass: ceil((32 + 31 + 30 + 29) / 8)

size_t chol_big_work_doubles(int n) {
    const size_t np = (size_t)round_up(n, 16);
    return np * np;
}

template <bool RG>
__global__ __launch_bounds__(CB_NT) void readout_chol_big_kernel(SolveParams sp) {
    extern __shared__ __attribute__((aligned(16))) char cb_smem[];
    typedef double f64x4 __attribute__((ext_vector_type(4)));
    __shared__ int sh_bad;
    __shared__ double sh_invd[CB_NMAX];
    __shared__ double sh_linv[16][17];
    __shared__ double sh_red[CB_NW];
    const int slot = blockIdx.x, tid = threadIdx.x;                     // RG: one workgroup per (group, lambda)
    const int g = RG ? slot / sp.n_ridge : slot;
    if constexpr (RG) {
        if (ridge_rejects(sp, slot)) return;
    }
    const int lane = tid & 63, wv = tid >> 6;
    const int wvu = __builtin_amdgcn_readfirstlane(wv);
    const int rows = sp.T - sp.transient, cols = sp.cols, nrhs = sp.n_out;
    const bool wide = rows < cols;
    const int n = wide ? rows : cols;      // Gram dimension
    const int m = wide ? cols : rows;      // contraction length
    const int np = round_up(n, 16), ntile = np / 16;
    const int ld = np;
    double* Gw = sp.work + (size_t)slot * sp.work_stride;                  // [np][np] column-major, lower part
    const size_t a_off = ((size_t)g * sp.T + sp.transient) * cols;
    const double* A = sp.E ? sp.E + a_off : nullptr;
    const float* A32 = sp.E32 ? sp.E32 + a_off : nullptr;
    const double* Dg = sp.D + ((size_t)g * sp.T + sp.transient) * nrhs;
    const int lr = lane & 15, lq = lane >> 4;
    if (tid == 0) sh_bad = 0;

    // ---- phase 1: Gram ----------------------------------------------------------------------------
    {
        const int AS_LD = np + 4;
        double* Abuf[2] = {reinterpret_cast<double*>(cb_smem), reinterpret_cast<double*>(cb_smem) + (size_t)CB_KC * AS_LD};
        const int ept = (np * CB_KC + CB_NT - 1) / CB_NT;             // staged elements per thread (<= CB_EPT)
        double stg[CB_EPT];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int q = 0; q < CB_EPT; ++q) {
                const int e = tid + CB_NT * q;
                int kk, i;
                if (wide) { i = e / CB_KC; kk = e % CB_KC; } else { kk = e / np; i = e % np; }
                const int k = k0 + kk;
                const size_t ai_ = wide ? (size_t)i * cols + k : (size_t)k * cols + i;
                stg[q] = (q < ept && e < np * CB_KC && i < n && k < m) ? (A32 ? (double)A32[ai_] : A[ai_]) : 0.0;
            }
        };
        auto commit = [&](double* dst) {
#pragma unroll
            for (int q = 0; q < CB_EPT; ++q) {
                const int e = tid + CB_NT * q;
                if (q < ept && e < np * CB_KC) {
                    int kk, i;
                    if (wide) { i = e / CB_KC; kk = e % CB_KC; } else { kk = e / np; i = e % np; }
                    dst[kk * AS_LD + i] = stg[q];
                }
            }
        };
        const int fr_off = lq * AS_LD + lr;
        const int n_pass = (ntile + 3) / 4;
        for (int jb = 0; jb < n_pass; ++jb) {
            // lower tiles of tile columns [4 jb, 4 jb + 4): t-th of them -> (ti, tj); wave w takes t = w, w + CB_NW, ...
            const int tj0 = 4 * jb, tj1 = (tj0 + 4 < ntile) ? tj0 + 4 : ntile;
            int cnt = 0;
            for (int tj = tj0; tj < tj1; ++tj) cnt += ntile - tj;
            int my_ti[CB_TPW], my_tj[CB_TPW];
#pragma unroll
            for (int q = 0; q < CB_TPW; ++q) {
                int t = wvu + CB_NW * q, tj = tj0;
                bool ok = t < cnt;
                while (ok && t >= ntile - tj) { t -= ntile - tj; ++tj; }
                my_tj[q] = ok ? tj : -1;
                my_ti[q] = ok ? tj + t : 0;
            }
            f64x4 acc[CB_TPW];
#pragma unroll
            for (int q = 0; q < CB_TPW; ++q) acc[q] = f64x4{0.0, 0.0, 0.0, 0.0};
            fetch(0);
            commit(Abuf[0]);
            __syncthreads();
            int cur = 0;
            for (int k0 = 0; k0 < m; k0 += CB_KC) {
                const bool more = k0 + CB_KC < m;
                if (more) fetch(k0 + CB_KC);
                const double* Ac = Abuf[cur];
#pragma unroll
                for (int k4 = 0; k4 < CB_KC; k4 += 4) {
                    const double* slab = Ac + k4 * AS_LD + fr_off;
#pragma unroll
                    for (int q = 0; q < CB_TPW; ++q)
                        if (my_tj[q] >= 0)
                            acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(slab[my_ti[q] * 16], slab[my_tj[q] * 16], acc[q], 0, 0, 0);
                }
                if (more) commit(Abuf[cur ^ 1]);
                __syncthreads();
                cur ^= 1;
            }
#pragma unroll
            for (int q = 0; q < CB_TPW; ++q)
                if (my_tj[q] >= 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        Gw[(size_t)(my_tj[q] * 16 + lr) * ld + my_ti[q] * 16 + 4 * i + lq] = acc[q][i];
                }
            __syncthreads();
        }
        // right-hand sides into LDS: Bs[o][np]
        double* Bs = reinterpret_cast<double*>(cb_smem);
        __syncthreads();
        for (int e = tid; e < nrhs * np; e += CB_NT) {
            const int o = e / np, i = e % np;
            double v = 0.0;
            if (wide && i < n) {
                const double sc = sp.t_scale ? sp.t_scale[(size_t)g * nrhs + o] : 1.0;
                const double sh = sp.t_shift ? sp.t_shift[(size_t)g * nrhs + o] : 0.0;
                v = Dg[(size_t)i * nrhs + o] * sc + sh;
            }
            if (wide) Bs[e] = v;
        }
        if (!wide) {
            // tall case: right-hand side A^T B, thread -> (o, i), one pass over A (consecutive lanes = consecutive columns)
            for (int e = tid; e < nrhs * np; e += CB_NT) {
                const int o = e / np, i = e % np;
                double acc_b = 0.0;
                if (i < n) {
                    const double sc = sp.t_scale ? sp.t_scale[(size_t)g * nrhs + o] : 1.0;
                    const double sh = sp.t_shift ? sp.t_shift[(size_t)g * nrhs + o] : 0.0;
#pragma unroll 8
                    for (int k = 0; k < m; ++k) {
                        const double a = A32 ? (double)A32[(size_t)k * cols + i] : A[(size_t)k * cols + i];
                        acc_b = fma(a, Dg[(size_t)k * nrhs + o] * sc + sh, acc_b);
                    }
                }
                Bs[e] = acc_b;
            }
        }
        if constexpr (RG) {
            // ridge: lambda on the live diagonal only (rows >= n of the last tile are padding), before dmax / piv_tol
            const double lam = sp.ridge[slot];
            for (int i = tid; i < n; i += CB_NT) Gw[(size_t)i * ld + i] += lam;
        }
    }
    __threadfence_block();
    __syncthreads();
    double* Bs = reinterpret_cast<double*>(cb_smem);                    // [nrhs][np]          (32 KB)
    double* P = Bs + (size_t)8 * CB_NMAX;                                // [np][CB_PLD] panel  (68 KB)
    // pivot tolerance from the largest diagonal entry
    double dmax = 0.0;
    for (int i = tid; i < n; i += CB_NT) dmax = fmax(dmax, Gw[(size_t)i * ld + i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dmax = fmax(dmax, __shfl_down(dmax, off));
    if (lane == 0) sh_red[wv] = dmax;
    __syncthreads();
    double piv_tol = 0.0;
    for (int w = 0; w < CB_NW; ++w) piv_tol = fmax(piv_tol, sh_red[w]);
    piv_tol *= 1e-14;

    // ---- phase 3: left-looking panel Cholesky ---------------------------------------------------------
    for (int j = 0; j < ntile; ++j) {
        const int j0 = 16 * j;
        // (1) panel tiles: G(rt, j) - L(rt, :j0) L(j, :j0)^T
        for (int rt = j + wvu; rt < ntile; rt += CB_NW) {
            f64x4 c;
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = Gw[(size_t)(j0 + lr) * ld + rt * 16 + 4 * i + lq];
            const double* la = Gw + (size_t)lq * ld + rt * 16 + lr;       // L[rt*16 + lr][k + lq]
            const double* lb = Gw + (size_t)lq * ld + j0 + lr;            // L[j0 + lr][k + lq]
#pragma unroll 4
            for (int k = 0; k < j0; k += 4)
                c = __builtin_amdgcn_mfma_f64_16x16x4f64(-la[(size_t)k * ld], lb[(size_t)k * ld], c, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) P[(rt * 16 + 4 * i + lq) * CB_PLD + lr] = c[i];
        }
        __syncthreads();
        // (2) diagonal block: factorise and invert in registers (wave 0), as in the LDS kernel
        if (wv == 0) {
            const int r = lane & 15;
            double a[16], x[16], my_invd;
#pragma unroll
            for (int c = 0; c < 16; ++c) a[c] = P[(j0 + r) * CB_PLD + c];
            const unsigned rejected = ch_diag_regs<false, true>(a, x, my_invd, j0, n, piv_tol, r);
            if (lane < 16) {
#pragma unroll
                for (int c = 0; c < 16; ++c) P[(j0 + r) * CB_PLD + c] = a[c];
                sh_invd[j0 + r] = my_invd;
            }
            if (rejected && lane == 0) sh_bad = 1;
            if (lane < 16) {
#pragma unroll
                for (int i = 0; i < 16; ++i) sh_linv[i][r] = x[i];
            }
        }
        __syncthreads();
        // (3) panel solve: L(rt, j) = P(rt) L11^-T
        for (int rt = j + 1 + wvu; rt < ntile; rt += CB_NW) {
            f64x4 c = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k0 = 0; k0 < 16; k0 += 4)
                c = __builtin_amdgcn_mfma_f64_16x16x4f64(P[(rt * 16 + lr) * CB_PLD + k0 + lq], sh_linv[lr][k0 + lq], c, 0, 0, 0);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int i = 0; i < 4; ++i) P[(rt * 16 + 4 * i + lq) * CB_PLD + lr] = c[i];
        }
        __syncthreads();
        // (4) the finished panel (rows j0 .. np-1, 16 columns) back to the workspace, column-major
        for (int e = tid; e < (np - j0) * 16; e += CB_NT) {
            const int c = e / (np - j0), rr = j0 + e % (np - j0);
            Gw[(size_t)(j0 + c) * ld + rr] = P[rr * CB_PLD + c];
        }
        __threadfence_block();
        __syncthreads();
    }

    // ---- phase 4: L L^T x = b, one wave per right-hand side; lane holds rows lane + 64 s ---------------
    if (wv < nrhs) {
        double* xb = Bs + (size_t)wv * np;
        constexpr int NS = CB_NMAX / 64;
        const int ns = (np + 63) / 64;
        double b[NS], l[NS], lnext[NS];
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2) b[s2] = (s2 < ns && lane + 64 * s2 < np) ? xb[lane + 64 * s2] : 0.0;
        auto load_col = [&](double (&dst)[NS], int jc) {
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2) {
                const int i = lane + 64 * s2;
                dst[s2] = (s2 < ns && jc >= 0 && jc < n && i < n) ? Gw[(size_t)jc * ld + i] : 0.0;
            }
        };
        auto pick = [&](const double (&v)[NS], int jc) -> double {        // element jc of the distributed vector
            double own = 0.0;
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2) own = ((jc >> 6) == s2) ? v[s2] : own;
            return __shfl(own, jc & 63);
        };
        load_col(l, 0);
        for (int jc = 0; jc < n; ++jc) {                                   // forward: L z = b
            load_col(lnext, jc + 1);
            const double zj = pick(b, jc) * sh_invd[jc];
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2) {
                const int i = lane + 64 * s2;
                b[s2] = (i == jc) ? zj : ((i > jc) ? fma(-l[s2], zj, b[s2]) : b[s2]);
            }
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2) l[s2] = lnext[s2];
        }
        load_col(l, n - 1);
        for (int jc = n - 1; jc >= 0; --jc) {                              // backward: L^T x = z
            load_col(lnext, jc - 1);
            double part = 0.0;
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2) {
                const int i = lane + 64 * s2;
                part = (i > jc && i < n) ? fma(l[s2], b[s2], part) : part;
            }
            part = wave_sum(part);
            const double xj = (pick(b, jc) - part) * sh_invd[jc];
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2) b[s2] = (lane + 64 * s2 == jc) ? xj : b[s2];
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2) l[s2] = lnext[s2];
        }
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2)
            if (s2 < ns && lane + 64 * s2 < np) xb[lane + 64 * s2] = b[s2];
    }
    __syncthreads();

    // ---- phase 5: W_out ----------------------------------------------------------------------------------
    if (wide) {
        // W_out[o][c] = sum_i A[i][c] alpha[i][o]: every element of A fetched once by 16-byte loads; thread
        // (part, unit) sums a share of the rows for the unit's 2 (float64) or 4 (float32) columns and all
        // right-hand sides, the partial sums meet in LDS
        double* part = P;                                                // [parts][8][cols] behind Bs
        if (sp.part_ok) {
            const int cpt = A32 ? 4 : 2, nunit = cols / cpt;
            int parts = CB_NT / nunit;
            if (parts > 3) parts = 3;
            const int pt = tid / nunit, un = tid - pt * nunit;
            if (pt < parts) {
                const int per = (n + parts - 1) / parts;
                const int i0 = pt * per, i1 = (i0 + per < n) ? i0 + per : n;
                double w[4][8];
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int o = 0; o < 8; ++o) w[c][o] = 0.0;
                const size_t ac = (size_t)cpt * un;
#pragma unroll 4
                for (int i = i0; i < i1; ++i) {
                    double a[4];
                    if (A32) {
                        const float4 af = *reinterpret_cast<const float4*>(A32 + ac + (size_t)i * cols);
                        a[0] = (double)af.x; a[1] = (double)af.y; a[2] = (double)af.z; a[3] = (double)af.w;
                    } else {
                        const double2 ad = *reinterpret_cast<const double2*>(A + ac + (size_t)i * cols);
                        a[0] = ad.x; a[1] = ad.y; a[2] = 0.0; a[3] = 0.0;
                    }
#pragma unroll
                    for (int o = 0; o < 8; ++o)
                        if (o < nrhs) {
                            const double al = Bs[o * np + i];
#pragma unroll
                            for (int c = 0; c < 4; ++c)
                                if (c < cpt) w[c][o] = fma(a[c], al, w[c][o]);
                        }
                }
#pragma unroll
                for (int o = 0; o < 8; ++o)
                    if (o < nrhs) {
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (c < cpt) part[(pt * 8 + o) * cols + cpt * un + c] = w[c][o];
                    }
            }
            __syncthreads();
            for (int e = tid; e < nrhs * cols; e += CB_NT) {
                const int o = e / cols, c = e - o * cols;
                double v = part[o * cols + c];
                for (int q = 1; q < parts; ++q) v += part[(q * 8 + o) * cols + c];
                sp.W_out[((size_t)slot * nrhs + o) * cols + c] = v;
            }
        } else {
            for (int c = tid; c < cols; c += CB_NT) {
                double w[8];
#pragma unroll
                for (int o = 0; o < 8; ++o) w[o] = 0.0;
                for (int i = 0; i < n; ++i) {
                    const double a = A32 ? (double)A32[(size_t)i * cols + c] : A[(size_t)i * cols + c];
#pragma unroll
                    for (int o = 0; o < 8; ++o)
                        if (o < nrhs) w[o] = fma(a, Bs[o * np + i], w[o]);
                }
#pragma unroll
                for (int o = 0; o < 8; ++o)
                    if (o < nrhs) sp.W_out[((size_t)slot * nrhs + o) * cols + c] = w[o];
            }
        }
    } else {
        for (int e = tid; e < nrhs * cols; e += CB_NT) {
            const int o = e / cols, c = e % cols;
            sp.W_out[((size_t)slot * nrhs + o) * cols + c] = Bs[o * np + c];
        }
    }
    if (tid == 0) sp.status[slot] = sh_bad;
}

static int chol_big_parts(int cols, bool f32) {          // 0 = the partial-sums pass does not apply
    const int cpt = f32 ? 4 : 2;
    if (cols % cpt) return 0;
    const int nunit = cols / cpt;
    if (nunit > CB_NT) return 0;
    const int parts = CB_NT / nunit > 3 ? 3 : CB_NT / nunit;
    return ((size_t)8 * CB_NMAX * 8 + (size_t)parts * 8 * cols * 8 <= 140 * 1024) ? parts : 0;
}
static size_t chol_big_lds_bytes(int cols, bool f32) {
    const size_t gram = 2 * (size_t)CB_KC * (CB_NMAX + 4) * 8;
    size_t tail = (size_t)CB_NMAX * CB_PLD * 8;
    const size_t pp = (size_t)chol_big_parts(cols, f32) * 8 * cols * 8;
    if (pp > tail) tail = pp;
    tail += (size_t)8 * CB_NMAX * 8;
    return gram > tail ? gram : tail;
}

int launch_readout_chol_big(const double* E, const float* E32, const double* D, int n_groups, int T, int transient,
                            int cols, int n_out, const double* t_scale, const double* t_shift,
                            double* W_out, int* status, void* workspace, hipStream_t stream,
                            const double* ridge, int n_ridge) {
    SolveParams sp;
    sp.ridge = ridge; sp.n_ridge = n_ridge;
    const int rows = T - transient;
    const int n = rows < cols ? rows : cols;
    if (n > CB_NMAX || n_out > 8) return -1;
    const size_t lds = chol_big_lds_bytes(cols, E32 != nullptr);
    sp.part_ok = chol_big_parts(cols, E32 != nullptr) > 0 ? 1 : 0;
    sp.E = E; sp.E32 = E32; sp.D = D; sp.n_groups = n_groups; sp.T = T; sp.transient = transient;
    sp.cols = cols; sp.n_out = n_out; sp.t_scale = t_scale; sp.t_shift = t_shift;
    sp.W_out = W_out; sp.status = status;
    sp.work = reinterpret_cast<double*>(workspace); sp.work_stride = chol_big_work_doubles(n);
    sp.wide = rows < cols; sp.m = sp.wide ? cols : rows; sp.n = n; sp.skip = 0;
    void (*fn)(SolveParams) = ridge ? readout_chol_big_kernel<true> : readout_chol_big_kernel<false>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fn, dim3(ridge ? n_groups * n_ridge : n_groups), dim3(CB_NT), lds, stream, sp);
    return (int)hipGetLastError();
}

}  // namespace esn
