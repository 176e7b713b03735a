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
#include "esn_solve.h"

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

// What the phases of one workgroup share.  Gs: the 36 packed tiles (phases 2-4; the E staging, both DMA rings and the
// W_out part sums alias them); Bs: [CH_NP][CH_RHS] right-hand sides / solution.
template <typename TE>
struct ChCtx {
    int slot, g, tid, lane, wv, lr, lq;
    int n, m, ntile, cols, nrhs;            // Gram dimension (<= CH_NP), contraction length, ceil(n / 16)
    const TE* A;                            // [rows][cols] of group g, behind the transient
    const double* Dg;
    double* Gs; double* Bs;
    // cycle sums of the diagnostic build.  st_acc: Gram wait | barrier | operand read | MFMA issue, W_out wait |
    // barrier | rows; st_ph: panel + trailing update | the two barrier waits | the diagonal tile (wave 0)
    // (mutable: the phases take the context const, which holds for everything they compute with; the diagnostic build
    // alone writes these sums through it)
    ESN_STAMPS_ONLY(mutable unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_ph[4] = {0, 0, 0, 0};)
};

// Phase 1 state: tile t of the 36 lower tiles goes to wave t % 8, so waves w and w + 4 (one SIMD) carry 9 between
// them; the tall case also needs A^T B: thread (o, i) = (e / 128, e % 128), e = tid + 512 p.
struct ChGram {
    int ti[5], tj[5], cnt;
    f64x4 acc[5];
    double atb[2];
};
__device__ __forceinline__ void ch_gram_init(ChGram& gr, int wv) {
    gr.cnt = wv < 4 ? 5 : 4;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int t = wv + CH_NW * q < CH_TILES ? wv + CH_NW * q : 0;
        int ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
        gr.ti[q] = ti;
        gr.tj[q] = t - ti * (ti + 1) / 2;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) gr.acc[q] = f64x4{0.0, 0.0, 0.0, 0.0};
    gr.atb[0] = gr.atb[1] = 0.0;
}

// ---- phase 1: G = sum_k a_k a_k^T on the float64 matrix pipe ------------------------------
// v_mfma_f64_16x16x4_f64 (A[l%16][l/16], B[l/16][l%16], C reg i: row 4i + l/16, col l%16) runs at
// the vector-FMA rate on gfx950 (64 cycles, probe in tools/mfma_layout_probe.hip).  Only the 36 lower
// 16x16 tiles are formed.
//
// By DMA ring (wide float32 E, sp.dma): float32 chunks of 32 k x 128 rows through a ring of CH_RING buffers,
// CH_RING - 1 in flight.  DMA piece j of wave w covers rows 8 d .. 8 d + 7 (d = 2 w + j) and all eight k-quads of the
// chunk: lane l fetches the 16 B of row 8 d + (l & 7), k-quad l >> 3.  Byte (r, k) of a buffer is therefore
// 1024 (r >> 3) + 128 (k >> 2) + 16 (r & 7) + 4 (k & 3): an operand read (16 rows x 4 k) takes two LDS
// cycles per lane group, the least a 4-byte read of 16-byte runs allows, and steps k4 apart by a
// constant offset.  Rows >= n are past num_records, k-quads >= m get an out-of-range offset: both land
// as zeros.  The MFMA sequence and k order are those of the register-staged pass (bitwise the same G).
template <typename TE>
__device__ __forceinline__ void ch_gram_ring(const ChCtx<TE>& cx, ChGram& gr, int m_run) {
    const int lane = cx.lane, wv = cx.wv, m = cx.m, cols = cx.cols;
    char* ring = reinterpret_cast<char*>(cx.Gs);
    const __amdgpu_buffer_rsrc_t ers = ch_rsrc(cx.A, cx.n * cols * 4);
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
    const int lbase = 1024 * (cx.lr >> 3) + 16 * (cx.lr & 7) + 4 * cx.lq;
    for (int c = 0, b = 0; c < nch; ++c, b = (b + 1 == CH_RING ? 0 : b + 1)) {
        ESN_STAMP(s0);
        const int later = nch - 1 - c < CH_RING - 2 ? nch - 1 - c : CH_RING - 2;
        ch_wait_dma(2 * later);
        ESN_STAMP(s1);
        __builtin_amdgcn_s_barrier();                       // chunk c landed for all; chunk c-1 read by all
        if (c + CH_RING - 1 < nch) issue(c + CH_RING - 1, b == 0 ? CH_RING - 1 : b - 1);
        const char* buf = ring + b * CH_RBUF + lbase;
        const float* pa[5];
        const float* pb[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            pa[q] = reinterpret_cast<const float*>(buf + 2048 * gr.ti[q]);
            pb[q] = reinterpret_cast<const float*>(buf + 2048 * gr.tj[q]);
        }
        ESN_STAMP(s2);
        // operand-read latency: one read of the chunk, waited for (the stamp waits lgkmcnt(0))
        ESN_STAMPS_ONLY({ float x = pa[0][0]; asm volatile("" :: "v"(x)); })
        ESN_STAMP(s3);
        // the tile count is hoisted out of the k4 steps: a full chunk is one straight block, so its
        // operand reads run ahead of the MFMAs across steps
        auto step = [&](int s, auto cnt) {
#pragma unroll
            for (int q = 0; q < decltype(cnt)::value; ++q)
                gr.acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)pa[q][32 * s], (double)pb[q][32 * s], gr.acc[q], 0, 0, 0);
        };
        const int kmax = (m - c * CH_KC < CH_KC) ? m - c * CH_KC : CH_KC;
        if (kmax == CH_KC && gr.cnt == 5) {
#pragma unroll
            for (int s = 0; s < CH_KC / 4; ++s) step(s, std::integral_constant<int, 5>());
        } else if (kmax == CH_KC) {
#pragma unroll
            for (int s = 0; s < CH_KC / 4; ++s) step(s, std::integral_constant<int, 4>());
        } else if (gr.cnt == 5) {
            for (int s = 0; s < kmax / 4; ++s) step(s, std::integral_constant<int, 5>());
        } else {
            for (int s = 0; s < kmax / 4; ++s) step(s, std::integral_constant<int, 4>());
        }
        ESN_STAMP(s4);
        ESN_STAMPS_ONLY(cx.st_acc[0] += s1 - s0; cx.st_acc[1] += s2 - s1; cx.st_acc[2] += s3 - s2;
                        cx.st_acc[3] += s4 - s3;)
    }
    __syncthreads();                                        // every DMA waited for; the ring is read out
}

// By register staging (every other instance and shape): chunk c is multiplied out of Abuf[c & 1] while chunk c+1 is
// in flight to registers (with two workgroups per CU, the partner's work covers what one chunk of MFMAs does not).
// A chunk is 32 k x 128 i; each thread moves two runs of 4 elements that are contiguous in E (16-byte
// loads when sp.vec): 4 consecutive k of one Gram row (wide) or 4 consecutive Gram rows of one k (tall).
// Wide: a 16-lane group takes 16 rows, so the 8-byte LDS stores of a group hit 32 distinct banks.
template <typename TE, bool wide>
__device__ __forceinline__ void ch_gram_staged(const SolveParams& sp, const ChCtx<TE>& cx, ChGram& gr, int m_run,
                                               double* const (&Abuf)[2]) {
    const int tid = cx.tid, n = cx.n, m = cx.m, cols = cx.cols, nrhs = cx.nrhs, g = cx.g;
    const TE* A = cx.A;
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
    for (int k0 = 0, cur = 0; k0 < m_run; k0 += CH_KC, cur ^= 1) {
        if (k0 == 0) {
            fetch(0);
            commit(Abuf[0]);
            __syncthreads();
        }
        ESN_STAMP(s0);
        if (k0 + CH_KC < m_run) fetch(k0 + CH_KC);
        const double* Ac = Abuf[cur];
        const int kmax = (m - k0 < CH_KC) ? m - k0 : CH_KC;
        // (rows past m and columns past n of the chunk are zero-filled by fetch)
        const double* slab0 = Ac + cx.lq * CH_AS_LD + cx.lr;
        for (int k4 = 0; k4 < kmax; k4 += 4) {
            const double* slab = slab0 + k4 * CH_AS_LD;
#pragma unroll
            for (int q = 0; q < 5; ++q)
                if (q < gr.cnt)
                    gr.acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(slab[gr.ti[q] * 16], slab[gr.tj[q] * 16], gr.acc[q], 0, 0, 0);
        }
        if constexpr (!wide) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int e = tid + CH_NT * p, o = e / CH_NP, i = e % CH_NP;
                if (o < nrhs) {
                    const double sc = sp.t_scale ? sp.t_scale[(size_t)g * nrhs + o] : 1.0;
                    const double sh = sp.t_shift ? sp.t_shift[(size_t)g * nrhs + o] : 0.0;
                    for (int kk = 0; kk < kmax; ++kk)
                        gr.atb[p] = fma(Ac[kk * CH_AS_LD + i], cx.Dg[(size_t)(k0 + kk) * nrhs + o] * sc + sh, gr.atb[p]);
                }
            }
        }
        ESN_STAMP(s1);
        if (k0 + CH_KC < m_run) commit(Abuf[cur ^ 1]);
        ESN_STAMP(s2);
        __syncthreads();
        ESN_STAMP(s3);
        // MFMA issue | load wait + commit | barrier
        ESN_STAMPS_ONLY(cx.st_acc[3] += s1 - s0; cx.st_acc[0] += s2 - s1; cx.st_acc[1] += s3 - s2;)
    }
}

// ---- phase 2: G and the right-hand sides into LDS ----------------------------------------
// Ridge: lambda on the live diagonal only (the padding rows of a ragged last tile stay as they are), before
// dmax / piv_tol are taken; + 0.0 leaves a non-negative diagonal bitwise as it is.
template <typename TE, bool wide, bool RG>
__device__ __forceinline__ void ch_gram_to_lds(const SolveParams& sp, const ChCtx<TE>& cx, const ChGram& gr) {
    const int tid = cx.tid, n = cx.n, nrhs = cx.nrhs, g = cx.g;
    double* Gs = cx.Gs;
#pragma unroll
    for (int q = 0; q < 5; ++q)
        if (q < gr.cnt) {
            double* T = Gs + ch_tile(gr.ti[q], gr.tj[q]);
#pragma unroll
            for (int i = 0; i < 4; ++i) T[ch_el(4 * i + cx.lq, cx.lr)] = gr.acc[q][i];
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
                v = cx.Dg[(size_t)i * nrhs + o] * sc + sh;
            }
            cx.Bs[e] = v;
        } else {
            const int o = e / CH_NP, i = e % CH_NP;
            cx.Bs[i * CH_RHS + o] = (o < nrhs && i < n) ? gr.atb[p] : 0.0;
        }
    }
    __syncthreads();
    if constexpr (RG) {
        const double lam = sp.ridge[cx.slot];
        for (int i = tid; i < n; i += CH_NT) Gs[ch_tile(i >> 4, i >> 4) + ch_el(i & 15, i & 15)] += lam;
        __syncthreads();
    }
}

// ---- phase 3: blocked right-looking Cholesky, 16-column blocks ----------------------------
// per block kb: (b) panel L21 = A21 L11^-T, one tile per wave; (c) trailing update A22 -= L21 L21^T of
// the lower tiles, where wave 0 takes the next diagonal tile and goes on to factorise and invert it (a)
// while waves 1-7 update the rest.  Two barriers per 16 columns; all products are 16x16x4 float64
// MFMAs out of / into the packed tiles.  Returns (wave 0) whether a live pivot was rejected.
template <typename TE>
__device__ __forceinline__ int ch_factor(const SolveParams& sp, const ChCtx<TE>& cx) {
    const int lane = cx.lane, wv = cx.wv, lr = cx.lr, lq = cx.lq, n = cx.n, ntile = cx.ntile;
    double* Gs = cx.Gs;
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
        ESN_STAMP(f0);
        ESN_STAMPS_ONLY(unsigned long long f1 = f0, f2 = f0;)
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
            ESN_STAMP_SET(f1);
            __syncthreads();
            ESN_STAMP_SET(f2);
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
        ESN_STAMP(f3);
        if (wv == 0 && kb + 1 < nblk) bad |= ch_factor_diag(Gs + ch_tile(kb + 1, kb + 1), 16 * (kb + 1), n, piv_tol, lane);
        ESN_STAMP(f4);
        __syncthreads();
        ESN_STAMP(f5);
        ESN_STAMPS_ONLY(cx.st_ph[0] += (f1 - f0) + (f3 - f2); cx.st_ph[1] += (f2 - f1) + (f5 - f4);
                        cx.st_ph[2] += f4 - f3;)
    }
    return bad;
}

// ---- phase 4: L L^T alpha = B by 16-row tiles ---------------------------------------------
// Forward, step I: z_I = L_II^-1 b_I, then b_J -= L_JI z_I for J > I (wave J - I - 1).  Backward, step I:
// x_I = L_II^-T z_I, then z_J -= L_IJ^T x_I for J < I (wave J).  Each product is four 16x16x4 MFMAs
// (columns = right-hand sides, lanes with lr >= 8 carry zeros); the accumulator layout of z_I is the B
// operand layout of the update, so every updating wave forms z_I itself.  Wave 7 forms it as well and
// stores it one step later, when no wave reads those rows any more.  One barrier per tile step.
template <typename TE>
__device__ __forceinline__ void ch_substitute(const ChCtx<TE>& cx) {
    const int wv = cx.wv, lr = cx.lr, lq = cx.lq, ntile = cx.ntile;
    double* Gs = cx.Gs;
    double* Bs = cx.Bs;
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

// ---- phase 5: W_out ---------------------------------------------------------------------
// one row of E into a thread's sums: w[c][o] = fma(a[c], al[o], w[c][o]) for the live outputs
template <typename TA, int CPT>
__device__ __forceinline__ void ch_wacc(double (&w)[CPT][CH_RHS], const TA (&a)[CPT], const double* al, int nrhs) {
#pragma unroll
    for (int o = 0; o < CH_RHS; ++o)
        if (o < nrhs) {
            const double x = al[o];
#pragma unroll
            for (int c = 0; c < CPT; ++c) w[c][o] = fma((double)a[c], x, w[c][o]);
        }
}
// the sums of part pt >= 1 for its unit's columns into part[pt - 1][o][cols]
template <int CPT>
__device__ __forceinline__ void ch_put_part(double* part, const double (&w)[CPT][CH_RHS], int pt, int un, int cols,
                                            int nrhs) {
#pragma unroll
    for (int o = 0; o < CH_RHS; ++o)
        if (o < nrhs) {
#pragma unroll
            for (int c = 0; c < CPT; ++c) part[((pt - 1) * CH_RHS + o) * cols + CPT * un + c] = w[c][o];
        }
}

// Wide: W_out[o][c] = sum_i A[i][c] alpha[i][o].  Every element of A is fetched once, by 16-byte loads:
// thread (part, unit) sums a third of the rows for the unit's CPT columns and all nrhs outputs;
// parts 1 and 2 leave their sums in LDS (the factor is no longer needed), part 0 adds them.
// dma: the same sums, E streamed through a ring of CH_WRING buffers: chunk c holds rows
// i0 + rw c .. i0 + rw c + rw - 1 of each part in that part's CH_WSEG segment (row-major as in E),
// so each thread reads its 16 B of a row with one conflict-free LDS read.  Wave w fetches 1 KB piece
// w of every segment; bytes past a segment's rows get an out-of-range offset and land as zeros.
// Row order per thread and the combine order of the parts are unchanged (bitwise the same W_out).
// Columns that are no whole number of 16-byte runs, or part sums that do not fit the tile area: one column per thread.
template <typename TE>
__device__ __forceinline__ void ch_wout_wide(const SolveParams& sp, const ChCtx<TE>& cx, bool dma) {
    const int tid = cx.tid, n = cx.n, cols = cx.cols, nrhs = cx.nrhs;
    const TE* A = cx.A;
    const double* Bs = cx.Bs;
    constexpr int CPT = 16 / sizeof(TE);
    const int nunit = cols / CPT;
    int parts = nunit > 0 ? CH_NT / nunit : 0;
    parts = parts > 3 ? 3 : parts;
    if (sp.vec && cols % CPT == 0 && parts > 0 && (parts - 1) * CH_RHS * cols <= CH_TILES * 256 && !(sp.skip & 8)) {
        double* part = cx.Gs;                            // [parts - 1][CH_RHS][cols]
        const int pt = tid / nunit, un = tid - pt * nunit;
        double w[CPT][CH_RHS];
#pragma unroll
        for (int c = 0; c < CPT; ++c)
#pragma unroll
            for (int o = 0; o < CH_RHS; ++o) w[c][o] = 0.0;
        const int per = (n + parts - 1) / parts;
        const int i0 = pt * per, i1 = (i0 + per < n) ? i0 + per : n;
        int rw = CH_WSEG / (cols * 4);                   // rows of each part per W_out chunk
        rw = rw > CH_WROWS ? CH_WROWS : rw;
        bool wdma = false;
        if constexpr (sizeof(TE) == 4) {
          wdma = dma && rw > 0;
          if (wdma) {
            const int lane = cx.lane, wv = cx.wv;
            char* ring = reinterpret_cast<char*>(cx.Gs);
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
            for (int c = 0, b = 0; c < nch; ++c, b = (b + 1 == CH_WRING ? 0 : b + 1)) {
                ESN_STAMP(s0);
                ch_wait_dma(nch - 1 - c < CH_WRING - 2 ? 3 * (nch - 1 - c) : 3 * (CH_WRING - 2));
                ESN_STAMP(s1);
                __builtin_amdgcn_s_barrier();
                if (c + CH_WRING - 1 < nch) issue(c + CH_WRING - 1, b == 0 ? CH_WRING - 1 : b - 1);
                ESN_STAMP(s2);
                if (pt < parts) {
                    const char* seg = ring + (b * 3 + pt) * CH_WSEG + CPT * sizeof(TE) * un;
                    const int ib = i0 + c * rw;
                    const int nr = ((ib + rw < i1) ? ib + rw : i1) - ib;
#pragma unroll
                    for (int rr = 0; rr < CH_WROWS; ++rr) {
                        if (rr >= nr) break;
                        float a[4];
                        double al[CH_RHS];
                        ch_wrow(seg + rr * rowb, Bs + (ib + rr) * CH_RHS, a, al);
                        ch_wacc(w, a, al, nrhs);
                    }
                }
                ESN_STAMP(s3);
                ESN_STAMPS_ONLY(cx.st_acc[4] += s1 - s0; cx.st_acc[5] += s2 - s1; cx.st_acc[6] += s3 - s2;)
            }
            __syncthreads();                             // the ring is read out: the part sums alias it
          }
        }
        if (!wdma && pt < parts) {
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
                ch_wacc(w, a, Bs + i * CH_RHS, nrhs);
            }
        }
        if (pt > 0 && pt < parts) ch_put_part(part, w, pt, un, cols, nrhs);
        __syncthreads();
        if (pt == 0) {
#pragma unroll
            for (int o = 0; o < CH_RHS; ++o)
                if (o < nrhs) {
#pragma unroll
                    for (int c = 0; c < CPT; ++c) {
                        double v = w[c][o];
                        for (int q = 1; q < parts; ++q) v += part[((q - 1) * CH_RHS + o) * cols + CPT * un + c];
                        sp.W_out[((size_t)cx.slot * nrhs + o) * cols + CPT * un + c] = v;
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
                if (o < nrhs) sp.W_out[((size_t)cx.slot * nrhs + o) * cols + c] = w[o];
        }
    }
}

// Tall: the solution is W_out^T
template <typename TE>
__device__ __forceinline__ void ch_wout_tall(const SolveParams& sp, const ChCtx<TE>& cx) {
    for (int e = cx.tid; e < cx.nrhs * cx.cols; e += CH_NT) {
        const int o = e / cx.cols, c = e % cx.cols;
        sp.W_out[((size_t)cx.slot * cx.nrhs + o) * cx.cols + c] = cx.Bs[c * CH_RHS + o];
    }
}

#ifdef ESN_STAMPS
// row wv: st_acc; row 8 + wv: the four phases between the kernel's stamps k[0..4], their total, st_ph
template <typename TE>
__device__ __forceinline__ void ch_put_stamps(const SolveParams& sp, const ChCtx<TE>& cx,
                                              const unsigned long long (&k)[5]) {
    if (!sp.stamps || cx.slot != 0 || cx.lane != 0) return;
    unsigned long long* row = sp.stamps + cx.wv * 8;
    for (int i = 0; i < 7; ++i) row[i] = cx.st_acc[i];
    row += 8 * 8;
    for (int i = 0; i < 4; ++i) row[i] = k[i + 1] - k[i];
    row[4] = k[4] - k[0];
    for (int i = 0; i < 3; ++i) row[5 + i] = cx.st_ph[i];      // the factor phase, split
}
#endif

template <typename TE, bool wide, bool RG>
__global__ __launch_bounds__(CH_NT) __attribute__((amdgpu_waves_per_eu(4))) void readout_chol_kernel(SolveParams sp) {
    extern __shared__ __attribute__((aligned(16))) char chol_smem[];
    ChCtx<TE> cx;
    cx.slot = blockIdx.x; cx.tid = threadIdx.x;                     // RG: one workgroup per (group, lambda)
    cx.g = RG ? cx.slot / sp.n_ridge : cx.slot;
    if constexpr (RG) {
        if (ridge_rejects(sp, cx.slot)) return;
    }
    cx.lane = cx.tid & 63; cx.wv = __builtin_amdgcn_readfirstlane(cx.tid >> 6);
    cx.lr = cx.lane & 15; cx.lq = cx.lane >> 4;
    const int rows = sp.T - sp.transient;
    cx.cols = sp.cols; cx.nrhs = sp.n_out;
    cx.n = wide ? rows : cx.cols;
    cx.m = wide ? cx.cols : rows;
    cx.ntile = (cx.n + 15) / 16;
    cx.A = ch_src(sp, (TE*)nullptr) + ((size_t)cx.g * sp.T + sp.transient) * cx.cols;
    cx.Dg = sp.D + ((size_t)cx.g * sp.T + sp.transient) * cx.nrhs;
    cx.Gs = reinterpret_cast<double*>(chol_smem);
    cx.Bs = cx.Gs + CH_TILES * 256;
    ChGram gr;
    ch_gram_init(gr, cx.wv);
    const int m_run = (sp.skip & 1) ? CH_KC : cx.m;
    constexpr bool can_dma = wide && sizeof(TE) == 4;
    const bool dma = can_dma && sp.dma && sp.vec;
    ESN_STAMPS_ONLY(unsigned long long st_k[5];)
    ESN_STAMP_SET(st_k[0]);
    if constexpr (can_dma) {
        if (dma) ch_gram_ring(cx, gr, m_run);
    }
    // the two staging buffers of the register-staged pass, [CH_KC][CH_AS_LD] each.  Declared here, not in the phase: as
    // the phase's own local the array is folded away before inlining and <float, tall, ridge> takes 127 VGPRs, not 115
    double* Abuf[2] = {cx.Gs, cx.Gs + CH_KC * CH_AS_LD};
    ch_gram_staged<TE, wide>(sp, cx, gr, dma ? 0 : m_run, Abuf);
    ESN_STAMP_SET(st_k[1]);
    ch_gram_to_lds<TE, wide, RG>(sp, cx, gr);
    const int bad = ch_factor(sp, cx);
    ESN_STAMP_SET(st_k[2]);
    if (!(sp.skip & 4)) ch_substitute(cx);
    ESN_STAMP_SET(st_k[3]);
    if constexpr (wide) ch_wout_wide(sp, cx, dma);
    else ch_wout_tall(sp, cx);
    if (cx.tid == 0) sp.status[cx.slot] = bad;
    ESN_STAMP_SET(st_k[4]);
    ESN_STAMPS_ONLY(ch_put_stamps(sp, cx, st_k);)
}

int launch_readout_chol(const ReadoutArgs& a) {
    SolveParams sp = solve_params(a);
    if (sp.n > CH_NP || a.n_out > CH_RHS) return -1;
    sp.skip = knobs().chol_skip;
    sp.dma = knobs().chol_dma;
    // 16-byte loads of 4 consecutive elements: every row of every group starts 16-byte aligned
    const uintptr_t base = a.E32 ? (uintptr_t)a.E32 : (uintptr_t)a.E;
    sp.vec = (base % 16 == 0) && (a.cols % (a.E32 ? 4 : 2) == 0);
    void (*fn)(SolveParams);
    if (a.ridge)
        fn = a.E32 ? (sp.wide ? readout_chol_kernel<float, true, true> : readout_chol_kernel<float, false, true>)
                   : (sp.wide ? readout_chol_kernel<double, true, true> : readout_chol_kernel<double, false, true>);
    else
        fn = a.E32 ? (sp.wide ? readout_chol_kernel<float, true, false> : readout_chol_kernel<float, false, false>)
                   : (sp.wide ? readout_chol_kernel<double, true, false> : readout_chol_kernel<double, false, false>);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)CH_LDS);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fn, dim3(solve_grid(a)), dim3(CH_NT), CH_LDS, a.stream, sp);
    return (int)hipGetLastError();
}

}  // namespace esn
