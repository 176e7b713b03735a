// fp16 / bf16 predict at 257..512 reservoir units on v_mfma_f32_16x16x32: the skewed schedule of
// esn_recur_mfma_impl.h (two wave sets one third of a step apart, see there) with every image re-cut for
// the 16 x 16 x 32 shape.  Why: the chip lowers its clock under this kernel's load, and holds a 13-17 %
// higher one on the small shape (tools/probes/mfma_shape_probe.hip: the kernel's own slots rebuilt with
// both shapes -- 12 % more cycles, 4-10 % less wall time per slot).  What changes with the shape:
//
//  * State image, fragment-major:  Zf[column tile c of 16 frames][32-k group kk][lane][16 B].  Lane
//    (q = lane >> 4, col = lane & 15) of block (c, kk) holds the eight halves of k-chunk q of frame 16 c + col --
//    exactly the B operand of one MFMA, read by ONE linear, conflict-free ds_read_b128 (address = block + 16 lane).
//  * k order.  The accumulator tile of a 16x16x32 MFMA leaves rows 4 g .. 4 g + 3 (g = lane >> 4) of column
//    lane & 15 in a lane; two row tiles give that lane eight values = one 16-byte chunk of the NEXT step's B
//    operand.  So state row R = 32 kk + 16 t + 4 g + e (t = 0, 1) lives at position 32 kk + 8 g + 4 t + e of
//    its 32-k group (s16_pos below); the weight image (esn_pack.hip) is cut in the same order, and phase E
//    stores 16 bytes per lane and tile pair at block + 16 lane -- linear again, half the stores.
//  * Read-out.  The B fragment of column tile c and group kk IS the operand of the read-out MFMA of that tile
//    (the 32x32x16 kernel reads a second, differently cut view of the rows, with bank conflicts).
//  * [U ; F] group kk = 16 in natural order: inputs at k = 512 + ci, feedback at kfb + o.
// Serves Mp = 512, Kp = 544 (n_in <= 16, n_out <= 8), 8 waves of 64 rows x 128 frames, 128 accumulator
// registers.  Everything else -- slot program, fixed-buffer weight prefetch, OOB loads instead of branches,
// LDS-DMA input staging, packed-half noise tail, the counter noise as a function of (seed, frame, step, row) --
// is the 32x32x16 kernel's, and the two are compared bit-for-bit-tolerance in tests/test_gpu_parity.py.
#pragma once
#include "esn_state_noise.h"

namespace esn {

constexpr int S16_NKK = 17;            // 32-k groups: 16 of state rows + the [U ; F] group
constexpr int S16_NKH = 8;             // state groups per half
constexpr int S16_MP = 512;

// IO32: float32 U / Y (esn_predict_batch_f32); the float64-I/O instances are unchanged by it
template <typename TR, int NOISE, bool IO32 = false>
__global__ __launch_bounds__(512) void recur_skew16_kernel(RecurParams p) {
    extern __shared__ __attribute__((aligned(16))) char zf[];
    constexpr int NW = 8, BT = 128, NOWN = 8, NKK = S16_NKK, NKH = S16_NKH;
    constexpr int NTHREADS = NW * 64;
    constexpr int TILE_B = NKK * 1024;                    // bytes of one column tile's image
    ESN_STAMP(t_entry)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Geometry& g = p.g;
    const int n_res = p.n_res, n_in = p.n_in, n_out = p.n_out;
    const int kin_p = g.kfb - g.kin;
    const int kfb_p = round_up(n_out, 4);
    const int out_rows = p.S - p.transient;

    const int tile = xcd_remap(blockIdx.x, p.n_tiles);
    const int slot0 = tile * BT;
    const int grp0 = slot_group(p, slot0);
    if (grp0 >= p.n_groups) return;
    const int wset = slot_wset(p, slot0);

    // tables behind the state image (as in esn_recur_mfma_impl.h) + the step-independent half of the noise key
    int* tab_fr = reinterpret_cast<int*>(zf + (size_t)NOWN * TILE_B);
    uint32_t* tab_key = reinterpret_cast<uint32_t*>(tab_fr + BT);
    float2* tab_in = reinterpret_cast<float2*>(tab_key + BT);
    float2* tab_un = tab_in + NOWN * kin_p;
    char* in_slots = reinterpret_cast<char*>(tab_un + NOWN * 16);       // [NOWN][2][1 KB] raw input rows (float64 or float32)
    int* tab_off = reinterpret_cast<int*>(in_slots + (size_t)NOWN * 2048);
    // counter noise: the (frame, step) keys of the 128 frames, written once per step by the tile's own wave (sixteen
    // lanes, one mix32) instead of being re-derived by every lane of every wave for each of its eight tiles; two
    // buffers by step parity (set B reads step s while set A already writes step s + 1)
    uint32_t* tab_ks = reinterpret_cast<uint32_t*>(tab_off + BT);
    // group of every slot, for the prologue alone: it borrows the head of the input staging slots, whose first writer is
    // the LDS-DMA of step 1, barriers later.  Every per-slot division of the prologue is done here, once per slot
    int* tab_grp = reinterpret_cast<int*>(in_slots);
    const int lkin = __builtin_ctz(kin_p);                 // kin_p = round4(n_in) is 4, 8 or 16
    for (int i = tid; i < BT; i += NTHREADS) {
        int gtmp;
        const int fr = slot_frame(p, slot0 + i, gtmp);
        tab_fr[i] = fr;
        tab_grp[i] = gtmp;
        tab_key[i] = mix32((uint32_t)p.seed ^ (((uint32_t)fr + p.frame_off) * 0x9E3779B9U));   // noise_key, stage 1
    }
    // ---- LDS init: zeros over the whole state image (state rows and the [U ; F] group of every column tile), linear
    // 16-byte stores; the bench and every detector call without a continuation start from exactly this image
    {
        constexpr int CHUNKS = NOWN * TILE_B / 16;
        static_assert(CHUNKS % NTHREADS == 0, "whole passes");
#pragma unroll
        for (int i = 0; i < CHUNKS / NTHREADS; ++i)
            *reinterpret_cast<u32x4*>(zf + (size_t)(i * NTHREADS + tid) * 16) = u32x4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
    for (int i = tid; i < NOWN * kin_p; i += NTHREADS) {
        const int c16 = i >> lkin, c = i & (kin_p - 1);
        const int cg = tab_grp[c16 * 16];
        float2 v = make_float2(0.f, 0.f);
        if (cg < p.n_groups && c < n_in) {
            v.x = p.in_scale ? (float)p.in_scale[(size_t)cg * n_in + c] : 1.f;
            v.y = p.in_shift ? (float)p.in_shift[(size_t)cg * n_in + c] : 0.f;
        }
        tab_in[i] = v;
    }
    for (int i = tid; i < NOWN * 16; i += NTHREADS) {
        const int c16 = i / 16, o = i % 16;
        const int cg = tab_grp[c16 * 16];
        float2 v = make_float2(1.f, 0.f);
        if (cg < p.n_groups && o < n_out) {
            if (p.t_scale) v.x = (float)(1.0 / p.t_scale[(size_t)cg * n_out + o]);
            if (p.t_shift) v.y = (float)p.t_shift[(size_t)cg * n_out + o];
        }
        tab_un[i] = v;
    }
    // (every lambda of this kernel is S16_INLINE: the step loop below exists once per wave set, and without the
    //  attribute the compiler outlines the lambdas that now have two callers into real functions -- s_swappc, the
    //  accumulators through 1-1.4 KB of scratch)
#define S16_INLINE __attribute__((always_inline))
    // x0 into the state rows: one 16-byte chunk (frame f, group kk, k-chunk q) per trip = the natural rows
    // 32 kk + 16 t + 4 q + e (t = 0, 1; e = 0..3) of s16_pos, rows past n_res and padding frames as zeros
    if (p.x0) {
        for (int i = tid; i < BT * 2 * NKH * 4; i += NTHREADS) {
            const int f = i & (BT - 1), kq = i >> 7, kk = kq >> 2, q = kq & 3;
            const bool live = tab_fr[f] >= 0;
            const double* xr = p.x0 + (size_t)(live ? tab_grp[f] : 0) * n_res;
            uint32_t w[4];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int k = 32 * kk + 16 * t + 4 * q;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (live && k + e < n_res) ? (float)xr[k + e] : 0.f;
                w[2 * t] = TR::pack2(v[0], v[1]);
                w[2 * t + 1] = TR::pack2(v[2], v[3]);
            }
            *reinterpret_cast<u32x4*>(zf + ((size_t)((f >> 4) * NKK + kk) * 64 + q * 16 + (f & 15)) * 16) = u32x4{w[0], w[1], w[2], w[3]};
        }
    }
    // y0 into the feedback columns: one quad of outputs per (frame, quad), as finish_readout stores them
    if (p.y0) {
        for (int i = tid; i < BT * 2; i += NTHREADS) {
            const int f = i & (BT - 1), o0 = 4 * (i >> 7);
            const bool live = tab_fr[f] >= 0;
            const double* yr = p.y0 + (size_t)(live ? tab_grp[f] : 0) * n_out;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (live && o0 + e < n_out) ? (float)yr[o0 + e] : 0.f;
            const int pos = g.kfb - S16_MP + o0;                         // position inside the [U ; F] group
            if (o0 < kfb_p)
                TR::store4(zf + ((size_t)((f >> 4) * NKK + 16) * 64 + (pos >> 3) * 16 + (f & 15)) * 16 + 2 * (pos & 7),
                           v[0], v[1], v[2], v[3]);
        }
    }
    __syncthreads();

    // ---- the wave's own column tile (tile `wave`): read-out lane view = output rows 4 oq .. 4 oq + 3 of frame ofc
    // (oq = lane >> 4, ofc = lane & 15: finish_readout)
    const int own_grp = __builtin_amdgcn_readfirstlane(slot_group(p, slot0 + wave * 16));
    const bool has_ro = own_grp < p.n_groups;                 // wave-uniform
    float wo_inv = 1.f;
    if (has_ro)
        wo_inv = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.packed_wout)
                                                 + (size_t)own_grp * p.wout_stride + p.wo16_off + (size_t)NKK * 1024);
    const uint32_t in_stride = (uint32_t)(p.T_in * n_in);
    // inputs of step 0, straight from HBM (every later step arrives by LDS-DMA)
    // (the [U ; F] group keeps natural order: input ci of frame f at position ci of group 16)
    for (int e = tid; e < BT * kin_p; e += NTHREADS) {
        const int f = e >> lkin, ci = e & (kin_p - 1);
        const int fr = tab_fr[f];
        float v = 0.f;
        if (fr >= 0 && ci < n_in) {
            const int row = p.in_row_off;
            const double raw = (row < p.T_in) ? (double)in_ptr<IO32>(p)[(size_t)fr * in_stride + (size_t)row * n_in + ci] : 0.0;
            const float2 ss = tab_in[(f >> 4) * kin_p + ci];
            v = fmaf((float)raw, ss.x, ss.y);
        }
        TR::store1(zf + ((size_t)((f >> 4) * NKK + 16) * 64 + (ci >> 3) * 16 + (f & 15)) * 16 + 2 * (ci & 7), v);
    }

    const NoiseCoef nc = noise_coef(p.noise);
    f32x4 yacc = {0.f, 0.f, 0.f, 0.f};
    const int lane16 = lane * 16;
    constexpr int OOB = 0x7ffffff0;

    // Y complete: feedback columns into the image, unscaled output row `orow` to HBM, reset yacc
    auto finish_readout = [&](int orow, bool write_fb) S16_INLINE {
        int ln_ro = lane;
        asm volatile("" : "+v"(ln_ro));                      // derived per step, not kept across the GEMM phases
        const int ofc = ln_ro & 15, oq = ln_ro >> 4;
        if (!has_ro) return;
        const int of = wave * 16 + ofc;
        f32x4 y = yacc;
        const int o0 = 4 * oq;
        const int fr = tab_fr[of];
        const float4* un4 = reinterpret_cast<const float4*>(tab_un + wave * 16 + o0);           // {1/scale, shift} x 4
        const float4 u01 = un4[0], u23 = un4[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] += __shfl_xor(y[j], 32);        // rows 8..15: the residual image's product
        y *= wo_inv;
        if (o0 < kfb_p) {
            if (write_fb) {
                const int pos = g.kfb - S16_MP + o0;                     // position inside the [U ; F] group
                TR::store4(zf + ((size_t)(wave * NKK + 16) * 64 + (pos >> 3) * 16 + ofc) * 16 + 2 * (pos & 7),
                           y[0], y[1], y[2], y[3]);
            }
            if (IO32 && orow >= 0 && fr >= 0) {        // the float64 path's values, one 16-byte store per quad
                float* yo = p.Y32 + ((size_t)fr * out_rows + orow) * n_out;
                if ((n_out & 3) == 0) {
                    *reinterpret_cast<float4*>(yo + o0) =
                        make_float4((y[0] - u01.y) * u01.x, (y[1] - u01.w) * u01.z, (y[2] - u23.y) * u23.x, (y[3] - u23.w) * u23.z);
                } else {
                    const float2* un = tab_un + wave * 16 + o0;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (o0 + j < n_out) yo[o0 + j] = (y[j] - un[j].y) * un[j].x;
                }
            } else if (!IO32 && orow >= 0 && fr >= 0) {
                double* yo = p.Y + ((size_t)fr * out_rows + orow) * n_out;
                if ((n_out & 3) == 0) {
                    typedef double f64x2s __attribute__((ext_vector_type(2)));
                    *reinterpret_cast<f64x2s*>(yo + o0) =
                        f64x2s{(double)((y[0] - u01.y) * u01.x), (double)((y[1] - u01.w) * u01.z)};
                    *reinterpret_cast<f64x2s*>(yo + o0 + 2) =
                        f64x2s{(double)((y[2] - u23.y) * u23.x), (double)((y[3] - u23.w) * u23.z)};
                } else {
                    const float2* un = tab_un + wave * 16 + o0;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (o0 + j < n_out) yo[o0 + j] = (double)((y[j] - un[j].y) * un[j].x);
                }
            }
        }
        yacc = f32x4{0.f, 0.f, 0.f, 0.f};
    };

    // ================= skewed schedule =============================================================
    // slot 3s   : A P0(s) reads X_A(s)            B P2(s-1) writes X_B(s)
    // slot 3s+1 : A P1(s) reads X_B(s)            B P0(s)   reads X_A(s)     + read-out Y_s -> F_s (both sets)
    // slot 3s+2 : A P2(s) writes X_A(s+1)         B P1(s)   reads X_B(s)     + yU_s
    const int lag = wave >= NW / 2 ? 1 : 0;
    f32x4 acc[4][8];
    u32x4 abuf[2][4], b[4], ra[4];
    auto zero_acc = [&]() S16_INLINE {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 8; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.packed_w) + (size_t)wset * p.wset_stride + p.w16_off), 0,
        S16_MP * NKK * 64, 0x00020000);
    const int w_frag0 = wave * NKK * 4;                    // fragment (wave, kk, m) at ((wave NKK + kk) 4 + m) KB
    auto loadA = [&](u32x4 (&a)[4], int kk) S16_INLINE {  // kk >= NKK: zeros, no traffic
        const bool live = kk < NKK;
        const int voff = live ? lane16 : OOB;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            a[m] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                w_rsrc, voff, live ? (w_frag0 + kk * 4 + m) * 1024 : 0, 0));
    };
    const __amdgpu_buffer_rsrc_t wo_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.packed_wout)
                          + (size_t)(has_ro ? own_grp : 0) * p.wout_stride + p.wo16_off),
        0, NKK * 1024 + 16, 0x00020000);
    // W_out fragments of one trip (two groups): ra[2j] = group kk0 + i + j (the half being multiplied),
    // ra[2j+1] = group (kk0 + i + j) ^ 8 (the other half); `on` false: zeros, no traffic
    auto load_ra = [&](int j, int kk, bool on) S16_INLINE {
        on = on && kk < 2 * NKH;
        const int voff = on ? lane16 : OOB;
        ra[2 * j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wo_rsrc, voff, on ? kk * 1024 : 0, 0));
        ra[2 * j + 1] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wo_rsrc, voff, on ? (kk ^ 8) * 1024 : 0, 0));
    };
    auto ro_prefetch = [&](int kk0, bool on) S16_INLINE { load_ra(0, kk0, on); load_ra(1, kk0 + 1, on); };
    typedef const __attribute__((address_space(3))) u32x4* lds_frag_t;
    // State groups [kk0, kk0 + 8) out of abuf, two per trip; abuf[j] holds group kk0 + j on entry and kk0 + 8 + j on
    // exit.  B ring: slot n & 3 holds column tile n's fragment and is refilled behind that tile's four MFMAs with
    // tile n + 4's (n < 4: same group; else tile n - 4 of the next group) -- twelve MFMAs of look-ahead, 16 registers.
    // RO: the read-out of the own tile rides along, both halves of k per group position (a wave reads out in ONE of its
    // two halves per step, see run_set; the other half is instantiated without it).
    auto gemm_half = [&](int kk0, auto ro_tag, bool ro_on) S16_INLINE {
        constexpr bool RO = decltype(ro_tag)::value;
        const int voff_ro = ro_on ? lane16 : OOB;      // (step 0 and tiles of padding: zero fragments, no traffic)
        // (addresses re-derived from the lane id per call, opaque to the optimiser: kept live across the step loop they
        //  are spilled, and a scratch reload in front of the loop costs an s_waitcnt vmcnt(0) INSIDE it -- the reload is
        //  the youngest vector-memory operation, so waiting for it drains the whole weight prefetch every trip)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const uint32_t zb = (uint32_t)(uintptr_t)zf + (uint32_t)(ln << 4);
        uint32_t bp0 = zb + (uint32_t)kk0 * 1024;                               // tiles 0-3 / 4-7 of group kk0 + i
        uint32_t bp1 = bp0 + 4 * TILE_B;
#pragma unroll
        for (int n = 0; n < 4; ++n) b[n] = *reinterpret_cast<lds_frag_t>((uintptr_t)(bp0 + n * TILE_B));
        uint32_t rp = zb + (uint32_t)(wave * TILE_B) + (uint32_t)kk0 * 1024;      // own tile, this half / other half
        uint32_t xp = zb + (uint32_t)(wave * TILE_B) + (uint32_t)(kk0 ^ 8) * 1024;
        int sA = (w_frag0 + (kk0 + 2) * 4) * 1024;        // weight fragments two groups ahead
        int sR = (kk0 + 2) * 1024;                        // W_out fragments one trip ahead
        auto trip = [&](int i, auto tail_tag) S16_INLINE {
            constexpr bool TAIL = decltype(tail_tag)::value;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int kk = kk0 + i + j;
                u32x4 rb0, rbx;
#pragma unroll
                for (int n = 0; n < 8; ++n) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        TR::mma16(acc[m][n], abuf[j][m], b[n & 3]);
                        const int u = n * 4 + m;
                        if (RO) {      // own tile's fragments of this group and of its twin in the other half; the W_out
                                       // fragments of the next trip go out right behind the read-out MFMA that used them
                            if (u == 0) rb0 = *reinterpret_cast<lds_frag_t>((uintptr_t)(rp + j * 1024));
                            if (u == 1) rbx = *reinterpret_cast<lds_frag_t>((uintptr_t)(xp + j * 1024));
                            // (none in the last trip: the next reader of ra is behind the next ro_prefetch)
                            if (u == 8) {
                                TR::mma16(yacc, ra[2 * j], rb0);
                                if (!TAIL)
                                    ra[2 * j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                        wo_rsrc, voff_ro, sR + j * 1024, 0));
                            }
                            if (u == 10) {
                                TR::mma16(yacc, ra[2 * j + 1], rbx);
                                if (!TAIL)
                                    ra[2 * j + 1] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                        wo_rsrc, voff_ro, (sR ^ 8192) + j * 1024, 0));
                            }
                        }
                        if (n == 7) {                     // weight fragment m of the group two ahead
                            if (TAIL) {
                                const bool live = kk + 2 < NKK;
                                abuf[j][m] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                    w_rsrc, live ? lane16 : OOB, live ? (w_frag0 + (kk + 2) * 4 + m) * 1024 : 0, 0));
                            } else {
                                abuf[j][m] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                    w_rsrc, lane16, sA + (j * 4 + m) * 1024, 0));
                            }
                        }
                        if (m == 3) {
                            if (n < 4) b[n] = *reinterpret_cast<lds_frag_t>((uintptr_t)(bp1 + n * TILE_B + j * 1024));
                            else b[n - 4] = *reinterpret_cast<lds_frag_t>((uintptr_t)(bp0 + (n - 4) * TILE_B + (j + 1) * 1024));
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            asm volatile("v_add_u32 %0, 2048, %0" : "+v"(bp0));
            asm volatile("v_add_u32 %0, 2048, %0" : "+v"(bp1));
            if (RO) { rp += 2048; xp += 2048; }
            sA += 8192;
            sR += 2048;
        };
        // (Tried: a peeled first trip whose MFMAs start from C = 0 instead of the 128 v_mov of zero_acc -- the third copy of
        //  the trip body costs 20-35 spilled registers in the hot path: 14.5 vs 11.9 ms.)
        for (int i = 0; i < NKH - 2; i += 2) trip(i, std::false_type{});
        trip(NKH - 2, std::true_type{});
    };
    // [U ; F] group: abuf[0] holds group 16 on entry
    auto uf_group = [&](u32x4 ra_u) S16_INLINE {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const uint32_t up = (uint32_t)(uintptr_t)zf + (uint32_t)(ln << 4) + 16 * 1024;
#pragma unroll
        for (int n = 0; n < 4; ++n) b[n] = *reinterpret_cast<lds_frag_t>((uintptr_t)(up + n * TILE_B));
        {   // yU_s = Wout[:, inputs] U_s (the feedback columns of that group carry zero weights)
            const u32x4 rb_u = *reinterpret_cast<lds_frag_t>((uintptr_t)(up + wave * TILE_B));
            TR::mma16(yacc, ra_u, rb_u);
        }
#pragma unroll
        for (int n = 0; n < 8; ++n) {
#pragma unroll
            for (int m = 0; m < 4; ++m) TR::mma16(acc[m][n], abuf[0][m], b[n & 3]);
            if (n < 4) b[n] = *reinterpret_cast<lds_frag_t>((uintptr_t)(up + (n + 4) * TILE_B));
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto next_step_A = [&]() S16_INLINE { loadA(abuf[0], 0); loadA(abuf[1], 1); };

    // phase E for tile positions [N0, N1): eight values per lane and row-tile pair -> one 16-byte store
    constexpr bool PK_NOISE = NOISE == ESN_NOISE_COUNTER && std::is_same<TR, TraitsF16>::value;
    const NoiseCoefHalf nh = noise_coef_half(nc);
    const uint32_t seed_hi = (uint32_t)(p.seed >> 32);
    auto activate = [&](int s, auto n0_tag, auto n1_tag, int ln) S16_INLINE {
        constexpr int N0 = decltype(n0_tag)::value, N1 = decltype(n1_tag)::value;
        const int g4 = ln >> 4, col = ln & 15;
        uint32_t k1[N1 - N0];
        int frs[N1 - N0];
#pragma unroll
        for (int n = N0; n < N1; ++n) {
            const int t = n;
            if (NOISE == ESN_NOISE_COUNTER) k1[n - N0] = tab_ks[(s & 1) * BT + t * 16 + col];
            if (NOISE == ESN_NOISE_TENSOR) frs[n - N0] = tab_fr[t * 16 + col];
        }
#pragma unroll
        for (int n = N0; n < N1; ++n) {
            const int t = n;
            uint32_t key = 0;
            const double* nz = nullptr;
            if (NOISE == ESN_NOISE_COUNTER)        // noise_key(seed, frame, step) + row4 stride: row4 = 16 wave + 4 m + g4
                key = k1[n - N0] + (uint32_t)(16 * wave + g4) * NOISE_ROW4_STRIDE;
            if (NOISE == ESN_NOISE_TENSOR && frs[n - N0] >= 0)
                nz = p.noise_u + ((size_t)frs[n - N0] * p.S + s) * n_res;
            char* dst = zf + (size_t)t * TILE_B + (size_t)(2 * wave) * 1024 + (size_t)ln * 16;
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                uint32_t out[4];
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    const int m = 2 * pr + tt;
                    const f32x4 a4 = acc[m][n];
                    if constexpr (PK_NOISE) {
                        float tv[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) tv[j] = biased_tanh(a4[j], nh);
                        const u32x2 x = noised_half_quad(tv, noise_quad(key, (uint32_t)(4 * m)), nh);
                        out[2 * tt] = x[0];
                        out[2 * tt + 1] = x[1];
                    } else {
                        float v[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = TR::act(a4[j]);
                        add_state_noise<NOISE>(v, noise_quad(key, (uint32_t)(4 * m)), nz, p.noise_u, 64 * wave + 16 * m + 4 * g4,
                                               n_res, nc);
                        out[2 * tt] = TR::pack2(v[0], v[1]);
                        out[2 * tt + 1] = TR::pack2(v[2], v[3]);
                    }
                }
                *reinterpret_cast<u32x4*>(dst + pr * 1024) = u32x4{out[0], out[1], out[2], out[3]};
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    const std::integral_constant<int, 0> n_lo;
    const std::integral_constant<int, 4> n_mid;
    const std::integral_constant<int, 8> n_hi;

    // ---- inputs: set B stages them for all column tiles, two tiles per wave (as in the 32x32x16 kernel) ----------
    // float32 I/O: 16-byte chunks of four inputs (n_in % 4 == 0), else 4-byte chunks of one (n_in = 2: the skewed kernels
    // take n_in in {2, 4, 8, 16}); either way 16 cpf <= 64 chunks per tile, ONE DMA instruction, the tile's rows back to
    // back in its slot
    const bool in_w16 = !IO32 || (n_in & 3) == 0;      // (U is then 16-byte aligned: esn_predict_batch_f32)
    const int cpf = IO32 ? (in_w16 ? n_in / 4 : n_in) : n_in / 2;      // chunks per frame row
    constexpr int IN_TRIPS = IO32 ? 1 : 2;
    constexpr int IN_TILES = NOWN / (NW / 2);
    const int in_c0 = IN_TILES * (wave - NW / 2);
    const int lcpf = __builtin_ctz(cpf);
    const size_t in_frame_bytes = (size_t)in_stride * sizeof(io_elem<IO32>);
    int j0;
    slot_group(p, slot0, j0);
    size_t u_base_frame = j0 < p.F ? (size_t)grp0 * p.F + j0 : ((size_t)grp0 + (p.spw ? p.n_wsets : 1)) * p.F;
    if (u_base_frame >= (size_t)p.n_frames) u_base_frame = (size_t)p.n_frames - 1;
    for (int i = tid; i < BT; i += NTHREADS) {
        const int fr = tab_fr[i];
        tab_off[i] = fr >= 0 ? (int)(((size_t)fr - u_base_frame) * in_frame_bytes) : -1;
    }
    __syncthreads();
    const size_t u_left = ((size_t)p.n_frames - u_base_frame) * in_frame_bytes;
    // The base and the record count are uniform (kernel arguments and the tile's first slot), but they come out of
    // integer divisions, which run on the vector ALU: built from them as they are, the descriptor sits in four VGPRs
    // and every LDS-DMA launch of dma_inputs_b is wrapped in a readfirstlane loop.  One readfirstlane set here instead
    const uintptr_t u_base = reinterpret_cast<uintptr_t>(p.U) + u_base_frame * in_frame_bytes;
    const uint32_t u_base_lo = __builtin_amdgcn_readfirstlane((uint32_t)u_base);
    const uint32_t u_base_hi = __builtin_amdgcn_readfirstlane((uint32_t)(u_base >> 32));
    const int u_records = __builtin_amdgcn_readfirstlane((int)(u_left < 0x7fffffffu ? u_left : 0x7fffffffu));
    const __amdgpu_buffer_rsrc_t u_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<char*>(((uintptr_t)u_base_hi << 32) | u_base_lo), 0, u_records, 0x00020000);
    auto dma_inputs_b = [&](int s) S16_INLINE {
        const int row = s + p.in_row_off;
        const bool row_ok = row < p.T_in;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        int off[IN_TILES][IN_TRIPS];
#pragma unroll
        for (int ti = 0; ti < IN_TILES; ++ti)
#pragma unroll
            for (int i = 0; i < IN_TRIPS; ++i) {
                const int e = 64 * i + ln;
                off[ti][i] = tab_off[(in_c0 + ti) * 16 + ((e >> lcpf) & 15)];
            }
#pragma unroll
        for (int ti = 0; ti < IN_TILES; ++ti) {
            const int c = in_c0 + ti;
#pragma unroll
            for (int i = 0; i < IN_TRIPS; ++i) {
                const int e = 64 * i + ln;
                const bool on = off[ti][i] >= 0 && row_ok && e < 16 * cpf;
                if constexpr (IO32) {
                    auto* slot = (__attribute__((address_space(3))) void*)(in_slots + (size_t)(c * 2 + i) * 1024);
                    const int voff = on ? off[ti][i] + ((e & (cpf - 1)) << (in_w16 ? 4 : 2)) : OOB;
                    if (in_w16)
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(u_rsrc, slot, 16, voff, row_ok ? row * n_in * 4 : 0, 0, 0);
                    else
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(u_rsrc, slot, 4, voff, row_ok ? row * n_in * 4 : 0, 0, 0);
                } else {
                    const int voff = on ? off[ti][i] + ((e & (cpf - 1)) << 4) : OOB;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(
                        u_rsrc, (__attribute__((address_space(3))) void*)(in_slots + (size_t)(c * 2 + i) * 1024), 16,
                        voff, row_ok ? row * n_in * 8 : 0, 0, 0);
                }
            }
        }
    };
    auto commit_inputs_b = [&](int s) S16_INLINE {
        const bool row_ok = s + p.in_row_off < p.T_in;
        const int lk2 = lkin - 1;
        int ln = lane;
        asm volatile("" : "+v"(ln));
#pragma unroll
        for (int ti = 0; ti < IN_TILES; ++ti) {
            const int c = in_c0 + ti;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int e2 = ln + 64 * k;
                const int f = (e2 >> lk2) & 15, c2 = e2 & ((kin_p >> 1) - 1), ci = 2 * c2;
                const bool live = tab_fr[c * 16 + f] >= 0 && ci < n_in;
                const float4 ss = *reinterpret_cast<const float4*>(tab_in + c * kin_p + ci);
                double2 raw;
                if constexpr (IO32) {
                    const float2 r32 = *reinterpret_cast<const float2*>(in_slots + (size_t)c * 2048 + (size_t)(f * n_in + ci) * 4);
                    raw = double2{(double)r32.x, (double)r32.y};
                } else {
                    const int ch = (f << lcpf) + c2;
                    raw = *reinterpret_cast<const double2*>(
                        in_slots + (size_t)(c * 2 + (ch >> 6)) * 1024 + (size_t)(ch & 63) * 16);
                }
                const float v0 = live ? fmaf((float)(row_ok ? raw.x : 0.0), ss.x, ss.y) : 0.f;
                const float v1 = live ? fmaf((float)(row_ok ? raw.y : 0.0), ss.z, ss.w) : 0.f;
                if (e2 < 8 * kin_p)
                    TR::store2(zf + ((size_t)(c * NKK + 16) * 64 + (ci >> 3) * 16 + f) * 16 + 2 * (ci & 7), v0, v1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // stamped build: a barrier split into its fence (the wave's own stores and LDS-DMA draining) and the s_barrier
    // itself (waiting for the other waves), with a stamp between the two
#ifdef ESN_STAMPS
    unsigned long long sk_acc[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define ESN_SK_ADD(i, a, b) sk_acc[i] += (b) - (a);
#define ESN_SYNC_SPLIT(mid) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); ESN_STAMP(mid) \
    __builtin_amdgcn_s_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#else
#define ESN_SK_ADD(i, a, b)
#define ESN_SYNC_SPLIT(mid) __syncthreads();
#endif
    const uint32_t key1_own = tab_key[wave * 16 + (lane & 15)];
    ESN_STAMP(t_prologue)
    // The step loop, once per wave set, entered by ONE wave-uniform branch: inside a body LAG is a constant, so a wave's
    // half without the read-out is gemm_half<RO = false> (no read-out MFMAs on zero fragments, no ds_read of the own
    // tile, no out-of-bounds W_out loads: about 100 instructions per wave and step, 16 of them MFMAs) and every
    // per-set choice (input commit, LDS-DMA launches, priorities, which phase finishes the read-out) is compile-time
    // code.  No accumulator is live across the branch, which is what a branch around the MFMAs inside ONE loop could
    // not have (the compiler shuffled the accumulators between its arms: 290 spilled registers).
    // Results are bitwise those of the one-path loop: the MFMAs that are gone added 0 * x to yacc for finite x, and
    // yacc is never -0.0 (it starts at +0.0, and under round-to-nearest a sum with a +0.0 term, or one that cancels
    // exactly, is +0.0), so yacc + (+-0.0) == yacc bit for bit.
    // Barriers: both bodies execute three s_barrier per step; set B one more before its loop (slot 0 is set A's alone)
    // and set A one more behind it (slot 3S: set B finishes X_B(S)).
    auto run_set = [&](auto lag_tag) S16_INLINE {
        constexpr bool LAG = decltype(lag_tag)::value;
        next_step_A();
        if (LAG) {
            ro_prefetch(0, false);                                 // step 0 reads nothing out: zero fragments
            __syncthreads();                                       // slot 0: set A alone
        }
        for (int s = 0; s < p.S; ++s) {
            const bool ro = has_ro && s > 0;
            ESN_STAMP(t0)
            zero_acc();
            // ---- P0 (set A: slot 3s; set B: slot 3s+1 with the read-out of Y_s)
            if (LAG) __builtin_amdgcn_s_setprio(1);
            if (NOISE == ESN_NOISE_COUNTER) {      // keys of step s for the own tile's frames: read from slot 3s+2 on
                const uint32_t k = mix32(key1_own ^ seed_hi ^ ((uint32_t)s * 0x85EBCA6BU + 0x27d4eb2fU));
                if (lane < 16) tab_ks[(s & 1) * BT + wave * 16 + lane] = k;
            }
            if (LAG) {
                if (s > 0) commit_inputs_b(s);
                gemm_half(0, std::true_type{}, ro);
                if (ro) finish_readout(s - 1 - p.transient, true);
                __builtin_amdgcn_s_setprio(0);
            } else {
                gemm_half(0, std::false_type{}, false);
                ro_prefetch(NKH, ro);                              // for P1, in flight over the barrier
            }
            ESN_STAMP(t1)
            ESN_SYNC_SPLIT(m1)
            ESN_STAMP(t2)
#ifdef ESN_STAMPS
            unsigned long long u3 = 0, u4 = 0;                     // around set B's LDS-DMA launches, inside its P1
#endif
            // ---- P1 (set A: slot 3s+1 with the read-out; set B: slot 3s+2)
            // W_out fragment of the [U ; F] group, consumed by the first MFMA group of P2: launched here so that it is in
            // flight across the barrier (the ra[] registers are dead from here to the next ro_prefetch in both sets)
            auto load_ra_u = [&]() S16_INLINE {
                return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                    wo_rsrc, has_ro ? lane16 : OOB, has_ro ? 16 * 1024 : 0, 0));
            };
            u32x4 ra_u;
            if (LAG) {
                gemm_half(NKH, std::false_type{}, false);
                ra_u = load_ra_u();
                // inputs of step s + 1, launched into the time set B waits for set A's phase E (slot 3s+2 is bound by
                // it); the staging slots are free, their last reader was this wave's commit_inputs_b(s).  Inside
                // phase E the launches held the wave for a thousand cycles: the LDS reads behind them wait for the DMA
                ESN_STAMP_SET(u3)
                if (s + 1 < p.S) dma_inputs_b(s + 1);
                ESN_STAMP_SET(u4)
            } else {
                gemm_half(NKH, std::true_type{}, ro);
                if (ro) finish_readout(s - 1 - p.transient, true);
                ra_u = load_ra_u();
            }
            ESN_STAMP(t3)
            ESN_SYNC_SPLIT(m3)
            ESN_STAMP(t4)
            // ---- P2: [U ; F] group + phase E
            __builtin_amdgcn_s_setprio(2);
            int ln_e = lane;
            asm volatile("" : "+v"(ln_e));
            uf_group(ra_u);
            ESN_STAMP(u1)
            activate(s, n_lo, n_mid, ln_e);
            ESN_STAMP(u2)
            next_step_A();
            if (LAG) ro_prefetch(0, has_ro && s + 1 < p.S);        // for P0(s+1)
            ESN_STAMP(u2b)
            activate(s, n_mid, n_hi, ln_e);
            ESN_STAMP(u5)
            __builtin_amdgcn_s_setprio(0);
            ESN_STAMP(t5)
            __syncthreads();
            ESN_STAMP(t6)
            ESN_SK_ADD(0, t0, t1) ESN_SK_ADD(1, t1, t2) ESN_SK_ADD(2, t2, t3)
            ESN_SK_ADD(3, t3, t4) ESN_SK_ADD(4, t4, t5) ESN_SK_ADD(5, t5, t6)
            ESN_SK_ADD(6, t4, u1) ESN_SK_ADD(7, u1, u2) ESN_SK_ADD(8, u2, u2b) ESN_SK_ADD(9, u3, u4)
            ESN_SK_ADD(10, u2b, u5) ESN_SK_ADD(11, u5, t5) ESN_SK_ADD(12, t1, m1) ESN_SK_ADD(13, t3, m3)
        }
    };
    if (lag) run_set(std::true_type{}); else run_set(std::false_type{});
#undef ESN_SK_ADD
#undef ESN_SYNC_SPLIT
#ifdef ESN_STAMPS
    if (p.stamps && blockIdx.x == 0 && lane == 0) {
        p.stamps[wave * 8 + 7] = t_prologue - t_entry;                // kernel entry to the first step
        for (int i = 0; i < 2; ++i) p.stamps[(8 + wave) * 8 + 6 + i] = sk_acc[12 + i];   // fence share of "wait Ba" / "wait Bb"
        for (int i = 0; i < 6; ++i) p.stamps[wave * 8 + i] = sk_acc[i];
        for (int i = 0; i < 6; ++i) p.stamps[(8 + wave) * 8 + i] = sk_acc[6 + i];    // inside P2
        p.stamps[wave * 8 + 6] = (unsigned long long)__builtin_amdgcn_s_getreg(63492);   // HW_ID
    }
#endif
    if (!lag) __syncthreads();                                     // slot 3S: set B finishes X_B(S)
    if (has_ro) {                                                  // Y_S = yU_{S-1} + Wout_x X_S
        for (int kk = 0; kk < 2 * NKH; ++kk) {
            const u32x4 rb = *reinterpret_cast<const u32x4*>(zf + (size_t)(wave * NKK + kk) * 1024 + lane16);
            const u32x4 rw = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wo_rsrc, lane16, kk * 1024, 0));
            TR::mma16(yacc, rw, rb);
        }
        finish_readout(p.S - 1 - p.transient, false);
    }
}
#undef S16_INLINE

template <typename TR, bool IO32>
static int launch_skew16(const RecurParams& p, hipStream_t stream) {
    const int kin_p = p.g.kfb - p.g.kin;
    const size_t lds = (size_t)8 * S16_NKK * 1024 + 4 * 128 + 4 * 128 + 8 * (size_t)8 * (kin_p + 16) + 8 * 2048 + 4 * 128 + 8 * 128;
    auto go = [&](auto kern) -> int {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(kern, dim3(p.n_tiles), dim3(512), lds, stream, p);
        return (int)hipGetLastError();
    };
    switch (p.noise_mode) {
        case ESN_NOISE_NONE: return go(recur_skew16_kernel<TR, ESN_NOISE_NONE, IO32>);
        case ESN_NOISE_TENSOR: return go(recur_skew16_kernel<TR, ESN_NOISE_TENSOR, IO32>);
        default: return go(recur_skew16_kernel<TR, ESN_NOISE_COUNTER, IO32>);
    }
}

}  // namespace esn
