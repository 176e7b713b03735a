// Fused detector tail, one workgroup per frame, one wave per tx antenna:
//   x[n] = Y[frame][n][2tx] + j Y[frame][n][2tx+1]            (driver :47-58, delay offset 0)
//   X    = FFT_N(x) / (N sqrt(Pi))                             (driver :439-441)
//   idx  = nearest point of the unit-power square QAM grid     (driver :17-28, :95-103)
//   bits = natural binary of idx, LSB first; errors vs TxBits  (driver :30-32, :451-456)
// float64 throughout, radix-2 FFT in LDS.
#include "esn_common.h"
#include "esn_launch.h"
#include "esn_ofdm_math.h"
#include <type_traits>

namespace esn {

// One workgroup per frame, 32 threads per tx antenna (n_t <= 16): the frame's rows are read once,
// fully coalesced (a row is n_t complex doubles), the twiddles come from one table per workgroup
// (same sincospi arguments as the reference order), the transform is ofdm_fft_lds of esn_ofdm_math.h.
// IO32: float32 Y (esn_detect_count_f32), widened on load into the same float64 buffer -- counts and X_hat are those
// of the float64 entry point on the widened Y
template <bool IO32>
__global__ __launch_bounds__(1024) void detect_count_kernel(DetectParams dp) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    const int N = dp.n_sub, n_t = dp.n_t, tid = threadIdx.x, half = N >> 1;
    const int nthr = blockDim.x;
    const int na_max = dp.na_wg;                             // antennas per workgroup
    const int n_chunks = (n_t + na_max - 1) / na_max;
    const int ld = N + 1;                                    // row pad: stage strides are powers of two
    double2* buf = reinterpret_cast<double2*>(dsm);          // [n_t][ld]
    double2* tw = buf + (size_t)na_max * ld;                 // [N/2]  exp(-2 pi i k / N)
    __shared__ int red[16];
    const int frame = blockIdx.x / n_chunks;
    const int a0 = (blockIdx.x - frame * n_chunks) * na_max;
    const int na = (n_t - a0 < na_max) ? n_t - a0 : na_max;
    const int group = frame / dp.frames_per_group;
    const double2* y = reinterpret_cast<const double2*>(dp.Y) + (size_t)frame * N * n_t;
    const float2* y32 = reinterpret_cast<const float2*>(dp.Y32) + (size_t)frame * N * n_t;

    // transmitted bits of the elements this thread will slice (the m x n_t bytes of a subcarrier are contiguous), fetched
    // NOW: the slicer at the end would otherwise pay a second global round trip behind the FFT
    constexpr int TXP = 4;                                   // elements prefetched per thread (N na / nthr at the benchmark shape)
    const bool tx_pre = dp.m == 4 && n_t == 4 && na == n_t && N * na <= TXP * nthr && ((uintptr_t)dp.tx_bits & 15) == 0;
    uint4 txw[TXP];
    if (tx_pre) {
#pragma unroll
        for (int q = 0; q < TXP; ++q) {
            const int e = tid + q * nthr, k = e / na;
            txw[q] = (e < N * na) ? *reinterpret_cast<const uint4*>(dp.tx_bits + ((size_t)frame * N + k) * 16) : uint4{0, 0, 0, 0};
        }
    }
    const double p_i_g = dp.p_i[group];
    ofdm_twiddles(tw, half, N, -1.0);
    for (int i = tid; i < N * na; i += nthr) {               // bit-reversed load, element i = (row, antenna)
        const int row = i / na, ant = i - row * na;
        const int rv = (int)(__brev((unsigned)row) >> (32 - dp.log2n));
        if constexpr (IO32) {
            const float2 v = y32[(size_t)row * n_t + a0 + ant];
            buf[ant * ld + rv] = make_double2((double)v.x, (double)v.y);
        } else {
            buf[ant * ld + rv] = y[(size_t)row * n_t + a0 + ant];
        }
    }
    __syncthreads();
    ofdm_fft_lds(buf, na, ld, tw, N, dp.log2n);

    const int side = 1 << (dp.m / 2);
    const double norm = det_norm(side);
    const double scale = det_scale(N, p_i_g);
    int errs = 0;
    for (int e = tid; e < N * na; e += nthr) {               // element e = (subcarrier k, antenna), antenna fastest
        const int k = e / na, ant = a0 + e - k * na;
        const double2 v = buf[(ant - a0) * ld + k];
        const double re = v.x * scale, im = v.y * scale;
        if (dp.X_hat)
            reinterpret_cast<double2*>(dp.X_hat)[((size_t)frame * N + k) * n_t + ant] = make_double2(re, im);
        const int idx = det_slice(re, norm, side) * side + det_slice(im, norm, side);
        if (tx_pre) {                                        // byte bb n_t + ant of the subcarrier's 16
            const int q = (e - tid) / nthr;
            uint4 w = txw[0];
#pragma unroll
            for (int qq = 1; qq < TXP; ++qq) if (q == qq) w = txw[qq];
            const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) errs += (int)(((uint32_t)(idx >> bb) & 1u) != ((wd[bb] >> (8 * ant)) & 0xffu));
        } else {
            errs += det_bit_errors(idx, dp.tx_bits + ((size_t)frame * N + k) * dp.m * n_t + ant, n_t, dp.m);
        }
    }
    det_count_tail(true, errs, red, dp.err + group, dp.bits + group, N * dp.m * na);
}

// ---- fixed-shape instances -------------------------------------------------------------------------------------------
// One wave per workgroup, kDetFixedFrames consecutive frames per workgroup, one frame at a time in the wave:
//   lane = (antenna a = lane & 3, r = lane >> 2), eight points per lane.  The lane loads rows r + 16 j (j = 0..7)
//   of its antenna -- one instruction covers 16 consecutive rows, 1 KB -- which in bit-reversed order are positions
//   8 rev4(r) + t (t = rev3(j)): the inputs of stages 1-3, which run in registers.  Two exchanges through the wave's
//   own 8 KB of LDS regroup the points for stages 4-5 (positions 32 u + 8 v + t', v = 0..3) and 6-7 (32 v + w), a
//   third one hands X to the slicer, lane = subcarrier (and + 64), all four antennas -- one 16-byte word of tx_bits
//   per subcarrier, compared on packed bytes.  The slot permutations make every 16-byte LDS access conflict-free
//   (reads in the 16-lane groups of ds_read_b128, writes in runs of 8 lanes).  LDS of one wave is in program order,
//   so the exchanges need no s_barrier.  Same butterflies on the same operands as the generic kernel (stage s pairs
//   x and x + 2^(s-1) with twiddle tw[(x mod 2^(s-1)) N / 2^s]), so the spectrum is bit-identical.
// Per workgroup, not per frame: the twiddle table, norm, the group and scale of each of its frames (lane i holds those
// of frame i); counters go out once per run of frames of one group.  Rows and tx words of frame f + 1 are issued before
// the butterflies of frame f start (two register sets, the loop takes two frames per trip).
constexpr int kDetFixedFrames = 8;
constexpr int kDetFixedLdsX = 4 * 130 * 16;                   // exchange area: [4][130] double2 is the widest image
constexpr int kDetFixedLds = kDetFixedLdsX + 64 * 16;         // + twiddles [64]

__device__ __forceinline__ void det_wave_sync() {             // orders this wave's LDS writes before its later reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ double det_uniform(double v) {     // a wave-uniform double, held in scalar registers
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ __forceinline__ double det_lane_double(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                            __builtin_amdgcn_readlane(__double2loint(v), lane));
}

template <bool IO32, int LOG2N, int NT, int M>
__global__ __launch_bounds__(64) void detect_count_fixed_kernel(DetectParams dp) {
    // the lane map below is the one of 128 subcarriers x 4 antennas with one 16-byte tx word per subcarrier; another
    // shape needs its own map beside the instantiation
    static_assert(LOG2N == 7 && NT == 4 && M * NT == 16, "detect_count_fixed_kernel: lane map of (7, 4, 4)");
    constexpr int N = 1 << LOG2N, SIDE = 1 << (M / 2);
    using YT = typename std::conditional<IO32, float2, double2>::type;
    struct Pre { YT y[8]; uint4 tx[2]; };                     // one frame's rows and tx words, in flight
    __shared__ __attribute__((aligned(16))) char sm[kDetFixedLds];
    const int lane = threadIdx.x, a = lane & 3, r = lane >> 2;
    const int f0 = blockIdx.x * kDetFixedFrames;
    const int nf = min(kDetFixedFrames, dp.n_frames - f0);
    auto lds = [&](int byte) -> double2& { return *reinterpret_cast<double2*>(sm + byte); };

    lds(kDetFixedLdsX + 16 * lane) = det_twiddle(lane, N);
    // group and scale of frame f0 + i in lane i
    const int my_group = (f0 + min(lane, nf - 1)) / dp.frames_per_group;
    const double my_scale = det_scale(N, dp.p_i[my_group]);
    const double norm = det_uniform(det_norm(1 << (dp.m / 2)));
    det_wave_sync();
    const double2 W0 = lds(kDetFixedLdsX), W16 = lds(kDetFixedLdsX + 16 * 16), W32 = lds(kDetFixedLdsX + 32 * 16),
                  W48 = lds(kDetFixedLdsX + 48 * 16);
    const double2 w0 = make_double2(det_uniform(W0.x), det_uniform(W0.y)), w16 = make_double2(det_uniform(W16.x), det_uniform(W16.y)),
                  w32 = make_double2(det_uniform(W32.x), det_uniform(W32.y)), w48 = make_double2(det_uniform(W48.x), det_uniform(W48.y));
    // byte offsets of this lane in the three exchange images (slot = 16 bytes) and in the twiddle table
    const int r0 = r & 1, r1 = (r >> 1) & 1, r2 = (r >> 2) & 1, r3 = r >> 3;
    const int w1 = 16 * (4 * ((r3 << 5) | (r2 << 6) | (r1 << 1) | r0) + a);          // + 256 t
    const int g1 = 16 * (4 * (4 * (r >> 2) + 2 * r0 + r1) + a);                      // + 2048 v + 1024 h
    const int w2 = 16 * (4 * (32 * (r & 3) + 2 * r3 + (r2 ^ r0)) + a);               // + 512 v + 256 h
    const int g2 = 16 * (4 * r + a);                                                 // ^ 64 (v & 1), + 2048 v + 1024 h
    const int w3 = 16 * (130 * a + r);                                               // + 512 v + 256 h
    const int g3 = 16 * lane;                                                        // + 2080 antenna + 1024 half
    const int t4 = kDetFixedLdsX + 128 * (r >> 2), t5 = kDetFixedLdsX + 64 * (r >> 2);   // tw[8 t'], tw[4 t'], t' = (r >> 2) + 4 h
    const int t6 = kDetFixedLdsX + 32 * r, t7 = kDetFixedLdsX + 16 * r;                  // tw[2 w], tw[w], w = r + 16 h

    auto load = [&](Pre& p, int frame) {
        const char* yb = reinterpret_cast<const char*>(dp.Y) + ((size_t)frame * (N * NT) + lane) * sizeof(YT);
#pragma unroll
        for (int j = 0; j < 8; ++j) p.y[j] = *reinterpret_cast<const YT*>(yb + (size_t)j * 16 * NT * sizeof(YT));
        const uint4* tb = reinterpret_cast<const uint4*>(dp.tx_bits) + (size_t)frame * N + lane;
        p.tx[0] = tb[0];
        p.tx[1] = tb[64];
    };

    int errs = 0, run = 0;                                    // of the current run of frames of one group
    auto frame_body = [&](const Pre& cur, int f) {
        double2 x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {                         // position 8 rev4(r) + rev3(j)
            const int t = ((j & 1) << 2) | (j & 2) | (j >> 2);
            x[t] = make_double2((double)cur.y[j].x, (double)cur.y[j].y);
        }
        // stages 1-3
        det_bfly(x[0], x[1], w0); det_bfly(x[2], x[3], w0); det_bfly(x[4], x[5], w0); det_bfly(x[6], x[7], w0);
        det_bfly(x[0], x[2], w0); det_bfly(x[1], x[3], w32); det_bfly(x[4], x[6], w0); det_bfly(x[5], x[7], w32);
        det_bfly(x[0], x[4], w0); det_bfly(x[1], x[5], w16); det_bfly(x[2], x[6], w32); det_bfly(x[3], x[7], w48);
#pragma unroll
        for (int t = 0; t < 8; ++t) lds(w1 + 256 * t) = x[t];
        det_wave_sync();
        // stages 4-5 on positions 32 u + 8 v + t', u = r & 3, t' = (r >> 2) + 4 h: x[4 h + v]
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int v = 0; v < 4; ++v) x[4 * h + v] = lds(g1 + 2048 * v + 1024 * h);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const double2 ta = lds(t4 + 512 * h), tb = lds(t5 + 256 * h), tc = lds(t5 + 256 * h + 512);
            det_bfly(x[4 * h], x[4 * h + 1], ta); det_bfly(x[4 * h + 2], x[4 * h + 3], ta);
            det_bfly(x[4 * h], x[4 * h + 2], tb); det_bfly(x[4 * h + 1], x[4 * h + 3], tc);
        }
        det_wave_sync();
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int v = 0; v < 4; ++v) lds(w2 + 512 * v + 256 * h) = x[4 * h + v];
        det_wave_sync();
        // stages 6-7 on positions 32 v + w, w = r + 16 h
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int v = 0; v < 4; ++v) x[4 * h + v] = lds((g2 ^ (64 * (v & 1))) + 2048 * v + 1024 * h);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const double2 ta = lds(t6 + 512 * h), tb = lds(t7 + 256 * h), tc = lds(t7 + 256 * h + 512);
            det_bfly(x[4 * h], x[4 * h + 1], ta); det_bfly(x[4 * h + 2], x[4 * h + 3], ta);
            det_bfly(x[4 * h], x[4 * h + 2], tb); det_bfly(x[4 * h + 1], x[4 * h + 3], tc);
        }
        det_wave_sync();
        // X = FFT / (N sqrt(Pi)): x[4 h + v] is subcarrier 32 v + 16 h + r of antenna a
        const double scale = det_lane_double(my_scale, f);
        const int group = __builtin_amdgcn_readlane(my_group, f);
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = make_double2(x[i].x * scale, x[i].y * scale);
        if (dp.X_hat) {
            char* xb = reinterpret_cast<char*>(dp.X_hat) + ((size_t)(f0 + f) * (N * NT) + lane) * sizeof(double2);
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int v = 0; v < 4; ++v) *reinterpret_cast<double2*>(xb + 2048 * v + 1024 * h) = x[4 * h + v];
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int v = 0; v < 4; ++v) lds(w3 + 512 * v + 256 * h) = x[4 * h + v];
        det_wave_sync();
        // slicer: subcarriers lane and lane + 64, the four antennas; tx word bb holds bit bb of the four, a byte each
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            uint32_t packed = 0;                              // byte a' = constellation index of antenna a'
#pragma unroll
            for (int aa = 0; aa < NT; ++aa) {
                const double2 v = lds(g3 + 2080 * aa + 1024 * kh);
                const int idx = det_slice(v.x, norm, SIDE) * SIDE + det_slice(v.y, norm, SIDE);
                packed |= (uint32_t)idx << (8 * aa);
            }
            const uint32_t wd[4] = {cur.tx[kh].x, cur.tx[kh].y, cur.tx[kh].z, cur.tx[kh].w};
#pragma unroll
            for (int bb = 0; bb < M; ++bb)                    // bytes are 0 or 1 on both sides: |difference| = mismatch
                errs = (int)__builtin_amdgcn_sad_u8((packed >> bb) & 0x01010101u, wd[bb], (uint32_t)errs);
        }
        det_wave_sync();
        ++run;
        if (f + 1 == nf || __builtin_amdgcn_readlane(my_group, f + 1 < nf ? f + 1 : f) != group) {   // the run ends
            int e = errs;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off);
            if (lane == 0) {
                atomicAdd(reinterpret_cast<unsigned long long*>(dp.err + group), (unsigned long long)e);
                atomicAdd(reinterpret_cast<unsigned long long*>(dp.bits + group), (unsigned long long)(run * (N * M * NT)));
            }
            errs = 0;
            run = 0;
        }
    };

    Pre A, B;
    load(A, f0);
    for (int f = 0; f < nf; f += 2) {
        const bool has_b = f + 1 < nf;
        if (has_b) load(B, f0 + f + 1);
        frame_body(A, f);
        if (!has_b) break;
        if (f + 2 < nf) load(A, f0 + f + 2);
        frame_body(B, f + 1);
    }
}

// the instances; a further shape: its lane map in the kernel, one line here and one in detect_fixed_kernel_for
template __global__ void detect_count_fixed_kernel<false, 7, 4, 4>(DetectParams);
template __global__ void detect_count_fixed_kernel<true, 7, 4, 4>(DetectParams);

static const void* detect_fixed_kernel_for(const DetectParams& dp, bool io32) {
    if (!knobs().detect_fixed) return nullptr;
    if (((uintptr_t)dp.tx_bits & 15) != 0 || ((uintptr_t)dp.Y & (io32 ? 7 : 15)) != 0) return nullptr;
    if (dp.n_sub == 128 && dp.n_t == 4 && dp.m == 4)
        return io32 ? reinterpret_cast<const void*>(detect_count_fixed_kernel<true, 7, 4, 4>)
                    : reinterpret_cast<const void*>(detect_count_fixed_kernel<false, 7, 4, 4>);
    return nullptr;
}

bool detect_geometry(const DetectParams& dp, DetectGeometry* g) {
    int na = dp.n_t < 16 ? dp.n_t : 16;
    auto lds_of = [&](int a) { return sizeof(double2) * ((size_t)a * (dp.n_sub + 1) + dp.n_sub / 2); };
    while (na > 1 && lds_of(na) > 150 * 1024) --na;
    g->na_wg = na;
    g->lds = lds_of(na);
    g->grid = dim3(dp.n_frames * ((dp.n_t + na - 1) / na));
    g->block = dim3(32 * na < 64 ? 64 : 32 * na);
    return g->lds <= 150 * 1024;
}

int launch_detect_count(const DetectParams& dp_in, hipStream_t stream, bool io32) {
    DetectParams dp = dp_in;
    if (const void* fixed = detect_fixed_kernel_for(dp, io32)) {
        dp.na_wg = dp.n_t;
        void* args[] = {&dp};
        const dim3 grid((dp.n_frames + kDetFixedFrames - 1) / kDetFixedFrames), block(64);
        return (int)hipLaunchKernel(fixed, grid, block, args, 0, stream);
    }
    DetectGeometry g;
    if (!detect_geometry(dp, &g)) return -1;
    dp.na_wg = g.na_wg;
    const void* kern = io32 ? reinterpret_cast<const void*>(detect_count_kernel<true>)
                            : reinterpret_cast<const void*>(detect_count_kernel<false>);
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds);
    if (e != hipSuccess) return (int)e;
    if (io32) hipLaunchKernelGGL(detect_count_kernel<true>, g.grid, g.block, g.lds, stream, dp);
    else hipLaunchKernelGGL(detect_count_kernel<false>, g.grid, g.block, g.lds, stream, dp);
    return (int)hipGetLastError();
}

}  // namespace esn
