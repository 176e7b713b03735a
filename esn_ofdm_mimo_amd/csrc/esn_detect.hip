// Fused detector tail, one workgroup per frame, one wave per tx antenna:
//   x[n] = Y[frame][n][2tx] + j Y[frame][n][2tx+1]            (driver :47-58, delay offset 0)
//   X    = FFT_N(x) / (N sqrt(Pi))                             (driver :439-441)
//   idx  = nearest point of the unit-power square QAM grid     (driver :17-28, :95-103)
//   bits = natural binary of idx, LSB first; errors vs TxBits  (driver :30-32, :451-456)
// float64 throughout, radix-2 FFT in LDS.
#include "esn_common.h"
#include "esn_launch.h"

namespace esn {


// One workgroup per frame, 32 threads per tx antenna (n_t <= 16): the frame's rows are read once,
// fully coalesced (a row is n_t complex doubles), the twiddles come from one table per workgroup
// (same sincospi arguments as the reference order).  The radix-2 stages are taken two at a time
// on four points in registers -- the same butterflies in the same order, so the spectrum is
// bit-identical to the plain radix-2 loop, with half the LDS round trips and barriers.
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
    for (int k = tid; k < half; k += nthr) {
        double sn, cs;
        sincospi(-2.0 * (double)k / (double)N, &sn, &cs);
        tw[k] = make_double2(cs, sn);
    }
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
    const int lane = tid & 63, wv = tid >> 6;
    const int sub = tid & 31, av = tid >> 5;                 // 32 threads per antenna
    double2* b = buf + (size_t)av * ld;
    const int quarter = N >> 2;
    auto bfly = [](double2& a, double2& c, const double2 w) {
        const double tr = c.x * w.x - c.y * w.y, ti = c.x * w.y + c.y * w.x;
        const double2 a0 = a;
        a = make_double2(a0.x + tr, a0.y + ti);
        c = make_double2(a0.x - tr, a0.y - ti);
    };
    int s = 1;
    for (; s + 1 <= dp.log2n; s += 2) {                      // stages s and s+1 on {base, +hm, +2hm, +3hm}
        const int hm = 1 << (s - 1);
        for (int t = sub; t < (av < na ? quarter : 0); t += 32) {
            const int j = t & (hm - 1);
            const int base = ((t >> (s - 1)) << (s + 1)) + j;
            double2 p0 = b[base], p1 = b[base + hm], p2 = b[base + 2 * hm], p3 = b[base + 3 * hm];
            const double2 w1 = tw[j * (N >> s)];             // exp(-2 pi i j / 2^s)
            bfly(p0, p1, w1);
            bfly(p2, p3, w1);
            const int ts2 = N >> (s + 1);
            bfly(p0, p2, tw[j * ts2]);                       // exp(-2 pi i j / 2^(s+1))
            bfly(p1, p3, tw[(j + hm) * ts2]);
            b[base] = p0; b[base + hm] = p1; b[base + 2 * hm] = p2; b[base + 3 * hm] = p3;
        }
        __syncthreads();
    }
    if (s <= dp.log2n) {                                     // odd number of stages: the last one alone
        const int hm = 1 << (s - 1), tstep = N >> s;
        for (int t = sub; t < (av < na ? half : 0); t += 32) {
            const int j = t & (hm - 1);
            const int base = ((t >> (s - 1)) << s) + j;
            double2 a = b[base], c = b[base + hm];
            bfly(a, c, tw[j * tstep]);
            b[base] = a; b[base + hm] = c;
        }
        __syncthreads();
    }

    const int side = 1 << (dp.m / 2);
    const double norm = sqrt(2.0 * (double)(side * side - 1) / 3.0);
    const double scale = 1.0 / ((double)N * sqrt(p_i_g));
    int errs = 0;
    for (int e = tid; e < N * na; e += nthr) {               // element e = (subcarrier k, antenna), antenna fastest
        const int k = e / na, ant = a0 + e - k * na;
        const double2 v = buf[(ant - a0) * ld + k];
        const double re = v.x * scale, im = v.y * scale;
        if (dp.X_hat)
            reinterpret_cast<double2*>(dp.X_hat)[((size_t)frame * N + k) * n_t + ant] = make_double2(re, im);
        int i = (int)rint((re * norm + (double)(side - 1)) * 0.5);
        int j = (int)rint((im * norm + (double)(side - 1)) * 0.5);
        i = min(max(i, 0), side - 1);
        j = min(max(j, 0), side - 1);
        const int idx = i * side + j;
        if (tx_pre) {                                        // byte bb n_t + ant of the subcarrier's 16
            const int q = (e - tid) / nthr;
            uint4 w = txw[0];
#pragma unroll
            for (int qq = 1; qq < TXP; ++qq) if (q == qq) w = txw[qq];
            const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) errs += (int)(((uint32_t)(idx >> bb) & 1u) != ((wd[bb] >> (8 * ant)) & 0xffu));
        } else {
            const uint8_t* tb = dp.tx_bits + ((size_t)frame * N + k) * dp.m * n_t + ant;
            for (int bb = 0; bb < dp.m; ++bb) errs += (((idx >> bb) & 1) != (int)tb[(size_t)bb * n_t]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) errs += __shfl_down(errs, off);
    const int nwv = (nthr + 63) >> 6;
    if (lane == 0) red[wv] = errs;
    __syncthreads();
    if (tid == 0) {
        int e = 0;
        for (int w = 0; w < nwv; ++w) e += red[w];
        atomicAdd(reinterpret_cast<unsigned long long*>(dp.err + group), (unsigned long long)e);
        atomicAdd(reinterpret_cast<unsigned long long*>(dp.bits + group), (unsigned long long)(N * dp.m * na));
    }
}

int launch_detect_count(const DetectParams& dp_in, hipStream_t stream, bool io32) {
    DetectParams dp = dp_in;
    int na = dp.n_t < 16 ? dp.n_t : 16;                      // antennas per workgroup
    auto lds_of = [&](int a) { return sizeof(double2) * ((size_t)a * (dp.n_sub + 1) + dp.n_sub / 2); };
    while (na > 1 && lds_of(na) > 150 * 1024) --na;
    const size_t lds = lds_of(na);
    if (lds > 150 * 1024) return -1;
    const int n_chunks = (dp.n_t + na - 1) / na;
    dp.na_wg = na;
    const void* kern = io32 ? reinterpret_cast<const void*>(detect_count_kernel<true>)
                            : reinterpret_cast<const void*>(detect_count_kernel<false>);
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    const dim3 grid(dp.n_frames * n_chunks), block(32 * na < 64 ? 64 : 32 * na);
    if (io32) hipLaunchKernelGGL(detect_count_kernel<true>, grid, block, lds, stream, dp);
    else hipLaunchKernelGGL(detect_count_kernel<false>, grid, block, lds, stream, dp);
    return (int)hipGetLastError();
}

}  // namespace esn
