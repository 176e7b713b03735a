// Ensemble detector tail: K members' time-domain outputs Y [K][B][N][2 n_t] (member-major: slab k is what member k's
// predict wrote) are combined per element
//   acc = w[g][0] y_0;  acc = acc + w[g][k] y_k,  k = 1 .. K-1 in this order, every product and sum rounded on its own
// (float members widened to double first; w = 1/K each without a weight table) and acc goes through the tail of
// detect_count_kernel (esn_detect.hip): ofdm_fft_lds on bit-reversed rows, det_scale, det_slice, det_bit_errors,
// det_count_tail -- the same butterflies on the same operands, so counts and X_hat are bitwise those of
// esn_detect_count on the summed Y, and with K = 1 (weight 1.0) those of esn_detect_count on the slab itself.
// One FFT per frame and antenna whatever K is: the kernel is a stream of K |Y| bytes with one LDS transform behind it.
#include "esn_common.h"
#include "esn_launch.h"
#include "esn_ofdm_math.h"

namespace esn {

constexpr int kEnsUnroll = 4;                                 // members whose loads are in flight together

// the 16-byte unit a lane loads: one complex double, or two complex floats
template <bool IO32> struct EnsUnit;
template <> struct EnsUnit<false> {
    using type = double2;
    static constexpr int elems = 1;
    static __device__ __forceinline__ double2 get(const double2& u, int) { return u; }
};
template <> struct EnsUnit<true> {
    using type = float4;
    static constexpr int elems = 2;
    static __device__ __forceinline__ double2 get(const float4& u, int j) {
        return j ? make_double2((double)u.z, (double)u.w) : make_double2((double)u.x, (double)u.y);
    }
};

__device__ __forceinline__ double2 ens_first(double w, double2 y) {
    return make_double2(__dmul_rn(w, y.x), __dmul_rn(w, y.y));
}
__device__ __forceinline__ double2 ens_next(double2 acc, double w, double2 y) {
    return make_double2(__dadd_rn(acc.x, __dmul_rn(w, y.x)), __dadd_rn(acc.y, __dmul_rn(w, y.y)));
}
__device__ __forceinline__ double ens_weight(const EnsParams& ep, int group, int k) {
    return ep.weights ? ep.weights[(size_t)group * ep.n_members + k] : 1.0 / (double)ep.n_members;
}
__device__ __forceinline__ int ens_rev(int row, int log2n) { return (int)(__brev((unsigned)row) >> (32 - log2n)); }

// One workgroup per (frame, chunk of antennas), 32 threads per antenna: the geometry of the generic tail.
// MEMBERS: member_err is asked for -- every member is also transformed and sliced on its own, through a second row
// buffer, one member after the other; its slab is still read once (the element feeds acc and the member's row).
template <bool IO32, bool MEMBERS>
__global__ __launch_bounds__(512) void detect_count_ens_kernel(EnsParams ep) {
    extern __shared__ __attribute__((aligned(16))) char esm[];
    const DetectParams& dp = ep.d;
    const int N = dp.n_sub, n_t = dp.n_t, tid = threadIdx.x, nthr = blockDim.x, K = ep.n_members;
    const int na_max = dp.na_wg;
    const int n_chunks = (n_t + na_max - 1) / na_max;
    const int ld = N + 1;
    double2* buf = reinterpret_cast<double2*>(esm);          // [na_max][ld]  the combination
    double2* tw = buf + (size_t)na_max * ld;                 // [N/2]
    double2* mbuf = tw + (N >> 1);                           // [na_max][ld]  one member (MEMBERS)
    __shared__ int red[16];
    const int frame = blockIdx.x / n_chunks;
    const int a0 = (blockIdx.x - frame * n_chunks) * na_max;
    const int na = (n_t - a0 < na_max) ? n_t - a0 : na_max;
    const size_t fsz = (size_t)N * n_t;                      // complex elements of a frame
    const size_t slab = (size_t)dp.n_frames * fsz;           // ... of a member
    using Y1 = typename std::conditional<IO32, float2, double2>::type;
    auto widen = [](const Y1& v) { return make_double2((double)v.x, (double)v.y); };
    const int side = 1 << (dp.m / 2);
    const double norm = det_norm(side);
    ofdm_twiddles(tw, N >> 1, N, -1.0);           // (the barrier behind the loads orders it before its first reader)
    const int group = frame / dp.frames_per_group;
    const Y1* y1 = reinterpret_cast<const Y1*>(dp.Y) + (size_t)frame * fsz;
    const double p_i_g = dp.p_i[group];

    if constexpr (!MEMBERS) {
        using U = EnsUnit<IO32>;
        using UT = typename U::type;
        // a whole frame in 16-byte units, two units of kEnsUnroll members in flight per lane
        if (na == n_t && (((uintptr_t)dp.Y | (slab * sizeof(Y1)) | (fsz * sizeof(Y1))) & 15) == 0) {
            const UT* yu = reinterpret_cast<const UT*>(y1);
            const size_t slab_u = slab / U::elems;
            const int units = (int)(fsz / U::elems);
            for (int u0 = tid; u0 < units; u0 += 2 * nthr) {
                const int u1 = u0 + nthr;
                const bool two = u1 < units;
                double2 acc[2][U::elems];
                for (int k0 = 0; k0 < K; k0 += kEnsUnroll) {
                    UT v[2][kEnsUnroll] = {};
#pragma unroll
                    for (int j = 0; j < kEnsUnroll; ++j) {
                        if (k0 + j >= K) break;                               // (uniform)
                        v[0][j] = yu[(size_t)(k0 + j) * slab_u + u0];
                        v[1][j] = yu[(size_t)(k0 + j) * slab_u + (two ? u1 : u0)];
                    }
#pragma unroll
                    for (int j = 0; j < kEnsUnroll; ++j) {
                        if (k0 + j < K) {
                            const double w = ens_weight(ep, group, k0 + j);
#pragma unroll
                            for (int h = 0; h < 2; ++h)
#pragma unroll
                                for (int c = 0; c < U::elems; ++c)
                                    acc[h][c] = (k0 + j == 0) ? ens_first(w, U::get(v[h][j], c))
                                                              : ens_next(acc[h][c], w, U::get(v[h][j], c));
                        }
                    }
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (h == 1 && !two) break;
#pragma unroll
                    for (int c = 0; c < U::elems; ++c) {
                        const int e = (h ? u1 : u0) * U::elems + c, row = e / n_t, ant = e - row * n_t;
                        buf[ant * ld + ens_rev(row, dp.log2n)] = acc[h][c];
                    }
                }
            }
        } else {                                             // element by element: antenna chunks, odd alignments
            for (int i = tid; i < N * na; i += nthr) {
                const int row = i / na, ant = i - row * na;
                const size_t off = (size_t)row * n_t + a0 + ant;
                double2 acc = make_double2(0.0, 0.0);
                for (int k0 = 0; k0 < K; k0 += kEnsUnroll) {
                    Y1 v[kEnsUnroll] = {};
#pragma unroll
                    for (int j = 0; j < kEnsUnroll; ++j)
                        if (k0 + j < K) v[j] = y1[(size_t)(k0 + j) * slab + off];
#pragma unroll
                    for (int j = 0; j < kEnsUnroll; ++j)
                        if (k0 + j < K) {
                            const double w = ens_weight(ep, group, k0 + j);
                            acc = (k0 + j == 0) ? ens_first(w, widen(v[j])) : ens_next(acc, w, widen(v[j]));
                        }
                }
                buf[ant * ld + ens_rev(row, dp.log2n)] = acc;
            }
        }
    }

    const double scale = det_scale(N, p_i_g);
    // spectrum of `b` -> indices -> this thread's bit errors; X_hat only for the combination
    auto slice_count = [&](const double2* b, bool store) {
        int errs = 0;
        for (int e = tid; e < N * na; e += nthr) {           // element e = (subcarrier k, antenna), antenna fastest
            const int k = e / na, ant = a0 + e - k * na;
            const double2 v = b[(ant - a0) * ld + k];
            const double re = v.x * scale, im = v.y * scale;
            if (store && dp.X_hat)
                reinterpret_cast<double2*>(dp.X_hat)[((size_t)frame * N + k) * n_t + ant] = make_double2(re, im);
            const int idx = det_slice(re, norm, side) * side + det_slice(im, norm, side);
            errs += det_bit_errors(idx, dp.tx_bits + ((size_t)frame * N + k) * dp.m * n_t + ant, n_t, dp.m);
        }
        return errs;
    };

    if constexpr (MEMBERS) {
        for (int k = 0; k < K; ++k) {
            const double w = ens_weight(ep, group, k);
            for (int i = tid; i < N * na; i += nthr) {       // element i is this thread's in every pass
                const int row = i / na, ant = i - row * na;
                const double2 y = widen(y1[(size_t)k * slab + (size_t)row * n_t + a0 + ant]);
                const int pos = ant * ld + ens_rev(row, dp.log2n);
                mbuf[pos] = y;
                buf[pos] = k ? ens_next(buf[pos], w, y) : ens_first(w, y);
            }
            __syncthreads();
            ofdm_fft_lds(mbuf, na, ld, tw, N, dp.log2n);
            const int errs = slice_count(mbuf, false);
            // the member's errors into member_err[group][k].  det_count_tail always adds to both counters: with 0 bits
            // it issues an atomic add of zero to the group's bit counter, K per frame, which changes nothing
            det_count_tail(true, errs, red, ep.member_err + (size_t)group * K + k, dp.bits + group, 0);
        }
    } else {
        __syncthreads();
    }
    ofdm_fft_lds(buf, na, ld, tw, N, dp.log2n);
    const int errs = slice_count(buf, true);
    det_count_tail(true, errs, red, dp.err + group, dp.bits + group, N * dp.m * na);
}

// the geometry of the generic tail (detect_geometry) with, for member_err, the second row buffer
static bool ens_geometry(const EnsParams& ep, DetectGeometry* g) {
    const DetectParams& dp = ep.d;
    const int bufs = ep.member_err ? 2 : 1;
    int na = dp.n_t < 16 ? dp.n_t : 16;
    auto lds_of = [&](int a) { return sizeof(double2) * ((size_t)bufs * a * (dp.n_sub + 1) + dp.n_sub / 2); };
    while (na > 1 && lds_of(na) > 150 * 1024) --na;
    g->na_wg = na;
    g->lds = lds_of(na);
    g->grid = dim3(dp.n_frames * ((dp.n_t + na - 1) / na));
    g->block = dim3(32 * na < 64 ? 64 : 32 * na);
    return g->lds <= 150 * 1024;
}

template <bool IO32, bool MEMBERS>
static int launch_ens(const EnsParams& ep, const DetectGeometry& g, hipStream_t stream) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(detect_count_ens_kernel<IO32, MEMBERS>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((detect_count_ens_kernel<IO32, MEMBERS>), g.grid, g.block, g.lds, stream, ep);
    return (int)hipGetLastError();
}

int launch_detect_count_ens(const EnsParams& ep_in, hipStream_t stream, bool io32) {
    EnsParams ep = ep_in;
    DetectGeometry g;
    if (!ens_geometry(ep, &g)) return -1;
    ep.d.na_wg = g.na_wg;
    if (ep.member_err) return io32 ? launch_ens<true, true>(ep, g, stream) : launch_ens<false, true>(ep, g, stream);
    return io32 ? launch_ens<true, false>(ep, g, stream) : launch_ens<false, false>(ep, g, stream);
}

}  // namespace esn
