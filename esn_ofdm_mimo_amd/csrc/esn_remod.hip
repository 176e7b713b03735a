// Decide and re-modulate: the detector tail of esn_detect.hip, then its decisions turned back into the time-domain
// teacher rows a per-symbol re-fit of the read-out needs (decision-directed tracking) -- one launch, one workgroup per
// frame, the spectrum stays in LDS between the two transforms:
//   X     = FFT_N(y) / (N sqrt(Pi))        the operations of detect_count_kernel: X_hat, indices, counters bit-identical
//   idx   = nearest point of the unit-power square QAM grid, X_dec = that point
//   x_t   = N IFFT_N(X_dec) sqrt(Pi)       what the transmitter sent had every decision been right
//   D_hat = [delay zero rows | last cp samples of x_t | x_t], Re/Im interleaved per antenna: the teacher of
//           esn_harvest_batch (helper_mimo_esn_generic.py:26-38)
// float64 throughout, radix-2 in LDS.  The forward transform is decimation in time on the bit-reversed frame, the
// inverse one decimation in frequency on the natural-order spectrum in place -- its output is in bit-reversed order,
// which the row writer undoes -- so no second buffer and no reordering pass is needed.
#include "esn_common.h"
#include "esn_launch.h"
#include "esn_ofdm_math.h"

namespace esn {

// the butterfly of the inverse stage: undoes det_bfly up to the factor 2 (N over all stages, the N of N IFFT)
__device__ __forceinline__ void remod_ibfly(double2& a, double2& c, const double2 w) {      // w = exp(-2 pi i j / 2^s)
    const double dr = a.x - c.x, di = a.y - c.y;
    a = make_double2(a.x + c.x, a.y + c.y);
    c = make_double2(dr * w.x + di * w.y, di * w.x - dr * w.y);                             // (a - c) conj(w)
}

// One workgroup per frame (per chunk of antennas where LDS is short), 32 threads per tx antenna, the launch geometry
// and LDS layout of detect_count_kernel.  A frame's outputs depend on its own rows, tx bits and group only.
__global__ __launch_bounds__(512) void detect_remod_kernel(RemodParams rp) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    const DetectParams& dp = rp.d;
    const int N = dp.n_sub, n_t = dp.n_t, tid = threadIdx.x, half = N >> 1;
    const int nthr = blockDim.x;
    const int na_max = dp.na_wg;                             // antennas per workgroup
    const int n_chunks = (n_t + na_max - 1) / na_max;
    const int ld = N + 1;                                    // row pad: stage strides are powers of two
    double2* buf = reinterpret_cast<double2*>(dsm);          // [na][ld]
    double2* tw = buf + (size_t)na_max * ld;                 // [N/2]  exp(-2 pi i k / N)
    __shared__ int red[8];
    const int frame = blockIdx.x / n_chunks;
    const int a0 = (blockIdx.x - frame * n_chunks) * na_max;
    const int na = (n_t - a0 < na_max) ? n_t - a0 : na_max;
    const int group = frame / dp.frames_per_group;
    const double2* y = reinterpret_cast<const double2*>(dp.Y) + (size_t)frame * N * n_t;
    const double p_i_g = dp.p_i[group];
    ofdm_twiddles(tw, half, N, -1.0);
    for (int i = tid; i < N * na; i += nthr) {               // bit-reversed load, element i = (row, antenna)
        const int row = i / na, ant = i - row * na;
        const int rv = (int)(__brev((unsigned)row) >> (32 - dp.log2n));
        buf[ant * ld + rv] = y[(size_t)row * n_t + a0 + ant];
    }
    __syncthreads();
    // ---- forward: the transform of detect_count_kernel
    ofdm_fft_lds(buf, na, ld, tw, N, dp.log2n);

    // ---- slice: X_hat, counters and decided bits as the tail gives them; the decision replaces X in place
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
        const int ir = det_slice(re, norm, side), ii = det_slice(im, norm, side);
        const int idx = ir * side + ii;
        const size_t bit0 = ((size_t)frame * N + k) * dp.m * n_t + ant;      // bit bb of this element: + bb n_t
        if (dp.tx_bits) errs += det_bit_errors(idx, dp.tx_bits + bit0, n_t, dp.m);
        if (rp.dec_bits)
            for (int bb = 0; bb < dp.m; ++bb) rp.dec_bits[bit0 + (size_t)bb * n_t] = (uint8_t)((idx >> bb) & 1);
        buf[(ant - a0) * ld + k] = make_double2(det_level(ir, side, norm), det_level(ii, side, norm));
    }
    det_count_tail(dp.tx_bits != nullptr, errs, red, dp.err + group, dp.bits + group, N * dp.m * na);

    // ---- inverse: decimation in frequency, stages log2n .. 1, natural order in, bit-reversed order out; the unpaired
    // stage of an odd count goes first, the others two at a time on the same four points as the forward pass; 32
    // threads per antenna
    const int sub = tid & 31, av = tid >> 5;
    double2* b = buf + (size_t)(av < na ? av : 0) * ld;
    const int n_quarter = av < na ? N >> 2 : 0, n_half = av < na ? half : 0;
    int s = dp.log2n;
    if (s & 1) {
        for (int t = sub; t < n_half; t += 32) {
            const OfdmPair p = ofdm_pair(t, s, N);
            double2 a = b[p.base], c = b[p.base + p.hm];
            remod_ibfly(a, c, tw[p.k]);
            b[p.base] = a; b[p.base + p.hm] = c;
        }
        __syncthreads();
        --s;
    }
    for (s -= 1; s >= 1; s -= 2) {                           // stages s+1, then s
        for (int t = sub; t < n_quarter; t += 32) {
            const OfdmQuad q = ofdm_quad(t, s, N);
            double2 p0 = b[q.base], p1 = b[q.base + q.hm], p2 = b[q.base + 2 * q.hm], p3 = b[q.base + 3 * q.hm];
            remod_ibfly(p0, p2, tw[q.k2]);
            remod_ibfly(p1, p3, tw[q.k3]);
            const double2 w1 = tw[q.k1];
            remod_ibfly(p0, p1, w1);
            remod_ibfly(p2, p3, w1);
            b[q.base] = p0; b[q.base + q.hm] = p1; b[q.base + 2 * q.hm] = p2; b[q.base + 3 * q.hm] = p3;
        }
        __syncthreads();
    }

    // ---- teacher rows: thread = (row r0 + i step, antenna), a row's antennas in neighbouring lanes (16 bytes each)
    const double amp = sqrt(p_i_g);
    const int rows = rp.delay + rp.cp + N;
    const int ant = tid % na, step = nthr / na;              // (threads past step * na, in a short last chunk, idle)
    double2* dh = reinterpret_cast<double2*>(rp.D_hat) + (size_t)frame * rows * n_t + a0 + ant;
    for (int r = tid < step * na ? tid / na : rows; r < rows; r += step) {
        double2 v = make_double2(0.0, 0.0);
        if (r >= rp.delay) {
            int n = r - rp.delay - rp.cp;                    // sample of x_t; the prefix is its last cp samples
            if (n < 0) n += N;
            const int rv = (int)(__brev((unsigned)n) >> (32 - dp.log2n));
            const double2 x = buf[ant * ld + rv];
            v = make_double2(x.x * amp, x.y * amp);
        }
        dh[(size_t)r * n_t] = v;
    }
}

int launch_detect_remod(const RemodParams& rp_in, hipStream_t stream) {
    RemodParams rp = rp_in;
    DetectGeometry g;
    if (!detect_geometry(rp.d, &g)) return -1;
    rp.d.na_wg = g.na_wg;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(detect_remod_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(detect_remod_kernel, g.grid, g.block, g.lds, stream, rp);
    return (int)hipGetLastError();
}

}  // namespace esn
