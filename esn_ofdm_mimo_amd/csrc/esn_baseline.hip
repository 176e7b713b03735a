// Baseline equaliser the reference plots the ESN against, float64 / complex128:
//
//   channel_estimate_kernel   per (block, rx): Y_LS = (1/N) FFT(y_LS[cp:]); per tx: LS at the pilot
//       subcarriers sc = tx, tx+n_t, ... (X_LS sparse pattern), linear inter/extrapolation to all N,
//       IFFT truncated to isi taps, diagonal MMSE shrinkage c/(1 + scaler/r_h), DFT back
//       (Demo_MIMO_4x8_Sionna_CDL_ESN_v2.py:358-382, prior :212-214,279)
//   mmse_detect_kernel        per frame: Y = (1/N) FFT(y[cp:]) per rx; per subcarrier
//       X = (H^H H + No/Pi I)^-1 H^H Y / sqrt(Pi)  (:40-45, :444-448); nearest QAM point, natural
//       binary LSB-first bits, error count vs TxBits (:95-103, :451-456)
#include "esn_common.h"
#include "esn_launch.h"
#include "esn_mmse_solve.h"
#include "esn_ofdm_math.h"

namespace esn {

__global__ __launch_bounds__(256) void channel_estimate_kernel(ChanEstParams cp) {
    extern __shared__ __attribute__((aligned(16))) char csm[];
    const int N = cp.n_sub, T = N + cp.cp, n_t = cp.n_t, n_r = cp.n_r, isi = cp.isi, m = cp.m;
    double2* Yf = reinterpret_cast<double2*>(csm);        // [N]  (1/N) FFT of the LS pilot at this rx
    double2* full = Yf + N;                                // [N]  interpolated LS estimate
    double2* hls = full + N;                               // [N / n_t + 1] LS at the pilot subcarriers
    double2* ctd = hls + (N / n_t + 1);                    // [isi] time-domain taps
    double2* tw = ctd + isi;                               // [N/2] exp(-2 pi i k / N)
    const int tid = threadIdx.x, nth = blockDim.x;
    const int blk = blockIdx.x / n_r, rx = blockIdx.x % n_r;
    const double p_i = cp.p_i[blk], sp = sqrt(p_i);
    const int side = 1 << (m / 2);
    const double norm = det_norm(side);
    const double* y = cp.y_ls_cp + ((size_t)blk * T + cp.cp) * n_r * 2 + 2 * rx;
    ofdm_twiddles(tw, N >> 1, N, -1.0);
    for (int i = tid; i < N; i += nth) {
        const int rv = (int)(__brev((unsigned)i) >> (32 - cp.log2n));
        Yf[rv] = make_double2(y[(size_t)i * n_r * 2] / N, y[(size_t)i * n_r * 2 + 1] / N);
    }
    __syncthreads();
    ofdm_fft_lds(Yf, 1, N, tw, N, cp.log2n);
    const int n_p = (N + n_t - 1) / n_t;                   // pilots per tx (sc = tx + n_t i < N)
    // prior: r_h[k] = exp(-k / (cp/9)) / sum_{j<=cp} exp(-j / (cp/9)), k < isi   (driver:212-214,279)
    const double tc = fmax((double)cp.cp / 9.0, 1e-12);
    double rsum = 0.0;
    for (int j = 0; j <= cp.cp; ++j) rsum += exp(-(double)j / tc);
    const double scaler = (cp.no / p_i) / ((double)N / 2.0);
    for (int tx = 0; tx < n_t; ++tx) {
        const int np_tx = (N - tx + n_t - 1) / n_t;
        for (int i = tid; i < np_tx; i += nth) {
            const int sc = tx + n_t * i;
            const int idx = det_bits_index(cp.pilot_bits + ((size_t)blk * N * m + (size_t)sc * m) * n_t + tx, n_t, m);
            const double2 xp = make_double2(det_level(idx / side, side, norm) * sp + 1e-12,
                                            det_level(idx % side, side, norm) * sp);
            hls[i] = cdiv(Yf[sc], xp);
        }
        __syncthreads();
        // linear interpolation with extrapolation beyond the first / last pilot (scipy interp1d)
        for (int k = tid; k < N; k += nth) {
            int i = (k - tx >= 0) ? (k - tx) / n_t : 0;
            if (i > np_tx - 2) i = np_tx - 2;
            if (i < 0) i = 0;
            const double w = ((double)k - (double)(tx + n_t * i)) / (double)n_t;
            const double2 lo = hls[i], hi = (np_tx > 1) ? hls[i + 1] : hls[i];
            full[k] = make_double2(lo.x + w * (hi.x - lo.x), lo.y + w * (hi.y - lo.y));
        }
        __syncthreads();
        if (cp.ls_only) {      // H_LS of the block-fading drivers: the interpolated LS estimate as is (:321-333)
            for (int k = tid; k < N; k += nth) {
                double* ho = cp.H + ((((size_t)blk * N + k) * n_r + rx) * n_t + tx) * 2;
                ho[0] = full[k].x; ho[1] = full[k].y;
            }
            __syncthreads();
            continue;
        }
        // c_LS[j] = (1/N) sum_k full[k] e^{+2 pi i jk/N}, j < isi; then shrink
        if (tid < isi) {
            const double2 a = ofdm_dft_point([&](int k) { return full[k]; }, N, tid, N, 2.0);
            const double rh = exp(-(double)tid / tc) / rsum;
            const double g = 1.0 / (scaler / rh + 1.0);
            ctd[tid] = make_double2(a.x / N * g, a.y / N * g);
        }
        __syncthreads();
        // H[k] = sum_{j<isi} c[j] e^{-2 pi i jk/N}
        for (int k = tid; k < N; k += nth) {
            const double2 h = ofdm_dft_point([&](int j) { return ctd[j]; }, isi, k, N, -2.0);
            double* ho = cp.H + ((((size_t)blk * N + k) * n_r + rx) * n_t + tx) * 2;
            ho[0] = h.x; ho[1] = h.y;
        }
        __syncthreads();
    }
    (void)n_p;
}

__global__ __launch_bounds__(256) void mmse_detect_kernel(MmseParams mp) {
    extern __shared__ __attribute__((aligned(16))) char msm[];
    __shared__ int red[4];
    const int N = mp.n_sub, T = N + mp.cp, n_t = mp.n_t, n_r = mp.n_r, m = mp.m;
    double2* Y = reinterpret_cast<double2*>(msm);          // [n_r][N]
    double2* tw = Y + (size_t)n_r * N;                     // [N/2] exp(-2 pi i k / N)
    const int tid = threadIdx.x, nth = blockDim.x;
    const int frame = blockIdx.x, blk = frame / mp.frames_per_group;
    mmse_spectrum(Y, tw, mp.y_cp + ((size_t)frame * T + mp.cp) * n_r * 2, N, mp.log2n, n_r);
    const double p_i = mp.p_i[blk], lam = mp.zf ? 1e-12 : mp.no / p_i, isp = 1.0 / sqrt(p_i);
    const int side = 1 << (m / 2);
    const double norm = det_norm(side);
    int errs = 0;
    for (int k = tid; k < N; k += nth) {
        double2 x[MMSE_NT];
        mmse_solve_point(mp.H + (((size_t)blk * N + k) * n_r) * n_t * 2, Y, N, k, n_t, n_r, lam, x);
#pragma unroll
        for (int tx = 0; tx < MMSE_NT; ++tx) {
            if (tx >= n_t) continue;
            const double re = x[tx].x * isp, im = x[tx].y * isp;
            if (mp.X_hat) {
                double* xo = mp.X_hat + (((size_t)frame * N + k) * n_t + tx) * 2;
                xo[0] = re; xo[1] = im;
            }
            const int idx = det_slice(re, norm, side) * side + det_slice(im, norm, side);
            errs += det_bit_errors(idx, mp.tx_bits + ((size_t)frame * N * m + (size_t)k * m) * n_t + tx, n_t, m);
        }
    }
    det_count_tail(true, errs, red, mp.err + blk, mp.bits + blk, N * m * n_t);
}

// Perfect-CSI channel: H[k] = sum_j c[j] e^{-2 pi i jk/N} per link (H_true of OFDM_MIMO_2-2_NBF_LDPC.py:273-279)
__global__ __launch_bounds__(256) void taps_to_freq_kernel(TapsFreqParams tp) {
    const int N = tp.n_sub, n_t = tp.n_t, n_r = tp.n_r, isi = tp.isi;
    const size_t total = (size_t)tp.n_blocks * N * n_r * n_t;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int tx = (int)(e % n_t), rx = (int)((e / n_t) % n_r), k = (int)((e / ((size_t)n_t * n_r)) % N);
        const size_t blk = e / ((size_t)n_t * n_r * N);
        const double* c = tp.taps + (((blk * n_r + rx) * n_t + tx) * isi) * 2;
        const double2 h = ofdm_dft_point([&](int j) { return make_double2(c[2 * j], c[2 * j + 1]); }, isi, k, N, -2.0);
        tp.H[2 * e] = h.x; tp.H[2 * e + 1] = h.y;
    }
}

int launch_taps_to_freq(const TapsFreqParams& tp, hipStream_t stream) {
    const size_t total = (size_t)tp.n_blocks * tp.n_sub * tp.n_r * tp.n_t;
    const int blocks = (int)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
    hipLaunchKernelGGL(taps_to_freq_kernel, dim3(blocks), dim3(256), 0, stream, tp);
    return (int)hipGetLastError();
}

// Yf[N], full[N], hls[N / n_t + 1], ctd[isi], tw[N / 2]
size_t channel_estimate_lds_bytes(int n_sub, int n_t, int isi) {
    return sizeof(double2) * ((size_t)2 * n_sub + n_sub / n_t + 1 + isi + n_sub / 2);
}

int launch_channel_estimate(const ChanEstParams& cp, hipStream_t stream) {
    const size_t lds = channel_estimate_lds_bytes(cp.n_sub, cp.n_t, cp.isi);
    if (lds > MMSE_LDS_MAX) return -1;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(channel_estimate_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(channel_estimate_kernel, dim3(cp.n_blocks * cp.n_r), dim3(256), lds, stream, cp);
    return (int)hipGetLastError();
}

int launch_mmse_detect(const MmseParams& mp, hipStream_t stream) {
    if (mp.n_t > MMSE_NT) return -1;
    const size_t lds = sizeof(double2) * ((size_t)mp.n_r * mp.n_sub + mp.n_sub / 2);
    if (lds > MMSE_LDS_MAX) return -1;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(mmse_detect_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mmse_detect_kernel, dim3(mp.n_frames), dim3(256), lds, stream, mp);
    return (int)hipGetLastError();
}

}  // namespace esn
