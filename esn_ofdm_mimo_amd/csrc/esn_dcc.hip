// The LS-MMSE detector with decision-aided cancellation of the transmit amplifier's distortion: a classical receiver
// that knows the amplifier x / sqrt(1 + (|x|/A)^2) of gen_frames_kernel -- one launch, one workgroup per frame, the
// n_iter loop inside it, nothing between the received frame and the counters leaves the chip unless X_hat is asked for:
//   Y_k    = (1/N) FFT_N(y[cp:]) per rx                                 mmse_spectrum   } the operations and order of
//   X0_k   = (H_k^H H_k + No/Pi I)^-1 H_k^H Y_k / sqrt(Pi)              mmse_solve_point} mmse_detect_kernel: bit-identical
//   for it = 1 .. n_iter:
//     S_k   = the grid point nearest X^{it-1}_k                          det_slice, the level table
//     xt_i  = sqrt(Pi) sum_k S_k e^{+2 pi i ik/N}                        conj(FFT(conj S)) with the forward table, as
//                                                                        mmse_equalize_rows_kernel turns X back
//     d_i   = xt_i / sqrt(1 + (|xt_i|/A)^2) - xt_i                       the amplifier expression of gen_frames_kernel
//     D_k   = (1 / (N sqrt(Pi))) sum_i d_i e^{-2 pi i ik/N}
//     X^it_k = X0_k - (H_k^H H_k + No/Pi I)^-1 H_k^H (H_k D_k)           H_k D_k written over the Y image, rows summed in
//                                                                        order of tx, the same mmse_solve_point on it
//   slicer, bit errors and counters of mmse_detect_kernel on X^{n_iter}; err_iter takes the errors of every slicer pass.
// LDS (double2): Y [n_r][N] | X0 [n_t][N] | W [n_t][N] (S -> xt -> d -> D in place) | tw [N/2].  Y keeps the row stride
// N of mmse_spectrum, W the same: the byte count is the ABI's 16 ((n_r + 2 n_t) N + N/2).
// Who touches what: thread k owns column k of Y and X0.  Column k of W (D_k) is read by thread k alone, but the decision
// S_k goes to position rev(k) of W, another thread's column -- so H D is formed for every column first, and the solves
// and the decisions follow behind a barrier.  The amplifier pass takes the positions i <= rev(i) in pairs and stores each
// d at the other's place: the second transform finds its input bit-reversed without a pass of its own.
// Every sum runs in an order the shape decides (FFT stages, rx in the solve, tx in H D): a frame's X and error counts
// are the same alone and in any batch.  The only atomics are the integer counter tails.
// Three waves per SIMD (three frames per CU, as mmse_detect_kernel has them) are asked for: left alone the compiler takes
// 177 VGPRs and two, and two passes then cost 3.8 x that kernel instead of 3.0 (profiles/dcc_time.txt); the bound costs 7
// spilled VGPRs.
#include "esn_common.h"
#include "esn_launch.h"
#include "esn_mmse_solve.h"
#include "esn_ofdm_math.h"

namespace esn {

size_t mmse_dcc_lds_bytes(int n_sub, int n_t, int n_r) {
    return sizeof(double2) * (((size_t)n_r + 2 * (size_t)n_t) * n_sub + n_sub / 2);
}

constexpr int kDccThreads = 256, kDccWaves = kDccThreads / 64;

__global__ __launch_bounds__(kDccThreads, 3) void mmse_dcc_kernel(DccParams dp) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    __shared__ int red[kDccWaves];
    __shared__ int red_it[(DCC_MAX_ITER + 1) * kDccWaves];   // errors of slicer pass `it`, one slot per wave
    __shared__ double lev[32];
    const int N = dp.n_sub, T = N + dp.cp, n_t = dp.n_t, n_r = dp.n_r, m = dp.m, log2n = dp.log2n, n_iter = dp.n_iter;
    double2* Y = reinterpret_cast<double2*>(dsm);          // [n_r][N]: Y, then H D
    double2* X0 = Y + (size_t)n_r * N;                     // [n_t][N]
    double2* W = X0 + (size_t)n_t * N;                     // [n_t][N]
    double2* tw = W + (size_t)n_t * N;                     // [N/2] exp(-2 pi i k / N)
    const int tid = threadIdx.x, nth = blockDim.x;
    const int frame = blockIdx.x, blk = frame / dp.frames_per_group;
    const int side = 1 << (m / 2);
    const double norm = det_norm(side);
    qam_levels(lev, side, norm);                           // read behind the barriers of mmse_spectrum
    mmse_spectrum(Y, tw, dp.y_cp + ((size_t)frame * T + dp.cp) * n_r * 2, N, log2n, n_r);
    const double p_i = dp.p_i[blk], lam = dp.no / p_i, isp = 1.0 / sqrt(p_i);
    const double sp = sqrt(p_i), aclip = dp.a_clip[blk], dsc = det_scale(N, p_i);
    const bool count = dp.tx_bits != nullptr, count_it = count && dp.err_iter != nullptr;
    const uint8_t* tb = count ? dp.tx_bits + (size_t)frame * N * m * n_t : nullptr;
    const double* Hb = dp.H + (size_t)blk * N * n_r * n_t * 2;

    // the slicer pass on X^{it}_k[tx] = (re, im): errors; the last pass writes X_hat, every other leaves conj(S) where
    // the transform wants it
    auto decide = [&](int k, int tx, double re, double im, bool last, int& errs) {
        const int si = det_slice(re, norm, side), sj = det_slice(im, norm, side);
        if (last ? count : count_it) errs += det_bit_errors(si * side + sj, tb + (size_t)k * m * n_t + tx, n_t, m);
        if (!last) {
            const int rv = (int)(__brev((unsigned)k) >> (32 - log2n));
            W[(size_t)tx * N + rv] = make_double2(lev[si], -lev[sj]);
        } else if (dp.X_hat) {
            double* xo = dp.X_hat + (((size_t)frame * N + k) * n_t + tx) * 2;
            xo[0] = re; xo[1] = im;
        }
    };
    // a pass's errors into its row of red_it: every lane of every wave calls it
    auto tally = [&](int it, int errs) {
        if (!count_it) return;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) errs += __shfl_down(errs, off);
        if ((tid & 63) == 0) red_it[it * kDccWaves + (tid >> 6)] = errs;
    };

    int errs = 0;
    for (int k = tid; k < N; k += nth) {
        double2 x[MMSE_NT];
        mmse_solve_point(Hb + (size_t)k * n_r * n_t * 2, Y, N, k, n_t, n_r, lam, x);
#pragma unroll
        for (int tx = 0; tx < MMSE_NT; ++tx) {
            if (tx >= n_t) continue;
            const double re = x[tx].x * isp, im = x[tx].y * isp;
            X0[(size_t)tx * N + k] = make_double2(re, im);
            decide(k, tx, re, im, n_iter == 0, errs);
        }
    }
    tally(0, errs);

    for (int it = 1; it <= n_iter; ++it) {
        __syncthreads();
        ofdm_fft_lds(W, n_t, N, tw, N, log2n);             // conj(N IFFT(S)), natural order
        // ---- the amplifier's distortion of sqrt(Pi) N IFFT(S), scaled for D, each sample to its bit-reversed place
        auto distortion = [&](const double2 v) {
            const double xr = v.x * sp, xi = -v.y * sp;
            const double mag = sqrt(xr * xr + xi * xi) / aclip;
            const double gpa = 1.0 / sqrt(1.0 + mag * mag);
            return make_double2((xr * gpa - xr) * dsc, (xi * gpa - xi) * dsc);
        };
        for (int e = tid; e < n_t << log2n; e += nth) {
            const int i = e & (N - 1);
            const int rv = (int)(__brev((unsigned)i) >> (32 - log2n));
            if (i <= rv) {
                double2* row = W + (size_t)(e >> log2n) * N;
                const double2 a = row[i], b = row[rv];
                row[rv] = distortion(a);
                if (i != rv) row[i] = distortion(b);
            }
        }
        __syncthreads();
        ofdm_fft_lds(W, n_t, N, tw, N, log2n);             // D, natural order
        // ---- H_k D_k over column k of the Y image
        for (int k = tid; k < N; k += nth) {
            const double* hk = Hb + (size_t)k * n_r * n_t * 2;
            double2 d[MMSE_NT];
#pragma unroll
            for (int tx = 0; tx < MMSE_NT; ++tx) d[tx] = tx < n_t ? W[(size_t)tx * N + k] : make_double2(0.0, 0.0);
            for (int rx = 0; rx < n_r; ++rx) {
                double2 acc = make_double2(0.0, 0.0);
#pragma unroll
                for (int tx = 0; tx < MMSE_NT; ++tx) {
                    if (tx >= n_t) continue;
                    const double2 t = cmul(make_double2(hk[((size_t)rx * n_t + tx) * 2], hk[((size_t)rx * n_t + tx) * 2 + 1]),
                                           d[tx]);
                    acc.x += t.x; acc.y += t.y;
                }
                Y[(size_t)rx * N + k] = acc;
            }
        }
        __syncthreads();                                   // every D_k is read: the decisions may take W
        errs = 0;
        for (int k = tid; k < N; k += nth) {
            double2 c[MMSE_NT];
            mmse_solve_point(Hb + (size_t)k * n_r * n_t * 2, Y, N, k, n_t, n_r, lam, c);
#pragma unroll
            for (int tx = 0; tx < MMSE_NT; ++tx) {
                if (tx >= n_t) continue;
                const double2 x0 = X0[(size_t)tx * N + k];
                decide(k, tx, x0.x - c[tx].x, x0.y - c[tx].y, it == n_iter, errs);
            }
        }
        tally(it, errs);
    }
    det_count_tail(count, errs, red, dp.err + blk, dp.bits + blk, N * m * n_t);   // its barrier also covers red_it
    if (count_it && tid <= n_iter) {
        int e = 0;
        for (int w = 0; w < kDccWaves; ++w) e += red_it[tid * kDccWaves + w];
        atomicAdd(reinterpret_cast<unsigned long long*>(dp.err_iter + (size_t)blk * (n_iter + 1) + tid),
                  (unsigned long long)e);
    }
}

int launch_mmse_dcc(const DccParams& dp, hipStream_t stream) {
    if (dp.n_t > MMSE_NT || dp.n_iter < 0 || dp.n_iter > DCC_MAX_ITER) return -1;
    const size_t lds = mmse_dcc_lds_bytes(dp.n_sub, dp.n_t, dp.n_r);
    if (lds > MMSE_LDS_MAX) return -1;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(mmse_dcc_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mmse_dcc_kernel, dim3(dp.n_frames), dim3(kDccThreads), lds, stream, dp);
    return (int)hipGetLastError();
}

}  // namespace esn
