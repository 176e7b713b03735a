// The baseline's equaliser with its output back in the time domain: the input rows of an ESN that stands behind the
// LS-MMSE equaliser instead of beside it -- one launch, one workgroup per frame, the spectrum never leaves the chip:
//   Y_k   = (1/N) FFT_N(y[cp:]) per rx                                  mmse_spectrum   } the operations and order of
//   X_k   = (H_k^H H_k + No/Pi I)^-1 H_k^H Y_k / sqrt(Pi)               mmse_solve_point} mmse_detect_kernel: X_hat
//                                                                                         is bit-identical
//   z     = sqrt(Pi) N IFFT_N(X) per tx      the inverse transform and scaling of detect_remod_kernel's teacher
//   U_eq  = [last cp samples of z | z | pad zero rows], Re/Im interleaved per antenna: the input rows of
//           esn_predict_batch / esn_harvest_batch at n_in = 2 n_t
// float64 throughout; the float32 instance rounds at the store.  Thread k reads column k of Y [n_r][N] and then writes
// conj(X_k) into the same column of the first n_t rows (no other thread touches that column, so X takes the place of
// the Y image without a second buffer); behind a barrier the rows are put into bit-reversed order in place and
// ofdm_fft_lds runs once more with the forward table: N IFFT(X) = conj(FFT(conj X)).  No atomics, no counters: a
// frame's outputs depend on its own rows, its group's H and Pi only.
// LDS: 16 (max(n_r, n_t) N + N/2) bytes, at most MMSE_LDS_MAX.
#include "esn_common.h"
#include "esn_launch.h"
#include "esn_mmse_solve.h"
#include "esn_ofdm_math.h"

namespace esn {

size_t equalize_rows_lds_bytes(int n_sub, int n_t, int n_r) {
    return sizeof(double2) * ((size_t)(n_r > n_t ? n_r : n_t) * n_sub + n_sub / 2);
}

__device__ __forceinline__ void eq_store(double* o, double re, double im) {
    *reinterpret_cast<double2*>(o) = make_double2(re, im);
}
__device__ __forceinline__ void eq_store(float* o, double re, double im) {
    *reinterpret_cast<float2*>(o) = make_float2((float)re, (float)im);
}

template <typename OutT>
__global__ __launch_bounds__(256) void mmse_equalize_rows_kernel(EqRowsParams ep) {
    extern __shared__ __attribute__((aligned(16))) char esm[];
    const int N = ep.n_sub, T = N + ep.cp, n_t = ep.n_t, n_r = ep.n_r, log2n = ep.log2n;
    double2* Y = reinterpret_cast<double2*>(esm);          // [max(n_r, n_t)][N]: Y, then conj(X) in rows [0, n_t)
    double2* tw = Y + (size_t)(n_r > n_t ? n_r : n_t) * N; // [N/2] exp(-2 pi i k / N)
    const int tid = threadIdx.x, nth = blockDim.x;
    const int frame = blockIdx.x, blk = frame / ep.frames_per_group;
    mmse_spectrum(Y, tw, ep.y_cp + ((size_t)frame * T + ep.cp) * n_r * 2, N, log2n, n_r);
    const double p_i = ep.p_i[blk], lam = ep.no / p_i, isp = 1.0 / sqrt(p_i);
    for (int k = tid; k < N; k += nth) {
        double2 x[MMSE_NT];
        mmse_solve_point(ep.H + (((size_t)blk * N + k) * n_r) * n_t * 2, Y, N, k, n_t, n_r, lam, x);
#pragma unroll
        for (int tx = 0; tx < MMSE_NT; ++tx) {
            if (tx >= n_t) continue;
            const double re = x[tx].x * isp, im = x[tx].y * isp;
            if (ep.X_hat) {
                double* xo = ep.X_hat + (((size_t)frame * N + k) * n_t + tx) * 2;
                xo[0] = re; xo[1] = im;
            }
            Y[(size_t)tx * N + k] = make_double2(re, -im);
        }
    }
    __syncthreads();
    // ---- rows [0, n_t) into bit-reversed order: element i < rev(i) changes places with rev(i)
    for (int e = tid; e < n_t << log2n; e += nth) {
        const int i = e & (N - 1);
        const int rv = (int)(__brev((unsigned)i) >> (32 - log2n));
        if (i < rv) {
            double2* row = Y + (size_t)(e >> log2n) * N;
            const double2 a = row[i], b = row[rv];
            row[i] = b; row[rv] = a;
        }
    }
    __syncthreads();
    ofdm_fft_lds(Y, n_t, N, tw, N, log2n);                 // conj(N IFFT(X)), natural order
    // ---- rows: element e = (row, antenna), a row's antennas in neighbouring lanes
    const double amp = sqrt(p_i);
    const int live = ep.cp + N, rows = live + ep.pad;
    OutT* out = static_cast<OutT*>(ep.U_eq) + (size_t)frame * rows * n_t * 2;
    for (int e = tid; e < rows * n_t; e += nth) {
        const int r = e / n_t, tx = e - r * n_t;
        double re = 0.0, im = 0.0;
        if (r < live) {
            int n = r - ep.cp;                             // sample of z; the prefix is its last cp samples
            if (n < 0) n += N;
            const double2 z = Y[(size_t)tx * N + n];
            re = z.x * amp; im = -z.y * amp;
        }
        eq_store(out + (size_t)e * 2, re, im);
    }
}

int launch_equalize_rows(const EqRowsParams& ep, hipStream_t stream, bool io32) {
    if (ep.n_t > MMSE_NT) return -1;
    const size_t lds = equalize_rows_lds_bytes(ep.n_sub, ep.n_t, ep.n_r);
    if (lds > MMSE_LDS_MAX) return -1;
    const void* fn = io32 ? reinterpret_cast<const void*>(mmse_equalize_rows_kernel<float>)
                          : reinterpret_cast<const void*>(mmse_equalize_rows_kernel<double>);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    if (io32) hipLaunchKernelGGL(mmse_equalize_rows_kernel<float>, dim3(ep.n_frames), dim3(256), lds, stream, ep);
    else hipLaunchKernelGGL(mmse_equalize_rows_kernel<double>, dim3(ep.n_frames), dim3(256), lds, stream, ep);
    return (int)hipGetLastError();
}

}  // namespace esn
