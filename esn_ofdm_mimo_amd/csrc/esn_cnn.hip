// Windowed CNN (include/esn_hip.h: esn_cnn_train / esn_cnn_predict): Conv1d -> ReLU -> Conv1d -> ReLU -> Conv1d of one odd
// kernel size k over the whole scaled sequence, zero padded by p = (k - 1) / 2 rows, trained per group by `epochs`
// full-batch Adam steps on the mean squared error -- the reference's CNNModel and its training loop
// (system_model_2_all_comparision.py:14-27, :93-113).
//
// A layer is a matrix product.  Its input x [T][c_in] is kept with p zero rows before and after it, xp [(T + 2 p)][c_in],
// so the k c_in values row t reads are the contiguous view xp[t c_in .. (t + k) c_in): the windowed FNN's trick with the
// window k.  The parameters of a layer are kept as P [c_out][K + 1], K = k c_in, P[o][j c_in + i] = W[o][i][j] and
// P[o][K] = b[o]: the bias is one more column, fed by a constant 1.  With that
//   forward       z [T x c_out]      = [xp-view | 1] [T x (K + 1)] . P^T
//   input grad.   dx [T x c_in]      = dzp-view [T x k c_out] . P', dzp the output gradient with p zero rows around it and
//                                      P'[j' c_out + o][i] = W[o][i][k - 1 - j']
//   weight grad.  dP [c_out x (K + 1)] = dz^T [c_out x T] . [xp-view | 1]
// are plain products, all on v_mfma_f64_16x16x4_f64 (A[l % 16][l / 16], B[l / 16][l % 16], C register i: row
// 4 i + l / 16, column l % 16), for all three layers (the forward and the weight-gradient product are in
// esn_f64_strip.h, which the LSTM's training shares): a wave takes a strip of CNN_NB tiles that share the A operand,
// operands straight from memory.  Sums run over the inner index in ascending groups of four, whatever wave takes the
// strip: every sum's order depends on the shape alone.
//
// cnn_train_kernel    one workgroup of 512 threads per group, one launch for all epochs, float64.  Nothing of a group
//   fits on chip beside the rest (the middle layer's weights alone are 80 KB, its activations at T = 1024 512 KB), so a
//   group's P, Adam's moments, the padded activations and the padded gradients live in its part of the caller's workspace
//   (cnn_ws), which only this workgroup touches: the L1 / L2 hold what is hot, workgroup barriers order the phases.  The
//   zero rows are written once, the moments are never read in the first epoch: the workspace needs no zeroing.
//   An epoch: three forwards (the last writes dz3 = 2 (ys - Ds) / (|R| n_out), zero before `transient`, and each lane's
//   part of the loss), two input gradients (masked by the ReLU), then the weight gradients of all three layers, whose
//   accumulator lanes own the parameters and take the Adam step at once.  The loss: lanes by xor-shuffles, then the
//   eight waves in order.  No atomics, nothing leaves the workgroup: a group is bitwise the same alone and in any batch.
//   A parameter whose gradient is exactly 0 in every epoch keeps m = v = 0 and comes out bitwise as it went in.
// cnn_predict_kernel  the same forward functions, a workgroup per frame (at most CNN_PRED_WGS workgroups take the frames
//   in turn), the frame's group's parameters re-laid into the workgroup's scratch, activations there too.
#include "esn_common.h"
#include "esn_f64_strip.h"
#include "esn_launch.h"

namespace esn {

constexpr int CNN_PRED_WGS = 512;              // workgroups (and scratch regions) of a prediction at most

// the served shapes, stated once (include/esn_hip.h restates them in words, cnn.train_shape_error on the host)
const char* cnn_shape_limit(int n_in, int c1, int c2, int n_out, int kernel, int T) {
    if (n_in < 1 || n_in > 64) return "n_in must be in [1, 64]";
    if (c1 < 1 || c1 > 128 || c2 < 1 || c2 > 128) return "the channels c1, c2 must be in [1, 128]";
    if (n_out < 1 || n_out > 8) return "n_out must be in [1, 8]";
    if (kernel != 1 && kernel != 3 && kernel != 5 && kernel != 7) return "the kernel size must be 1, 3, 5 or 7";
    if (T < 1 || T > 4096) return "T must be in [1, 4096]";
    return nullptr;
}

// one group's (train) or one workgroup's (predict) part of the workspace, offsets in doubles.  Layer l = 0, 1, 2 maps
// c[l] -> c[l + 1] channels; xp[l] is its padded input, dz[l] its padded output gradient.
struct CnnWs {
    int c[4], K[3], rows;                      // rows = T + 2 p
    size_t prm[3], m[3], v[3], xp[3], dz[3], total;
};
__host__ __device__ inline CnnWs cnn_ws(int n_in, int c1, int c2, int n_out, int kernel, int T, bool train) {
    CnnWs w;
    w.c[0] = n_in; w.c[1] = c1; w.c[2] = c2; w.c[3] = n_out;
    w.rows = T + kernel - 1;
    size_t at = 0;
    for (int l = 0; l < 3; ++l) {
        w.K[l] = kernel * w.c[l];
        const size_t n = (size_t)w.c[l + 1] * (w.K[l] + 1);
        w.prm[l] = at; at += n;
        w.m[l] = at; if (train) at += n;
        w.v[l] = at; if (train) at += n;
    }
    for (int l = 0; l < 3; ++l) { w.xp[l] = at; at += (size_t)w.rows * w.c[l]; }
    for (int l = 0; l < 3; ++l) { w.dz[l] = at; if (train) at += (size_t)w.rows * w.c[l + 1]; }
    w.total = at;
    return w;
}
size_t cnn_workspace_bytes(int n_in, int c1, int c2, int n_out, int kernel, int n_groups, int n_frames, int T) {
    const size_t tr = n_groups > 0 ? (size_t)n_groups * cnn_ws(n_in, c1, c2, n_out, kernel, T, true).total : 0;
    const int wgs = n_frames < CNN_PRED_WGS ? n_frames : CNN_PRED_WGS;
    const size_t pr = wgs > 0 ? (size_t)wgs * cnn_ws(n_in, c1, c2, n_out, kernel, T, false).total : 0;
    return (tr > pr ? tr : pr) * sizeof(double);
}

// the layer's input gradient behind the ReLU that made its input: dzin[(t + p) c_in + i] = (sum_j' sum_o
// dzp[(t + j') c_out + o] W[o][i][k - 1 - j']) [xp[(t + p) c_in + i] > 0], j' and within it o ascending
__device__ __forceinline__ void cnn_input_grad(const double* dzp, const double* P, const double* xp, double* dzin, int T,
                                               int c_in, int c_out, int kernel, int wave, int lane) {
    const int lr = lane & 15, lq = lane >> 4, KS = kernel * c_in + 1, pad = (kernel - 1) / 2;
    const int nrt = (T + 15) / 16, nct = (c_in + 15) / 16, ncs = (nct + CNN_NB - 1) / CNN_NB;
    for (int s = wave; s < nrt * ncs; s += CNN_WAVES) {
        const int rt = s / ncs, ct0 = (s - rt * ncs) * CNN_NB;
        const int t = 16 * rt + lr < T ? 16 * rt + lr : T - 1;
        int ic[CNN_NB];
        cnn_f64x4 acc[CNN_NB];
#pragma unroll
        for (int q = 0; q < CNN_NB; ++q) {
            ic[q] = 16 * (ct0 + q) + lr < c_in ? 16 * (ct0 + q) + lr : c_in - 1;
            acc[q] = cnn_f64x4{0.0, 0.0, 0.0, 0.0};
        }
        for (int j = 0; j < kernel; ++j) {
            const double* a = dzp + (size_t)(t + j) * c_out;
            const double* b = P + (size_t)(kernel - 1 - j) * c_in;
            for (int o0 = 0; o0 < c_out; o0 += 4) {
                const int o = o0 + lq;
                const bool in = o < c_out;
                const double av = in ? a[o] : 0.0;
#pragma unroll
                for (int q = 0; q < CNN_NB; ++q)
                    if (ct0 + q < nct) acc[q] = cnn_mfma(av, in ? b[(size_t)o * KS + ic[q]] : 0.0, acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < CNN_NB; ++q) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 16 * rt + 4 * i + lq, col = 16 * (ct0 + q) + lr;
                if (row < T && col < c_in) {
                    const size_t at = (size_t)(row + pad) * c_in + col;
                    dzin[at] = xp[at] > 0.0 ? acc[q][i] : 0.0;
                }
            }
        }
    }
}

// P [c_out][K + 1] of one layer from torch's Conv1d layout W [c_out][c_in][k], b [c_out], and back
__device__ __forceinline__ void cnn_load_params(double* P, const double* W, const double* b, int c_in, int c_out,
                                                int kernel, int tid) {
    const int K = kernel * c_in, KS = K + 1;
    for (int e = tid; e < c_out * KS; e += CNN_THREADS) {
        const int o = e / KS, kk = e - o * KS;
        if (kk == K) {
            P[e] = b[o];
        } else {
            const int j = kk / c_in, i = kk - j * c_in;
            P[e] = W[((size_t)o * c_in + i) * kernel + j];
        }
    }
}
__device__ __forceinline__ void cnn_store_params(const double* P, double* W, double* b, int c_in, int c_out, int kernel,
                                                 int tid) {
    const int K = kernel * c_in, KS = K + 1;
    for (int e = tid; e < c_out * KS; e += CNN_THREADS) {
        const int o = e / KS, kk = e - o * KS;
        if (kk == K) {
            b[o] = P[e];
        } else {
            const int j = kk / c_in, i = kk - j * c_in;
            W[((size_t)o * c_in + i) * kernel + j] = P[e];
        }
    }
}

// the padded, scaled input of one sequence (zero rows appended BEFORE scaling) and the zero rows of every padded array
__device__ __forceinline__ void cnn_stage_input(double* xp0, const double* U, const double* in_scale, const double* in_shift,
                                                int T_in, int T, int n_in, int pad, int tid) {
    for (int e = tid; e < T * n_in; e += CNN_THREADS) {
        const int t = e / n_in, i = e - t * n_in;
        const double u = t < T_in ? U[e] : 0.0;
        xp0[(size_t)pad * n_in + e] = u * (in_scale ? in_scale[i] : 1.0) + (in_shift ? in_shift[i] : 0.0);
    }
}
__device__ __forceinline__ void cnn_zero_pads(double* xp, int T, int c, int pad, int tid) {
    for (int e = tid; e < pad * c; e += CNN_THREADS) {
        xp[e] = 0.0;
        xp[(size_t)(T + pad) * c + e] = 0.0;
    }
}

// (4 waves per SIMD: at most 128 VGPRs, so two workgroups share a CU and one fills the other's barriers and load waits;
// compiled freely the kernel takes 133 and ran at 0.72 of this speed)
__global__ __launch_bounds__(CNN_THREADS, 4) void cnn_train_kernel(CnnParams p) {
    __shared__ double lossw[CNN_WAVES];
    const int tid = threadIdx.x, g = blockIdx.x, wave = tid >> 6, lane = tid & 63;
    const int T = p.T, kernel = p.kernel, pad = (kernel - 1) / 2, n_out = p.n_out;
    const CnnWs w = cnn_ws(p.n_in, p.c1, p.c2, n_out, kernel, T, true);
    double* ws = p.workspace + (size_t)g * w.total;
    const int s = (int)((p.group_offset + (unsigned long long)g) % (unsigned long long)p.n_isets);
    const int nR = T - p.transient;
    const double inv_n = 1.0 / ((double)nR * (double)n_out), gscale = 2.0 * inv_n;

#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const size_t nw = (size_t)w.c[l + 1] * w.K[l];
        cnn_load_params(ws + w.prm[l], p.W0[l] + (size_t)s * nw, p.b0[l] + (size_t)s * w.c[l + 1], w.c[l], w.c[l + 1],
                        kernel, tid);
        cnn_zero_pads(ws + w.xp[l], T, w.c[l], pad, tid);
        cnn_zero_pads(ws + w.dz[l], T, w.c[l + 1], pad, tid);
    }
    cnn_stage_input(ws + w.xp[0], p.U + (size_t)g * p.T_in * p.n_in, p.in_scale ? p.in_scale + (size_t)g * p.n_in : nullptr,
                    p.in_shift ? p.in_shift + (size_t)g * p.n_in : nullptr, p.T_in, T, p.n_in, pad, tid);
    const double* Dg = p.D + (size_t)g * T * n_out;
    const double* tsc = p.t_scale ? p.t_scale + (size_t)g * n_out : nullptr;
    const double* tsh = p.t_shift ? p.t_shift + (size_t)g * n_out : nullptr;
    double b1pow = 1.0, b2pow = 1.0;
    __syncthreads();

    for (int ep = 0; ep < p.epochs; ++ep) {
        // ---- forward: x1, x2 behind their ReLUs, then the output gradient and this lane's part of the loss
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            double* xn = ws + w.xp[l + 1] + (size_t)pad * w.c[l + 1];
            const int cn = w.c[l + 1];
            cnn_forward(ws + w.xp[l], ws + w.prm[l], T, w.c[l], cn, w.K[l], wave, lane,
                        [=](int t, int o, double z) { xn[(size_t)t * cn + o] = fmax(z, 0.0); });
            __syncthreads();
        }
        double lsum = 0.0;
        {
            double* dz3 = ws + w.dz[2] + (size_t)pad * n_out;
            const int transient = p.transient;
            cnn_forward(ws + w.xp[2], ws + w.prm[2], T, w.c[2], n_out, w.K[2], wave, lane, [&](int t, int o, double z) {
                const double diff = z - (Dg[(size_t)t * n_out + o] * (tsc ? tsc[o] : 1.0) + (tsh ? tsh[o] : 0.0));
                const bool on = t >= transient;
                dz3[(size_t)t * n_out + o] = on ? diff * gscale : 0.0;
                if (on) lsum += diff * diff;
            });
        }
        __syncthreads();
        // ---- the gradients of x2 and x1
#pragma unroll
        for (int l = 2; l >= 1; --l) {
            cnn_input_grad(ws + w.dz[l], ws + w.prm[l], ws + w.xp[l], ws + w.dz[l - 1], T, w.c[l], w.c[l + 1], kernel, wave,
                           lane);
            __syncthreads();
        }
        // ---- the loss before this step: lanes by xor-shuffles, waves in order
        if (p.loss) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) lsum += __shfl_xor(lsum, d);
            if (lane == 0) lossw[wave] = lsum;
            __syncthreads();
            if (tid == 0) {
                double sum = 0.0;
                for (int e = 0; e < CNN_WAVES; ++e) sum += lossw[e];
                p.loss[(size_t)g * p.epochs + ep] = sum * inv_n;
            }
        }
        // ---- weight gradients and Adam, the strips of the three layers in one list (the heaviest layer first)
        b1pow *= p.beta1;
        b2pow *= p.beta2;
        const CnnAdam ad = {p.beta1, p.beta2, p.lr / (1.0 - b1pow), sqrt(1.0 - b2pow), p.eps, ep == 0};
        int base = 0;          // strips handed out so far: wave w takes those whose place in the list is w mod 8
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int l = q == 0 ? 1 : (q == 1 ? 2 : 0);
            const int nct = (w.K[l] + 1 + 15) / 16;
            const int n_strips = ((w.c[l + 1] + 15) / 16) * ((nct + CNN_NB - 1) / CNN_NB);
            for (int sl = (wave - base % CNN_WAVES + CNN_WAVES) % CNN_WAVES; sl < n_strips; sl += CNN_WAVES)
                cnn_weight_grad_strip(sl, ws + w.dz[l], ws + w.xp[l], ws + w.prm[l], ws + w.m[l], ws + w.v[l], T, w.c[l],
                                      w.c[l + 1], kernel, lane, ad);
            base += n_strips;
        }
        __syncthreads();
    }

#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const size_t nw = (size_t)w.c[l + 1] * w.K[l];
        cnn_store_params(ws + w.prm[l], p.W[l] + (size_t)g * nw, p.b[l] + (size_t)g * w.c[l + 1], w.c[l], w.c[l + 1], kernel,
                         tid);
    }
}

__global__ __launch_bounds__(CNN_THREADS) void cnn_predict_kernel(CnnParams p) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int T = p.T, kernel = p.kernel, pad = (kernel - 1) / 2, n_out = p.n_out, rows_out = T - p.transient;
    const CnnWs w = cnn_ws(p.n_in, p.c1, p.c2, n_out, kernel, T, false);
    double* ws = p.workspace + (size_t)blockIdx.x * w.total;
#pragma unroll
    for (int l = 0; l < 3; ++l) cnn_zero_pads(ws + w.xp[l], T, w.c[l], pad, tid);
    for (int f = blockIdx.x; f < p.n_frames; f += gridDim.x) {
        const int g = f / p.frames_per_group;
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            const size_t nw = (size_t)w.c[l + 1] * w.K[l];
            cnn_load_params(ws + w.prm[l], p.W0[l] + (size_t)g * nw, p.b0[l] + (size_t)g * w.c[l + 1], w.c[l], w.c[l + 1],
                            kernel, tid);
        }
        cnn_stage_input(ws + w.xp[0], p.U + (size_t)f * p.T_in * p.n_in,
                        p.in_scale ? p.in_scale + (size_t)g * p.n_in : nullptr,
                        p.in_shift ? p.in_shift + (size_t)g * p.n_in : nullptr, p.T_in, T, p.n_in, pad, tid);
        __syncthreads();
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            double* xn = ws + w.xp[l + 1] + (size_t)pad * w.c[l + 1];
            const int cn = w.c[l + 1];
            cnn_forward(ws + w.xp[l], ws + w.prm[l], T, w.c[l], cn, w.K[l], wave, lane,
                        [=](int t, int o, double z) { xn[(size_t)t * cn + o] = fmax(z, 0.0); });
            __syncthreads();
        }
        const double* tsc = p.t_scale ? p.t_scale + (size_t)g * n_out : nullptr;
        const double* tsh = p.t_shift ? p.t_shift + (size_t)g * n_out : nullptr;
        double* Yf = p.Y + (size_t)f * rows_out * n_out;
        const int transient = p.transient;
        cnn_forward(ws + w.xp[2], ws + w.prm[2], T, w.c[2], n_out, w.K[2], wave, lane, [=](int t, int o, double z) {
            if (t >= transient)
                Yf[(size_t)(t - transient) * n_out + o] = (z - (tsh ? tsh[o] : 0.0)) / (tsc ? tsc[o] : 1.0);
        });
        __syncthreads();                                                   // the next frame overwrites the scratch
    }
}

int launch_cnn_train(const CnnParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(cnn_train_kernel, dim3((unsigned)p.n_groups), dim3(CNN_THREADS), 0, stream, p);
    return (int)hipGetLastError();
}

int launch_cnn_predict(const CnnParams& p, hipStream_t stream) {
    const int wgs = p.n_frames < CNN_PRED_WGS ? p.n_frames : CNN_PRED_WGS;
    hipLaunchKernelGGL(cnn_predict_kernel, dim3((unsigned)wgs), dim3(CNN_THREADS), 0, stream, p);
    return (int)hipGetLastError();
}

}  // namespace esn
