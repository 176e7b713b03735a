// Windowed FNN (include/esn_hip.h: esn_fnn_train): Linear -> ReLU -> Linear over the ELM's window of scaled input rows,
// trained per group by `epochs` full-batch Adam steps on the mean squared error -- the reference's FNNModel and its
// training loop (system_model_2_all_comparision.py:40-49, :129-142).  The prediction is the ELM's kernels with ReLU
// (esn_elm.hip, launch_fnn_predict); this file is the training.
//
// fnn_train_kernel   one workgroup of 512 threads per group, one launch for all epochs, float64, plain FMA.
//   LDS      the master copy of W1 [H][K | 1] (odd row stride), W2, b1, b2; the group's scaled rows us [T][n_in], staged
//            once (the window of row t is the view us[t-(w-1) .. t], as in elm_f64_kernel); per tile of 16 trained rows
//            the hidden rows h, the hidden gradients dh and the output gradients dy.
//   forward  thread (hidden block of 4, rows rb + 4 j, k part kp of 4) holds a 4 x 4 block of partial sums over
//            k = kp, kp + 4, ..; the four parts join by two lane exchanges ((0 + 1) + (2 + 3)).
//   output   thread (row, output, part of 4): sum over h = part, part + 4, .., joined the same way; dy = 2 (ys - Ds) /
//            (|R| n_out), zero for the rows of the last tile beyond T; the squared residual goes to the item's own
//            loss sum.
//   dh       thread per (row, unit): (sum_o dy W2[o][h]) [h > 0], o ascending.
//   grads    the lanes that own the parameters add the tile's rows in ascending order into registers: a thread owns
//            W1[4 hb + i][kb + nkb j] (i < 4, j < 8, nkb = ceil(K / 8)), up to two elements of W2, one of b1, one of b2.
//   Adam     after the last tile and a barrier, by the owners, into LDS.  The moments of W2, b1 and b2 stay in the
//            owners' registers for the whole launch; those of W1 (64 doubles per thread beside the 32 gradient sums)
//            do not fit there and live in the caller's workspace, [group][m | v][element of the block][owner], read
//            and written by the owner alone, one coalesced line per element (never read in the first epoch, so the
//            workspace needs no zeroing).  beta^e by repeated multiplication.
// Every sum's order depends on the shape alone and nothing leaves the workgroup before the end, so a group is bitwise
// the same alone and inside any batch.  No atomics.  A parameter whose gradient is exactly 0 in every epoch keeps
// m = v = 0 and p - step * (0 / (0 + eps)) = p: bitwise untouched.
#include <atomic>
#include "esn_common.h"
#include "esn_launch.h"

namespace esn {

constexpr int FNN_THREADS = 512;
constexpr int FNN_TR = 16;                     // rows of a tile
constexpr int FNN_HB = 4, FNN_KB = 8;          // a thread's block of W1: 4 units x 8 window elements
constexpr int FNN_W2_PER = 2;                  // elements of W2 per thread: n_out n_hidden <= 1024
constexpr int FNN_DYS = 8;                     // row stride of dy (n_out <= 8)
constexpr size_t FNN_MAX_LDS = 160 * 1024;

struct FnnLds {                                // offsets in doubles
    int ks, hs, w1, us, w2, b1, b2, ht, dht, dyt, lossb, total;
};
__host__ __device__ inline FnnLds fnn_lds(int n_in, int H, int w, int n_out, int T) {
    FnnLds l;
    l.ks = (w * n_in) | 1;
    l.hs = H | 1;
    l.w1 = 0;
    l.us = l.w1 + H * l.ks;
    l.w2 = l.us + ((T * n_in + 1) & ~1);
    l.b1 = l.w2 + n_out * H;
    l.b2 = l.b1 + H;
    l.ht = l.b2 + n_out;
    l.dht = l.ht + FNN_TR * l.hs;
    l.dyt = l.dht + FNN_TR * l.hs;
    l.lossb = l.dyt + FNN_TR * FNN_DYS;
    l.total = l.lossb + FNN_TR * FNN_DYS;
    return l;
}
size_t fnn_train_workspace_bytes(int n_in, int n_hidden, int window, int n_groups) {
    const size_t n_own = (size_t)((n_hidden + FNN_HB - 1) / FNN_HB) * ((window * n_in + FNN_KB - 1) / FNN_KB);
    return (size_t)n_groups * 2 * FNN_HB * FNN_KB * n_own * sizeof(double);
}
size_t fnn_train_lds_bytes(int n_in, int n_hidden, int window, int n_out, int T) {
    const long long w1 = (long long)n_hidden * ((window * n_in) | 1), us = (long long)T * n_in;
    if (w1 + us > (long long)FNN_MAX_LDS) return (size_t)-1;           // (far beyond LDS: no int overflow below)
    return (size_t)fnn_lds(n_in, n_hidden, window, n_out, T).total * sizeof(double);
}

// a + the value of lane ^ 1, then + lane ^ 2: all four lanes of a quad end with ((q0 + q1) + (q2 + q3)), bitwise alike
__device__ __forceinline__ double fnn_quad_sum(double a) {
    a += __shfl_xor(a, 1);
    a += __shfl_xor(a, 2);
    return a;
}

// (fnn_adam, the Adam step, is in esn_common.h: the windowed CNN shares it)

__global__ __launch_bounds__(FNN_THREADS) void fnn_train_kernel(FnnTrainParams p) {
    extern __shared__ __attribute__((aligned(16))) char fsm[];
    double* sm = reinterpret_cast<double*>(fsm);
    const int n_in = p.n_in, w = p.window, K = w * n_in, H = p.n_hidden, n_out = p.n_out, T = p.T;
    const FnnLds l = fnn_lds(n_in, H, w, n_out, T);
    const int KS = l.ks, HS = l.hs;
    double *W1s = sm + l.w1, *us = sm + l.us, *W2s = sm + l.w2, *b1s = sm + l.b1, *b2s = sm + l.b2;
    double *ht = sm + l.ht, *dht = sm + l.dht, *dyt = sm + l.dyt, *lossb = sm + l.lossb;
    const int tid = threadIdx.x, g = blockIdx.x;
    const int s = (int)((p.group_offset + (unsigned long long)g) % (unsigned long long)p.n_isets);
    const int r0 = p.transient > w - 1 ? p.transient : w - 1, nR = T - r0;
    const int n_tiles = (nR + FNN_TR - 1) / FNN_TR;
    const double inv_n = 1.0 / ((double)nR * (double)n_out), gscale = 2.0 * inv_n;

    // ---- the master copy and the group's scaled rows
    for (int e = tid; e < H * K; e += FNN_THREADS) {
        const int h = e / K, k = e - h * K;
        W1s[h * KS + k] = p.W1_0[(size_t)s * H * K + e];
    }
    for (int e = tid; e < n_out * H; e += FNN_THREADS) W2s[e] = p.W2_0[(size_t)s * n_out * H + e];
    for (int e = tid; e < H; e += FNN_THREADS) b1s[e] = p.b1_0[(size_t)s * H + e];
    if (tid < n_out) b2s[tid] = p.b2_0[(size_t)s * n_out + tid];
    for (int e = tid; e < T * n_in; e += FNN_THREADS) {
        const int t = e / n_in, i = e - t * n_in;
        const double u = t < p.T_in ? p.U[((size_t)g * p.T_in + t) * n_in + i] : 0.0;      // zero rows BEFORE scaling
        const double sc = p.in_scale ? p.in_scale[(size_t)g * n_in + i] : 1.0;
        const double sh = p.in_shift ? p.in_shift[(size_t)g * n_in + i] : 0.0;
        us[e] = u * sc + sh;
    }

    // ---- what this thread owns
    const int nkb = (K + FNN_KB - 1) / FNN_KB, nhb = (H + FNN_HB - 1) / FNN_HB;
    const bool own1 = tid < nhb * nkb;
    const int hb1 = own1 ? tid / nkb : 0, kb1 = own1 ? tid - hb1 * nkb : 0;
    int oh[FNN_HB], ok[FNN_KB];                // clamped indices: a block beyond H or K reads the last element, writes nothing
#pragma unroll
    for (int i = 0; i < FNN_HB; ++i) oh[i] = FNN_HB * hb1 + i < H ? FNN_HB * hb1 + i : H - 1;
#pragma unroll
    for (int j = 0; j < FNN_KB; ++j) ok[j] = kb1 + nkb * j < K ? kb1 + nkb * j : K - 1;
    const int n_own = nhb * nkb;
    double* mw = p.workspace + (size_t)g * 2 * FNN_HB * FNN_KB * n_own + tid;       // m of this thread's element e at
    double* vw = mw + (size_t)FNN_HB * FNN_KB * n_own;                              // mw[e n_own], v at vw[e n_own]
    int e2[FNN_W2_PER], o2[FNN_W2_PER], h2[FNN_W2_PER];
    bool own2[FNN_W2_PER];
    double m2[FNN_W2_PER], v2[FNN_W2_PER];
#pragma unroll
    for (int j = 0; j < FNN_W2_PER; ++j) {
        const int e = tid + FNN_THREADS * j;
        own2[j] = e < n_out * H;
        e2[j] = own2[j] ? e : 0;
        o2[j] = e2[j] / H;
        h2[j] = e2[j] - o2[j] * H;
        m2[j] = v2[j] = 0.0;
    }
    const bool ownb1 = tid < H, ownb2 = tid < n_out;
    double mb1 = 0.0, vb1 = 0.0, mb2 = 0.0, vb2 = 0.0;
    // forward: hidden block (tid >> 4, + 32 ..), rows rb + 4 j of the tile, k = kp, kp + 4, ..
    const int kp = tid & 3, rb = (tid >> 2) & 3;
    // output: item (row, output) = tid >> 2, part tid & 3
    const int item = tid >> 2, n_items = FNN_TR * n_out;
    const int ir = item < n_items ? item / n_out : 0, io = item < n_items ? item - ir * n_out : 0;
    const double tsc = p.t_scale ? p.t_scale[(size_t)g * n_out + io] : 1.0;
    const double tsh = p.t_shift ? p.t_shift[(size_t)g * n_out + io] : 0.0;
    double b1pow = 1.0, b2pow = 1.0;
    __syncthreads();

    for (int ep = 0; ep < p.epochs; ++ep) {
        double g1[FNN_HB][FNN_KB], g2[FNN_W2_PER], gb1 = 0.0, gb2 = 0.0, lsum = 0.0;
#pragma unroll
        for (int i = 0; i < FNN_HB; ++i) {
#pragma unroll
            for (int j = 0; j < FNN_KB; ++j) g1[i][j] = 0.0;
        }
#pragma unroll
        for (int j = 0; j < FNN_W2_PER; ++j) g2[j] = 0.0;

        for (int tile = 0; tile < n_tiles; ++tile) {
            const int t0 = r0 + tile * FNN_TR;
            // ---- h = max(x W1^T + b1, 0)
            for (int hb = tid >> 4; hb < nhb; hb += FNN_THREADS / 16) {
                const double* wr[4];
                const double* xr[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int h = 4 * hb + i < H ? 4 * hb + i : H - 1;
                    wr[i] = W1s + h * KS;
                    const int t = t0 + rb + 4 * i < T ? t0 + rb + 4 * i : T - 1;
                    xr[i] = us + (t - (w - 1)) * n_in;
                }
                double acc[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
                }
                for (int k = kp; k < K; k += 4) {
                    double wv[4], xv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) { wv[i] = wr[i][k]; xv[i] = xr[i][k]; }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[i][j] = fma(wv[i], xv[j], acc[i][j]);
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double pre = fnn_quad_sum(acc[i][j]);
                        if (kp == 0 && 4 * hb + i < H) ht[(rb + 4 * j) * HS + 4 * hb + i] = fmax(pre + b1s[4 * hb + i], 0.0);
                    }
                }
            }
            __syncthreads();
            // ---- dy = 2 (ys - Ds) / (|R| n_out)
            if (item < n_items) {
                double sum = 0.0;
                const double* hr = ht + ir * HS;
                const double* w2r = W2s + io * H;
                for (int h = kp; h < H; h += 4) sum = fma(w2r[h], hr[h], sum);
                sum = fnn_quad_sum(sum);
                if (kp == 0) {
                    const int t = t0 + ir;
                    double dy = 0.0;
                    if (t < T) {
                        const double diff = (sum + b2s[io]) - (p.D[((size_t)g * T + t) * n_out + io] * tsc + tsh);
                        dy = diff * gscale;
                        lsum += diff * diff;
                    }
                    dyt[ir * FNN_DYS + io] = dy;
                }
            }
            __syncthreads();
            // ---- dh = (dy W2) [h > 0]
            for (int e = tid; e < FNN_TR * H; e += FNN_THREADS) {
                const int r = e / H, h = e - r * H;
                double sum = 0.0;
                for (int o = 0; o < n_out; ++o) sum = fma(dyt[r * FNN_DYS + o], W2s[o * H + h], sum);
                dht[r * HS + h] = ht[r * HS + h] > 0.0 ? sum : 0.0;
            }
            __syncthreads();
            // ---- the four gradients, rows ascending
            if (own1) {
                for (int r = 0; r < FNN_TR; ++r) {
                    const int t = t0 + r < T ? t0 + r : T - 1;
                    const double* xr = us + (t - (w - 1)) * n_in;
                    const double* dr = dht + r * HS;
                    double d[FNN_HB], x[FNN_KB];
#pragma unroll
                    for (int i = 0; i < FNN_HB; ++i) d[i] = dr[oh[i]];
#pragma unroll
                    for (int j = 0; j < FNN_KB; ++j) x[j] = xr[ok[j]];
#pragma unroll
                    for (int i = 0; i < FNN_HB; ++i) {
#pragma unroll
                        for (int j = 0; j < FNN_KB; ++j) g1[i][j] = fma(d[i], x[j], g1[i][j]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < FNN_W2_PER; ++j) {
                if (own2[j]) {
                    for (int r = 0; r < FNN_TR; ++r) g2[j] = fma(dyt[r * FNN_DYS + o2[j]], ht[r * HS + h2[j]], g2[j]);
                }
            }
            if (ownb1) {
                for (int r = 0; r < FNN_TR; ++r) gb1 += dht[r * HS + tid];
            }
            if (ownb2) {
                for (int r = 0; r < FNN_TR; ++r) gb2 += dyt[r * FNN_DYS + tid];
            }
            __syncthreads();
        }

        // ---- the loss before this step: the items' sums, in item order
        if (p.loss) {
            if (item < n_items && kp == 0) lossb[item] = lsum;
            __syncthreads();
            if (tid == 0) {
                double sum = 0.0;
                for (int e = 0; e < n_items; ++e) sum += lossb[e];
                p.loss[(size_t)g * p.epochs + ep] = sum * inv_n;
            }
        }
        // ---- Adam, by the owners
        b1pow *= p.beta1;
        b2pow *= p.beta2;
        const double step = p.lr / (1.0 - b1pow), rs2 = sqrt(1.0 - b2pow);
        if (own1) {
#pragma unroll
            for (int i = 0; i < FNN_HB; ++i) {
#pragma unroll
                for (int j = 0; j < FNN_KB; ++j) {
                    if (FNN_HB * hb1 + i < H && kb1 + nkb * j < K) {
                        const size_t at = (size_t)(i * FNN_KB + j) * n_own;
                        double m = ep ? mw[at] : 0.0, v = ep ? vw[at] : 0.0;
                        fnn_adam(W1s[oh[i] * KS + ok[j]], m, v, g1[i][j], p.beta1, p.beta2, step, rs2, p.eps);
                        mw[at] = m;
                        vw[at] = v;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < FNN_W2_PER; ++j) {
            if (own2[j]) fnn_adam(W2s[e2[j]], m2[j], v2[j], g2[j], p.beta1, p.beta2, step, rs2, p.eps);
        }
        if (ownb1) fnn_adam(b1s[tid], mb1, vb1, gb1, p.beta1, p.beta2, step, rs2, p.eps);
        if (ownb2) fnn_adam(b2s[tid], mb2, vb2, gb2, p.beta1, p.beta2, step, rs2, p.eps);
        __syncthreads();
    }

    for (int e = tid; e < H * K; e += FNN_THREADS) {
        const int h = e / K, k = e - h * K;
        p.W1[(size_t)g * H * K + e] = W1s[h * KS + k];
    }
    for (int e = tid; e < n_out * H; e += FNN_THREADS) p.W2[(size_t)g * n_out * H + e] = W2s[e];
    for (int e = tid; e < H; e += FNN_THREADS) p.b1[(size_t)g * H + e] = b1s[e];
    if (tid < n_out) p.b2[(size_t)g * n_out + tid] = b2s[tid];
}

int launch_fnn_train(const FnnTrainParams& p, hipStream_t stream) {
    static std::atomic<unsigned long long> raised{0};
    const int e = raise_dynamic_lds_once(reinterpret_cast<const void*>(fnn_train_kernel), FNN_MAX_LDS, raised);
    if (e) return e;
    hipLaunchKernelGGL(fnn_train_kernel, dim3((unsigned)p.n_groups), dim3(FNN_THREADS),
                       fnn_train_lds_bytes(p.n_in, p.n_hidden, p.window, p.n_out, p.T), stream, p);
    return (int)hipGetLastError();
}

}  // namespace esn
