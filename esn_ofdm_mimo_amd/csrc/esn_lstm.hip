// LSTM comparator (include/esn_hip.h: esn_lstm_train / esn_lstm_predict): one LSTM layer n_in -> H and a linear read-out
// H -> n_out over the whole scaled sequence, trained per group by `epochs` full-batch Adam steps on the mean squared
// error -- the reference's RNNModel and its training loop (system_model_2_all_comparision.py:29-38, :93-113).
//
// The parameters are kept as three layers in the packed layout of esn_f64_strip.h, P [c_out][c_in + 1] with the bias as
// the last column:  l = 0  P_ih [4H][n_in + 1] = [W_ih | b_ih],  l = 1  P_hh [4H][H + 1] = [W_hh | b_hh],
// l = 2  P_fc [n_out][H + 1] = [W_fc | b_fc].
//
// lstm_train_kernel   one workgroup of 512 threads per group, one launch for all epochs, float64.  A group's P, Adam's
//   moments, the scaled input, the gates, c, tanh(c), h, dz and dys live in its part of the caller's workspace (lstm_ws),
//   which only this workgroup touches.  Rows 0 of c and h are c[-1] = h[-1] = 0, written once; the moments are never read
//   in the first epoch: the workspace needs no zeroing.  An epoch:
//     a. xproj [T x 4H] = [X | 1] . P_ih^T + b_hh                                      (cnn_forward, matrix pipe)
//     b. forward sweep, t ascending: z = xproj[t] + W_hh h[t-1], gates (stored over xproj[t]), c, tanh(c), h
//     c. ys = [Hs | 1] . P_fc^T, the loss and dys = 2 (ys - Ds) / (|R| n_out), 0 before `transient`   (cnn_forward)
//     d. backward sweep, t descending: dh = W_fc^T dys[t] + W_hh^T dz[t+1], through the gates to dz[t]
//     e. dP_hh = dz^T [Hprev | 1], dP_ih = dz^T [X | 1], dP_fc = dys^T [Hs | 1] with the Adam step of every element by
//        the lane that holds it                                                        (cnn_weight_grad_strip)
//   The sweeps are 2 T dependent steps.  W_hh stays in registers and LDS from the Adam step of one epoch to that of the
//   next, in a two-dimensional split: thread (tr, tc) = (tid / 8, tid % 8) holds rows tr + 64 j, columns tc + 8 k.  The forward
//   step sums along its rows (k ascending), then over tc by xor-shuffles 1, 2, 4; the backward step sums down its
//   columns (j ascending), then over tr by xor-shuffles 8, 16, 32 and over the eight waves in order through LDS.  Thread
//   u < H owns hidden unit u in both sweeps: its c[t-1] and dc[t+1] never leave their register.
//     H <= 104         7 x 13 doubles per thread hold all of W_hh (448 x 104): 7 x 9 in registers, 7 x 4 in LDS (112 KB)
//     104 < H <= 128   8 x 12 doubles per thread (8 x 8 in registers, 8 x 4 in LDS, 128 KB) hold columns below 96;
//                      columns 96 .. H - 1 are read each step from the group's P_hh (L1 / L2)
//   Barriers inside a sweep wait for LDS only: a step's stores to the workspace are read again by their own thread, or
//   after the workgroup barrier that ends the sweep.  No atomics, nothing leaves the workgroup, every sum's order depends
//   on the shape alone: a group is bitwise the same alone and in any batch; the loss output changes nothing.
//
// lstm_predict_kernel  forward only.  A workgroup takes a tile of up to 16 frames of one group through all T steps
//   (at most LSTM_PRED_WGS workgroups take the tiles in turn).  Per step z [16 x 4H] = [h | x | 1] . B on
//   v_mfma_f64_16x16x4_f64 with the frames as the 16 rows.  Wave w owns the hidden units 16 w .. 16 w + 15 and the four
//   column tiles (one per gate) of those units, so a lane's four accumulators are i, f, g, o of the same (frame, unit):
//   the gates and c stay in registers, h goes to LDS as the next step's A operand and never to memory.  B in k-steps of
//   four: the first 16 k-steps of W_hh in registers, the next in LDS as far as it reaches (H <= 104: all 26), the rest
//   of W_hh and the k-steps of [W_ih | b_ih + b_hh] from an image in the workgroup's part of the workspace (L1 / L2),
//   which it lays out itself.  The last wave takes the read-out [h | 1] . P_fc^T of the step that was just finished.
//   Rows of a tile never mix: a frame is bitwise the same alone and in any batch.
#include "esn_common.h"
#include "esn_f64_strip.h"
#include "esn_launch.h"

namespace esn {

constexpr int LSTM_THREADS = CNN_THREADS;      // the strips of esn_f64_strip.h are dealt to eight waves
constexpr int LSTM_PRED_WGS = 1024;            // workgroups (and scratch regions) of a prediction at most
constexpr int LSTM_KREG = 16;                  // k-steps of W_hh a predicting wave keeps in registers
constexpr int LSTM_LDS = 160 * 1024;

// the served shapes, stated once (include/esn_hip.h restates them in words, lstm.train_shape_error on the host)
const char* lstm_shape_limit(int n_in, int n_hidden, int n_out, int T) {
    if (n_in < 1 || n_in > 64) return "n_in must be in [1, 64]";
    if (n_hidden < 1 || n_hidden > 128) return "n_hidden must be in [1, 128]";
    if (n_out < 1 || n_out > 8) return "n_out must be in [1, 8]";
    if (T < 1 || T > 4096) return "T must be in [1, 4096]";
    return nullptr;
}

// one group's part of the training workspace, offsets in doubles; layer l maps ci[l] -> co[l]
struct LstmWs {
    int ci[3], co[3];
    size_t prm[3], m[3], v[3], x, gates, cs, tcs, hs, dz, dys, total;
};
__host__ __device__ inline LstmWs lstm_ws(int n_in, int H, int n_out, int T) {
    LstmWs w;
    w.ci[0] = n_in; w.co[0] = 4 * H; w.ci[1] = H; w.co[1] = 4 * H; w.ci[2] = H; w.co[2] = n_out;
    size_t at = 0;
    for (int l = 0; l < 3; ++l) {
        const size_t n = (size_t)w.co[l] * (w.ci[l] + 1);
        w.prm[l] = at; at += n;
        w.m[l] = at; at += n;
        w.v[l] = at; at += n;
    }
    w.x = at; at += (size_t)T * n_in;
    w.gates = at; at += (size_t)T * 4 * H;       // xproj, then i, f, g, o
    w.cs = at; at += (size_t)(T + 1) * H;        // row t + 1 is c[t], row 0 zeros
    w.tcs = at; at += (size_t)T * H;             // tanh(c[t])
    w.hs = at; at += (size_t)(T + 1) * H;        // row t + 1 is h[t], row 0 zeros
    w.dz = at; at += (size_t)T * 4 * H;
    w.dys = at; at += (size_t)T * n_out;
    w.total = at;
    return w;
}

// the tiers of a prediction's B operand and what they take
struct LstmPred {
    int n_ut, ksh, ksx, hs, nreg, nlds, kstream;   // hs: row stride of h in LDS
    size_t lds_bytes, scratch;                     // scratch in doubles per workgroup
};
__host__ __device__ inline LstmPred lstm_pred(int n_in, int H) {
    LstmPred q;
    q.n_ut = (H + 15) / 16;
    q.ksh = (H + 3) / 4;
    q.ksx = (n_in + 1 + 3) / 4;
    q.hs = 4 * q.ksh + 1;
    const int hbuf = 16 * q.hs * 8, cap = (LSTM_LDS - hbuf) / (2048 * q.n_ut);
    q.nreg = q.ksh < LSTM_KREG ? q.ksh : LSTM_KREG;
    q.nlds = q.ksh - q.nreg < cap ? q.ksh - q.nreg : cap;
    q.kstream = q.ksh - q.nreg - q.nlds + q.ksx;
    q.lds_bytes = (size_t)hbuf + (size_t)q.nlds * q.n_ut * 2048;
    q.scratch = (size_t)q.n_ut * q.kstream * 256;
    return q;
}

size_t lstm_workspace_bytes(int n_in, int n_hidden, int n_out, int n_groups, int n_frames, int T) {
    const size_t tr = n_groups > 0 ? (size_t)n_groups * lstm_ws(n_in, n_hidden, n_out, T).total : 0;
    const int wgs = n_frames < LSTM_PRED_WGS ? n_frames : LSTM_PRED_WGS;
    const size_t pr = wgs > 0 ? (size_t)wgs * lstm_pred(n_in, n_hidden).scratch : 0;
    return (tr > pr ? tr : pr) * sizeof(double);
}

// a barrier that waits for this wave's LDS traffic only (the stores of a step to the workspace stay in flight)
__device__ __forceinline__ void lstm_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ double lstm_sigma(double a) { return 1.0 / (1.0 + exp(-a)); }

// W_hh[r][c] out of P_hh [4H][H + 1], zero beyond its ends (a clamped load and a select: no branch per element)
__device__ __forceinline__ double lstm_whh(const double* Phh, int r, int c, int H) {
    const double v = Phh[(size_t)(r < 4 * H ? r : 4 * H - 1) * (H + 1) + (c < H ? c : H - 1)];
    return (r < 4 * H && c < H) ? v : 0.0;
}

// P [c_out][c_in + 1] of one layer from torch's layout W [c_out][c_in], b [c_out], and back
__device__ __forceinline__ void lstm_load_params(double* P, const double* W, const double* b, int c_in, int c_out, int tid) {
    const int KS = c_in + 1;
    for (int e = tid; e < c_out * KS; e += LSTM_THREADS) {
        const int o = e / KS, k = e - o * KS;
        P[e] = k == c_in ? b[o] : W[(size_t)o * c_in + k];
    }
}
__device__ __forceinline__ void lstm_store_params(const double* P, double* W, double* b, int c_in, int c_out, int tid) {
    const int KS = c_in + 1;
    for (int e = tid; e < c_out * KS; e += LSTM_THREADS) {
        const int o = e / KS, k = e - o * KS;
        if (k == c_in) b[o] = P[e]; else W[(size_t)o * c_in + k] = P[e];
    }
}

// Of W_hh a thread holds RJ rows x (CKR columns in registers, the next CKL in LDS); columns tc + 8 k, k >= CKR + CKL
// (H > 8 (CKR + CKL) only) come from P_hh each step
template <int RJ, int CKR, int CKL>
__global__ __launch_bounds__(LSTM_THREADS) void lstm_train_kernel(LstmParams p) {
    constexpr int CKT = CKR + CKL, NX = 16 - CKT;          // NX: streamed columns per thread at most (H <= 128)
    __shared__ double hl[128], zl[512], dzl[512], red[CNN_WAVES][128], lossw[CNN_WAVES];
    __shared__ double Wl[RJ * CKL][LSTM_THREADS];          // element (j, k) of every thread side by side: no bank conflicts
    const int tid = threadIdx.x, g = blockIdx.x, wave = tid >> 6, lane = tid & 63;
    const int H = p.n_hidden, H4 = 4 * H, KH = H + 1, n_in = p.n_in, n_out = p.n_out, T = p.T;
    const LstmWs w = lstm_ws(n_in, H, n_out, T);
    double* ws = p.workspace + (size_t)g * w.total;
    double *Pih = ws + w.prm[0], *Phh = ws + w.prm[1], *Pfc = ws + w.prm[2];
    double *X = ws + w.x, *gates = ws + w.gates, *cs = ws + w.cs, *tcs = ws + w.tcs, *hs = ws + w.hs, *dz = ws + w.dz,
           *dys = ws + w.dys;
    const int s = (int)((p.group_offset + (unsigned long long)g) % (unsigned long long)p.n_isets);
    const int nR = T - p.transient, transient = p.transient;
    const double inv_n = 1.0 / ((double)nR * (double)n_out), gscale = 2.0 * inv_n;

#pragma unroll
    for (int l = 0; l < 3; ++l)
        lstm_load_params(ws + w.prm[l], p.W0[l] + (size_t)s * w.co[l] * w.ci[l], p.b0[l] + (size_t)s * w.co[l], w.ci[l],
                         w.co[l], tid);
    {
        const double* U = p.U + (size_t)g * p.T_in * n_in;
        const double* isc = p.in_scale ? p.in_scale + (size_t)g * n_in : nullptr;
        const double* ish = p.in_shift ? p.in_shift + (size_t)g * n_in : nullptr;
        for (int e = tid; e < T * n_in; e += LSTM_THREADS) {
            const int t = e / n_in, i = e - t * n_in;
            const double u = t < p.T_in ? U[e] : 0.0;
            X[e] = u * (isc ? isc[i] : 1.0) + (ish ? ish[i] : 0.0);
        }
    }
    if (tid < H) {
        cs[tid] = 0.0;
        hs[tid] = 0.0;
    }
    const double* Dg = p.D + (size_t)g * T * n_out;
    const double* tsc = p.t_scale ? p.t_scale + (size_t)g * n_out : nullptr;
    const double* tsh = p.t_shift ? p.t_shift + (size_t)g * n_out : nullptr;
    const int tc = tid & 7, tr = tid >> 3, CK = (H + 7) / 8;
    const bool unit = tid < H;                             // this thread owns hidden unit `tid` in the sweeps
    double b1pow = 1.0, b2pow = 1.0;
    __syncthreads();

    for (int ep = 0; ep < p.epochs; ++ep) {
        // ---- W_hh of this epoch into registers
        double Wr[RJ][CKR];
#pragma unroll
        for (int j = 0; j < RJ; ++j) {
#pragma unroll
            for (int k = 0; k < CKR; ++k) {
                const int r = tr + 64 * j, c = tc + 8 * k;
                Wr[j][k] = lstm_whh(Phh, r, c, H);
            }
#pragma unroll
            for (int k = 0; k < CKL; ++k) {
                const int r = tr + 64 * j, c = tc + 8 * (CKR + k);
                Wl[j * CKL + k][tid] = lstm_whh(Phh, r, c, H);
            }
        }
        // ---- a. the input projection with both biases
        cnn_forward(X, Pih, T, n_in, H4, n_in, wave, lane,
                    [=](int t, int o, double z) { gates[(size_t)t * H4 + o] = z + Phh[(size_t)o * KH + H]; });
        if (tid < 128) hl[tid] = 0.0;
        dzl[tid] = 0.0;
        __syncthreads();

        // ---- b. forward sweep
        double cprev = 0.0;
        for (int t = 0; t < T; ++t) {
            double xz[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) xz[q] = unit ? gates[(size_t)t * H4 + q * H + tid] : 0.0;
            double pj[RJ];
#pragma unroll
            for (int j = 0; j < RJ; ++j) pj[j] = 0.0;
#pragma unroll
            for (int k = 0; k < CKR; ++k) {
                const double hv = hl[tc + 8 * k];
#pragma unroll
                for (int j = 0; j < RJ; ++j) pj[j] = fma(Wr[j][k], hv, pj[j]);
            }
#pragma unroll
            for (int k = 0; k < CKL; ++k) {
                const double hv = hl[tc + 8 * (CKR + k)];
#pragma unroll
                for (int j = 0; j < RJ; ++j) pj[j] = fma(Wl[j * CKL + k][tid], hv, pj[j]);
            }
            for (int k = CKT; k < CK; ++k) {
                const int c = tc + 8 * k;
                const double hv = hl[c];
#pragma unroll
                for (int j = 0; j < RJ; ++j) {
                    const int r = tr + 64 * j;
                    pj[j] = fma(lstm_whh(Phh, r, c, H), hv, pj[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < RJ; ++j) {
#pragma unroll
                for (int d = 1; d <= 4; d <<= 1) pj[j] += __shfl_xor(pj[j], d);
                if (tc == 0) zl[tr + 64 * j] = pj[j];
            }
            lstm_lds_barrier();
            if (unit) {
                const double gi = lstm_sigma(xz[0] + zl[tid]), gf = lstm_sigma(xz[1] + zl[H + tid]);
                const double gg = tanh(xz[2] + zl[2 * H + tid]), go = lstm_sigma(xz[3] + zl[3 * H + tid]);
                const double c = gf * cprev + gi * gg, tcv = tanh(c), h = go * tcv;
                double* gt = gates + (size_t)t * H4 + tid;
                gt[0] = gi; gt[H] = gf; gt[2 * H] = gg; gt[3 * H] = go;
                cs[(size_t)(t + 1) * H + tid] = c;
                tcs[(size_t)t * H + tid] = tcv;
                hs[(size_t)(t + 1) * H + tid] = h;
                hl[tid] = h;
                cprev = c;
            }
            lstm_lds_barrier();
        }
        __syncthreads();

        // ---- c. read-out, the loss before this step and its gradient
        double lsum = 0.0;
        cnn_forward(hs + H, Pfc, T, H, n_out, H, wave, lane, [&](int t, int o, double z) {
            const double diff = z - (Dg[(size_t)t * n_out + o] * (tsc ? tsc[o] : 1.0) + (tsh ? tsh[o] : 0.0));
            const bool on = t >= transient;
            dys[(size_t)t * n_out + o] = on ? diff * gscale : 0.0;
            if (on) lsum += diff * diff;
        });
        __syncthreads();

        // ---- d. backward sweep (dzl is zero: dz[T] = 0)
        double dcn = 0.0;
        for (int t = T - 1; t >= 0; --t) {
            double gi = 0.0, gf = 0.0, gg = 0.0, go = 0.0, cp = 0.0, tcv = 0.0, dh = 0.0;
            if (unit) {
                const double* gt = gates + (size_t)t * H4 + tid;
                gi = gt[0]; gf = gt[H]; gg = gt[2 * H]; go = gt[3 * H];
                cp = cs[(size_t)t * H + tid];
                tcv = tcs[(size_t)t * H + tid];
                for (int o = 0; o < n_out; ++o) dh = fma(Pfc[(size_t)o * KH + tid], dys[(size_t)t * n_out + o], dh);
            }
            double qk[CKT], qx[NX];
#pragma unroll
            for (int k = 0; k < CKT; ++k) qk[k] = 0.0;
#pragma unroll
            for (int k = 0; k < NX; ++k) qx[k] = 0.0;
#pragma unroll
            for (int j = 0; j < RJ; ++j) {
                const int r = tr + 64 * j;
                const double dv = dzl[r & 511];
#pragma unroll
                for (int k = 0; k < CKR; ++k) qk[k] = fma(Wr[j][k], dv, qk[k]);
#pragma unroll
                for (int k = 0; k < CKL; ++k) qk[CKR + k] = fma(Wl[j * CKL + k][tid], dv, qk[CKR + k]);
#pragma unroll
                for (int k = 0; k < NX; ++k) {
                    const int c = tc + 8 * (CKT + k);
                    if (CKT + k < CK) qx[k] = fma(lstm_whh(Phh, r, c, H), dv, qx[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < CKT; ++k) {
#pragma unroll
                for (int d = 8; d <= 32; d <<= 1) qk[k] += __shfl_xor(qk[k], d);
                if (lane < 8) red[wave][tc + 8 * k] = qk[k];
            }
#pragma unroll
            for (int k = 0; k < NX; ++k) {
#pragma unroll
                for (int d = 8; d <= 32; d <<= 1) qx[k] += __shfl_xor(qx[k], d);
                if (lane < 8) red[wave][tc + 8 * (CKT + k)] = qx[k];
            }
            lstm_lds_barrier();
            if (unit) {
                double rec = 0.0;
#pragma unroll
                for (int e = 0; e < CNN_WAVES; ++e) rec += red[e][tid];
                dh += rec;
                const double d_o = dh * tcv, dc = dcn + dh * go * (1.0 - tcv * tcv);
                const double di = dc * gg, dg = dc * gi, df = dc * cp;
                dcn = dc * gf;
                const double zi = di * gi * (1.0 - gi), zf = df * gf * (1.0 - gf), zg = dg * (1.0 - gg * gg),
                             zo = d_o * go * (1.0 - go);
                double* dt = dz + (size_t)t * H4 + tid;
                dt[0] = zi; dt[H] = zf; dt[2 * H] = zg; dt[3 * H] = zo;
                dzl[tid] = zi; dzl[H + tid] = zf; dzl[2 * H + tid] = zg; dzl[3 * H + tid] = zo;
            }
            lstm_lds_barrier();
        }
        __syncthreads();

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
        // ---- e. weight gradients and Adam, the strips of the three layers in one list (the heaviest layer first)
        b1pow *= p.beta1;
        b2pow *= p.beta2;
        const CnnAdam ad = {p.beta1, p.beta2, p.lr / (1.0 - b1pow), sqrt(1.0 - b2pow), p.eps, ep == 0};
        int base = 0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int l = q == 0 ? 1 : (q == 1 ? 0 : 2);
            const double* dzp = l == 2 ? dys : dz;
            const double* xp = l == 0 ? X : (l == 1 ? hs : hs + H);
            const int n_strips = cnn_weight_grad_strips(w.ci[l], w.co[l], 1);
            for (int sl = (wave - base % CNN_WAVES + CNN_WAVES) % CNN_WAVES; sl < n_strips; sl += CNN_WAVES)
                cnn_weight_grad_strip(sl, dzp, xp, ws + w.prm[l], ws + w.m[l], ws + w.v[l], T, w.ci[l], w.co[l], 1, lane,
                                      ad);
            base += n_strips;
        }
        __syncthreads();
    }

#pragma unroll
    for (int l = 0; l < 3; ++l)
        lstm_store_params(ws + w.prm[l], p.W[l] + (size_t)g * w.co[l] * w.ci[l], p.b[l] + (size_t)g * w.co[l], w.ci[l],
                          w.co[l], tid);
}

// B[k][column] of the prediction's step product for lane `lane` of k-step ks, unit tile ut, gate q: k-steps below ksh are
// W_hh, the others [W_ih | b_ih + b_hh]; zero beyond the ends
__device__ __forceinline__ double lstm_b_elem(const LstmParams& p, int g, const LstmPred& pd, int ut, int q, int ks, int lane) {
    const int H = p.n_hidden, n_in = p.n_in, u = 16 * ut + (lane & 15);
    if (u >= H) return 0.0;
    const size_t row = (size_t)g * 4 * H + (size_t)q * H + u;
    if (ks < pd.ksh) {
        const int k = 4 * ks + (lane >> 4);
        return k < H ? p.W0[1][row * H + k] : 0.0;
    }
    const int k = 4 * (ks - pd.ksh) + (lane >> 4);
    return k < n_in ? p.W0[0][row * n_in + k] : (k == n_in ? p.b0[0][row] + p.b0[1][row] : 0.0);
}

__global__ __launch_bounds__(LSTM_THREADS) void lstm_predict_kernel(LstmParams p) {
    extern __shared__ __attribute__((aligned(16))) char lsm[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    const int H = p.n_hidden, n_in = p.n_in, n_out = p.n_out, T = p.T, T_in = p.T_in, fpg = p.frames_per_group;
    const int rows_out = T - p.transient;
    const LstmPred pd = lstm_pred(n_in, H);
    double* hl = reinterpret_cast<double*>(lsm);           // [16][pd.hs]
    double* Bl = hl + 16 * pd.hs;                          // [n_ut][nlds][4][64]
    double* Bs = p.workspace + (size_t)blockIdx.x * pd.scratch;   // [n_ut][kstream][4][64]
    const int tpg = (fpg + 15) / 16, n_groups = (p.n_frames + fpg - 1) / fpg;
    const long long n_tiles = (long long)n_groups * tpg;
    const int ut = wave, kfc = (H + 1 + 3) / 4;
    const bool owner = ut < pd.n_ut;

    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int g = (int)(tile / tpg);
        const long long f0 = (long long)g * fpg + 16 * (tile - (long long)g * tpg);
        long long fend = (long long)(g + 1) * fpg;
        if (fend > p.n_frames) fend = p.n_frames;
        if (f0 >= fend) continue;                          // (workgroup-uniform: a tile of the ragged last group)
        const int nv = fend - f0 < 16 ? (int)(fend - f0) : 16;
        // ---- this group's B: registers, LDS, and the streamed image in the workgroup's scratch
        for (int e = tid; e < pd.n_ut * pd.kstream * 256; e += LSTM_THREADS) {
            const int l = e & 63, q = (e >> 6) & 3, r = e >> 8, u = r / pd.kstream, si = r - u * pd.kstream;
            Bs[e] = lstm_b_elem(p, g, pd, u, q, pd.nreg + pd.nlds + si, l);
        }
        for (int e = tid; e < pd.n_ut * pd.nlds * 256; e += LSTM_THREADS) {
            const int l = e & 63, q = (e >> 6) & 3, r = e >> 8, u = r / pd.nlds, si = r - u * pd.nlds;
            Bl[e] = lstm_b_elem(p, g, pd, u, q, pd.nreg + si, l);
        }
        double Br[LSTM_KREG][4];
#pragma unroll
        for (int ks = 0; ks < LSTM_KREG; ++ks) {
#pragma unroll
            for (int q = 0; q < 4; ++q) Br[ks][q] = (owner && ks < pd.nreg) ? lstm_b_elem(p, g, pd, ut, q, ks, lane) : 0.0;
        }
        for (int e = tid; e < 16 * pd.hs; e += LSTM_THREADS) hl[e] = 0.0;
        const double* isc = p.in_scale ? p.in_scale + (size_t)g * n_in : nullptr;
        const double* ish = p.in_shift ? p.in_shift + (size_t)g * n_in : nullptr;
        const double* tsc = p.t_scale ? p.t_scale + (size_t)g * n_out : nullptr;
        const double* tsh = p.t_shift ? p.t_shift + (size_t)g * n_out : nullptr;
        const double* Wfc = p.W0[2] + (size_t)g * n_out * H;
        const double* bfc = p.b0[2] + (size_t)g * n_out;
        const double* Ua = p.U + (size_t)(f0 + (lr < nv ? lr : nv - 1)) * T_in * n_in;   // the frame of this lane's A row
        double cst[4] = {0.0, 0.0, 0.0, 0.0};
        __syncthreads();

        for (int t = 0; t <= T; ++t) {
            // ---- the read-out of step t - 1 (its h is in LDS until this step's first barrier)
            if (wave == CNN_WAVES - 1 && t > 0 && t - 1 >= p.transient) {
                cnn_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
                const int o = lr < n_out ? lr : n_out - 1;
                for (int ks = 0; ks < kfc; ++ks) {
                    const int k = 4 * ks + lq;
                    const double a = k < H ? hl[lr * pd.hs + k] : (k == H ? 1.0 : 0.0);
                    const double b = k < H ? Wfc[(size_t)o * H + k] : (k == H ? bfc[o] : 0.0);
                    acc = cnn_mfma(a, b, acc);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = 4 * i + lq;
                    if (row < nv && lr < n_out)
                        p.Y[((size_t)(f0 + row) * rows_out + (t - 1 - p.transient)) * n_out + lr] =
                            (acc[i] - (tsh ? tsh[lr] : 0.0)) / (tsc ? tsc[lr] : 1.0);
                }
            }
            if (t == T) break;
            double hv[4] = {0.0, 0.0, 0.0, 0.0};
            if (owner) {
                cnn_f64x4 acc[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = cnn_f64x4{0.0, 0.0, 0.0, 0.0};
                const double* ha = hl + lr * pd.hs + lq;
#pragma unroll
                for (int ks = 0; ks < LSTM_KREG; ++ks) {
                    if (ks < pd.nreg) {
                        const double a = ha[4 * ks];
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[q] = cnn_mfma(a, Br[ks][q], acc[q]);
                    }
                }
                const double* bl = Bl + (size_t)ut * pd.nlds * 256 + lane;
                for (int si = 0; si < pd.nlds; ++si) {
                    const double a = ha[4 * (pd.nreg + si)];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = cnn_mfma(a, bl[si * 256 + q * 64], acc[q]);
                }
                const double* bs = Bs + (size_t)ut * pd.kstream * 256 + lane;
                const int hstream = pd.kstream - pd.ksx;
                for (int si = 0; si < hstream; ++si) {
                    const double a = ha[4 * (pd.nreg + pd.nlds + si)];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = cnn_mfma(a, bs[si * 256 + q * 64], acc[q]);
                }
                for (int kx = 0; kx < pd.ksx; ++kx) {
                    const int k = 4 * kx + lq;
                    double a = k == n_in ? 1.0 : 0.0;
                    if (k < n_in) a = (t < T_in ? Ua[(size_t)t * n_in + k] : 0.0) * (isc ? isc[k] : 1.0) + (ish ? ish[k] : 0.0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = cnn_mfma(a, bs[(hstream + kx) * 256 + q * 64], acc[q]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double gi = lstm_sigma(acc[0][i]), gf = lstm_sigma(acc[1][i]), gg = tanh(acc[2][i]),
                                 go = lstm_sigma(acc[3][i]);
                    cst[i] = gf * cst[i] + gi * gg;
                    hv[i] = go * tanh(cst[i]);
                }
            }
            lstm_lds_barrier();                            // every wave has read h[t-1]
            if (owner && 16 * ut + lr < H) {
#pragma unroll
                for (int i = 0; i < 4; ++i) hl[(4 * i + lq) * pd.hs + 16 * ut + lr] = hv[i];
            }
            lstm_lds_barrier();
        }
        __syncthreads();                                   // the next tile overwrites LDS and the scratch
    }
}

int launch_lstm_train(const LstmParams& p, hipStream_t stream) {
    if (p.n_hidden <= 104)
        hipLaunchKernelGGL((lstm_train_kernel<7, 9, 4>), dim3((unsigned)p.n_groups), dim3(LSTM_THREADS), 0, stream, p);
    else
        hipLaunchKernelGGL((lstm_train_kernel<8, 8, 4>), dim3((unsigned)p.n_groups), dim3(LSTM_THREADS), 0, stream, p);
    return (int)hipGetLastError();
}

int launch_lstm_predict(const LstmParams& p, hipStream_t stream) {
    static std::atomic<unsigned long long> raised{0};
    const int e = raise_dynamic_lds_once(reinterpret_cast<const void*>(lstm_predict_kernel), LSTM_LDS, raised);
    if (e) return e;
    const int fpg = p.frames_per_group, tpg = (fpg + 15) / 16, n_groups = (p.n_frames + fpg - 1) / fpg;
    const long long n_tiles = (long long)n_groups * tpg;
    int wgs = p.n_frames < LSTM_PRED_WGS ? p.n_frames : LSTM_PRED_WGS;     // the scratch regions there are
    if (n_tiles < wgs) wgs = (int)n_tiles;
    hipLaunchKernelGGL(lstm_predict_kernel, dim3((unsigned)wgs), dim3(LSTM_THREADS), lstm_pred(p.n_in, p.n_hidden).lds_bytes,
                       stream, p);
    return (int)hipGetLastError();
}

}  // namespace esn
