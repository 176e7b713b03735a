// Hold-out choice of the ridge parameter: one workgroup per trained ESN scores every candidate read-out
// on a pilot the fit has not seen,
//
//   r[i][j] = sum_c E[i][c] W[j][c] - D_s[i][o],   j = l n_out + o,   score[l] = sum_i sum_o r[i][l n_out + o]^2,
//
// and picks the lowest l with the smallest finite score.  All n_ridge * n_out <= 128 read-out rows form the B operand of
// one [rows x cols] by [cols x 128] float64 product on the matrix pipe (v_mfma_f64_16x16x4_f64): E and W are streamed
// through LDS in chunks of HO_KC columns, every byte of them read once per group while the held-out segment has at most
// HO_M rows (W once per HO_M rows beyond that).  The next chunk's global loads are in flight while the current one is
// multiplied.  Every sum runs in an order fixed by the shape alone -- the k order of the chunks, the accumulator
// registers in index order, a fixed xor tree over the lanes, the two wave rows, the outputs in ascending order -- so a
// group's scores and choice do not depend on the batch it is scored in; there are no atomics.
#include "esn_common.h"
#include "esn_launch.h"
#include "esn_stage.h"

namespace esn {

constexpr int HO_NT = 512;                  // threads: 8 waves, 2 (rows) x 4 (columns) of 64 x 32 results each
constexpr int HO_M = 128;                   // held-out rows per pass
constexpr int HO_N = 128;                   // n_ridge * n_out at most (16 x 8)
constexpr int HO_KC = 32;                   // columns per chunk
// LDS row stride (doubles): rows 16-byte aligned, and HO_LD % 32 == 2 puts the 32 lanes of a ds_read_b64 group
// (16 rows x 2 consecutive k) on 32 different bank pairs
constexpr int HO_LD = HO_KC + 2;
constexpr int HO_PER = HO_M * HO_KC / HO_NT;                // staged elements per thread and operand: 8
// LDS (doubles): two buffers of { E chunk [HO_M][HO_LD] | W chunk [HO_N][HO_LD] } | column sums [2][HO_N] | scores [16].
// One workgroup per CU: the 64 accumulator registers and the 32 of the chunk in flight leave room for two waves per SIMD.
constexpr int HO_OFF_W = HO_M * HO_LD;
constexpr int HO_BUF = HO_OFF_W + HO_N * HO_LD;
constexpr int HO_OFF_P = 2 * HO_BUF;
constexpr int HO_OFF_S = HO_OFF_P + 2 * HO_N;
constexpr size_t HO_LDS = sizeof(double) * (size_t)(HO_OFF_S + 16);             // 141 440 B
static_assert(HO_M == HO_N, "one staging routine serves both operands");
static_assert(HO_LD % 2 == 0 && HO_LD % 32 == 2 && HO_BUF % 2 == 0, "aligned rows, conflict-free fragment reads");
static_assert(HO_LDS <= 160 * 1024, "the LDS of a CU");

typedef double ho_f64x4 __attribute__((ext_vector_type(4)));

struct HoldoutParams {
    const double* E; const float* E32; const double* D; const double* W;
    int T, transient, cols, n_out, n_ridge;
    const double* t_scale; const double* t_shift; const int* status_in;
    double* score; int* choice;
};

// Rows [0, n_rows) x columns [k0, k0 + HO_KC) of a row-major [.][cols] matrix into registers, zero outside it.  Every
// lane loads -- from a clamped, valid address -- and the zero is a select, so no load sits behind a branch.
template <typename T, int V>
__device__ __forceinline__ void ho_load(const T* __restrict__ base, int n_rows, int cols, int k0, int tid,
                                        double (&r)[HO_PER]) {
    constexpr int UPR = HO_KC / V;          // units per row
#pragma unroll
    for (int u = 0; u < HO_PER / V; ++u) {
        const int e = tid + HO_NT * u, i = e / UPR, k = k0 + (e % UPR) * V;
        const bool in = i < n_rows && k < cols;
        double v[V];
        stage_fetch(base + (size_t)(i < n_rows ? i : n_rows - 1) * cols + (k < cols ? k : 0), v);
#pragma unroll
        for (int x = 0; x < V; ++x) r[u * V + x] = in ? v[x] : 0.0;
    }
}

template <int V>
__device__ __forceinline__ void ho_store(double* __restrict__ dst, int tid, const double (&r)[HO_PER]) {
    constexpr int UPR = HO_KC / V;
#pragma unroll
    for (int u = 0; u < HO_PER / V; ++u) {
        const int e = tid + HO_NT * u, i = e / UPR, kk = (e % UPR) * V;
        double* d = dst + i * HO_LD + kk;
        if constexpr (V == 1) {
            d[0] = r[u];
        } else {
#pragma unroll
            for (int x = 0; x < V; x += 2)
                *reinterpret_cast<stage_f64x2*>(d + x) = stage_f64x2{r[u * V + x], r[u * V + x + 1]};
        }
    }
}

template <typename TE, bool VEC>
__global__ __launch_bounds__(HO_NT) void holdout_score_kernel(HoldoutParams sp) {
    extern __shared__ __attribute__((aligned(16))) char ho_smem[];
    double* Es = reinterpret_cast<double*>(ho_smem);                // [HO_M][HO_LD]
    double* Ws = Es + HO_OFF_W;                                     // [HO_N][HO_LD]
    double* Ps = Es + HO_OFF_P;                                     // [2][HO_N] column sums of the two wave rows
    double* Ss = Es + HO_OFF_S;                                     // [16] scores
    constexpr int VE = StageUnit<TE, VEC>::V, VW = StageUnit<double, VEC>::V;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int wr = wv >> 2, wc = wv & 3;                            // the wave's 64 rows and 32 columns of the product
    const int rows = sp.T - sp.transient, cols = sp.cols, nrhs = sp.n_out, L = sp.n_ridge, N = L * nrhs;
    const TE* Eg = stage_src(sp, (TE*)nullptr) + ((size_t)g * sp.T + sp.transient) * cols;       // [rows][cols]
    const double* Wg = sp.W + (size_t)g * N * cols;                                            // [N][cols]
    const double* Dg = sp.D + ((size_t)g * sp.T + sp.transient) * nrhs;

    // v_mfma_f64_16x16x4_f64: A[l % 16][l / 16], B[l / 16][l % 16], C reg i: row 4 i + l / 16, col l % 16.  This lane's
    // two result columns j (read-out rows of W), their output and its teacher scaling:
    int jo[2];
    double sc[2], sh[2], colsum[2] = {0.0, 0.0};
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int j = wc * 32 + ct * 16 + lr;
        jo[ct] = j < N ? j % nrhs : -1;
        sc[ct] = (j < N && sp.t_scale) ? sp.t_scale[(size_t)g * nrhs + jo[ct]] : 1.0;
        sh[ct] = (j < N && sp.t_shift) ? sp.t_shift[(size_t)g * nrhs + jo[ct]] : 0.0;
    }

    for (int r0 = 0; r0 < rows; r0 += HO_M) {
        const int mrows = rows - r0 < HO_M ? rows - r0 : HO_M;
        const TE* Eb = Eg + (size_t)r0 * cols;
        const bool wave_on = wr * 64 < mrows && wc * 32 < N;        // (the other waves only stage)
        ho_f64x4 acc[4][2];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[q][ct] = ho_f64x4{0.0, 0.0, 0.0, 0.0};
        // Two LDS buffers, one barrier per chunk: while chunk c is multiplied out of buffer c % 2, chunk c + 1 (in
        // registers since the previous trip) goes to the other buffer and the loads of chunk c + 2 are issued.
        double re[HO_PER], rw[HO_PER];
        ho_load<TE, VE>(Eb, mrows, cols, 0, tid, re);
        ho_load<double, VW>(Wg, N, cols, 0, tid, rw);
        __syncthreads();                                            // (the previous pass has read both buffers out)
        ho_store<VE>(Es, tid, re);
        ho_store<VW>(Ws, tid, rw);
        if (HO_KC < cols) {
            ho_load<TE, VE>(Eb, mrows, cols, HO_KC, tid, re);
            ho_load<double, VW>(Wg, N, cols, HO_KC, tid, rw);
        }
        __syncthreads();
        int buf = 0;
        for (int k0 = 0; k0 < cols; k0 += HO_KC, buf ^= 1) {
            if (k0 + HO_KC < cols) {                                // buffer buf ^ 1 was read out before the last barrier
                ho_store<VE>(Es + (buf ^ 1) * HO_BUF, tid, re);
                ho_store<VW>(Ws + (buf ^ 1) * HO_BUF, tid, rw);
            }
            if (k0 + 2 * HO_KC < cols) {                            // in flight during the product
                ho_load<TE, VE>(Eb, mrows, cols, k0 + 2 * HO_KC, tid, re);
                ho_load<double, VW>(Wg, N, cols, k0 + 2 * HO_KC, tid, rw);
            }
            if (wave_on) {
                const double* ea = Es + buf * HO_BUF + (wr * 64 + lr) * HO_LD + lq;
                const double* wb = Ws + buf * HO_BUF + (wc * 32 + lr) * HO_LD + lq;
#pragma unroll
                for (int k4 = 0; k4 < HO_KC; k4 += 4) {             // (columns past `cols` are zero in both operands)
                    const double b0 = wb[k4], b1 = wb[16 * HO_LD + k4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const double a = ea[q * 16 * HO_LD + k4];
                        acc[q][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc[q][0], 0, 0, 0);
                        acc[q][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc[q][1], 0, 0, 0);
                    }
                }
            }
            __syncthreads();                                        // chunk c is read out, chunk c + 1 is in place
        }
        // residuals of this pass, squared into the lane's two column sums: row tiles, then registers, ascending
        if (wave_on) {
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                if (jo[ct] < 0) continue;
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int i4 = 0; i4 < 4; ++i4) {
                        const int i = wr * 64 + q * 16 + 4 * i4 + lq;
                        if (i < mrows) {
                            const double r = acc[q][ct][i4] - (Dg[(size_t)(r0 + i) * nrhs + jo[ct]] * sc[ct] + sh[ct]);
                            colsum[ct] = fma(r, r, colsum[ct]);
                        }
                    }
            }
        }
    }

    // rows l / 16 = 0 .. 3 of a column meet in a fixed xor tree; then the two wave rows and the outputs in order
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        double v = colsum[ct];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (lq == 0) Ps[wr * HO_N + wc * 32 + ct * 16 + lr] = v;
    }
    __syncthreads();
    if (tid < L) {
        double s = 0.0;
        for (int o = 0; o < nrhs; ++o) {
            s += Ps[tid * nrhs + o];
            s += Ps[HO_N + tid * nrhs + o];
        }
        const bool ok = (!sp.status_in || sp.status_in[(size_t)g * L + tid] == 0) && fabs(s) <= 1.7976931348623157e308;
        s = ok ? s : __builtin_inf();
        Ss[tid] = s;
        sp.score[(size_t)g * L + tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double best = __builtin_inf();
        int best_l = -1;
        for (int l = 0; l < L; ++l)
            if (Ss[l] < best) {             // strict: the lowest index wins a tie; inf never wins
                best = Ss[l];
                best_l = l;
            }
        sp.choice[g] = best_l;
    }
}

int launch_holdout_score(const HoldoutArgs& a) {
    if (a.n_out > 8 || a.n_ridge > 16 || a.n_ridge * a.n_out > HO_N) return -1;
    const HoldoutParams sp = {a.E, a.E32, a.D, a.W, a.T, a.transient, a.cols, a.n_out, a.n_ridge,
                              a.t_scale, a.t_shift, a.status_in, a.score, a.choice};
    const bool vec = a.cols % 4 == 0;
    void (*fn)(HoldoutParams) = a.E32 ? (vec ? holdout_score_kernel<float, true> : holdout_score_kernel<float, false>)
                                      : (vec ? holdout_score_kernel<double, true> : holdout_score_kernel<double, false>);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)HO_LDS);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fn, dim3(a.n_groups), dim3(HO_NT), HO_LDS, a.stream, sp);
    return (int)hipGetLastError();
}

}  // namespace esn
