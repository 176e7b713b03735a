// Decision-directed channel estimate for the MMSE baseline under Doppler (include/esn_hip.h: esn_channel_track): the
// isi taps of every link, least squares with a per-tap prior, from `window` received data frames and the points that
// were decided (or sent) on them -- one workgroup per estimate, everything in LDS, float64:
//   Y_w   = FFT_N(y_w[cp:]) / (N sqrt(Pi))                  the transform and scale of the detector tail
//   X_w   = nearest unit-power QAM point of X_hat (the tail's slicer), or the point of the given bits
//   R[t,t',d] = sum_w sum_k conj(X_w[k,t]) X_w[k,t'] w^{kd}, d = 0 .. isi-1      w = exp(-2 pi i / N)
//   b[(t,l),r] = sum_w sum_k conj(X_w[k,t]) w^{-kl} Y_w[k,r]
//   G[(t,l),(t',l')] = R[t,t',l'-l] (l' >= l), conj(R[t',t,l-l']) (l' < l), + reg[l] on the diagonal: block-Toeplitz,
//                      n_t^2 isi lag sums instead of (n_t isi)^2 entries
//   c = G^-1 b   root-free Cholesky (G = L D L^H), all n_r right-hand sides at once;   H[k,r,t] = sum_l c[r,t,l] w^{kl}
// Order of every sum: a thread owns one (t, r) or (t, t') pair and one of S contiguous ranges of k and adds frame after
// frame, k ascending, into isi accumulators; the S partial sums join pairwise (range s + h into range s, h = S/2 .. 1).
// S depends on the shape alone, so an estimate is bitwise the same alone or inside any launch.  No atomics.
#include <atomic>
#include "esn_common.h"
#include "esn_launch.h"
#include "esn_ofdm_math.h"

namespace esn {

constexpr int CT_MAX_ISI = 16;         // accumulators a thread keeps in registers
constexpr int CT_MAX_THREADS = 384;
constexpr size_t CT_MAX_LDS = 150 * 1024;

static inline int ct_pairs(int n_t, int n_r) { return n_t * n_r + n_t * n_t; }
static inline int ct_pow2_up(int v) { int p = 1; while (p < v) p <<= 1; return p; }

// k ranges per pair: as many as the workgroup has threads for, a power of two, at most 16 and at most N
int chantrack_segments(int n_sub, int n_t, int n_r) {
    int s = 16;
    while (s > 1 && (s > n_sub || ct_pairs(n_t, n_r) * s > CT_MAX_THREADS)) s >>= 1;
    return s;
}

// LDS image in double2: twiddles [N] | spectra [n_r][N + 1], decisions [N][n_t] (later the joined sums) |
// partial sums [S/2][pairs][isi], later G [M][M2 + 1], right-hand sides [M][8] and (as doubles) the diagonal [M]
static inline size_t ct_work_elems(int n_sub, int n_t, int n_r, int isi) {
    const int M = n_t * isi, S = chantrack_segments(n_sub, n_t, n_r);
    const size_t part = (size_t)(S / 2) * ct_pairs(n_t, n_r) * isi;
    const size_t solve = (size_t)M * (ct_pow2_up(M) + 1) + (size_t)M * 8 + (M + 1) / 2;
    return part > solve ? part : solve;
}
size_t chantrack_lds_bytes(int n_sub, int n_t, int n_r, int isi) {
    return sizeof(double2) * ((size_t)n_sub + (size_t)n_r * (n_sub + 1) + (size_t)n_sub * n_t
                              + ct_work_elems(n_sub, n_t, n_r, isi));
}

__device__ __forceinline__ double2 ct_cmul(const double2 a, const double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ void ct_csub(double2& a, const double2 b) { a.x -= b.x; a.y -= b.y; }

__global__ __launch_bounds__(CT_MAX_THREADS) void channel_track_kernel(ChanTrackParams cp) {
    extern __shared__ __attribute__((aligned(16))) char tsm[];
    const int N = cp.n_sub, n_t = cp.n_t, n_r = cp.n_r, L = cp.isi, m = cp.m, S = cp.n_seg;
    const int T = N + cp.cp, ld = N + 1, mask = N - 1;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int PB = n_t * n_r, P = PB + n_t * n_t, M = n_t * L;
    const int lg = cp.log2m2, M2 = 1 << lg, ldg = M2 + 1;
    double2* om = reinterpret_cast<double2*>(tsm);        // [N]  w^j = exp(-2 pi i j / N)
    double2* Yf = om + N;                                  // [n_r][ld]
    double2* Xs = Yf + (size_t)n_r * ld;                   // [N][n_t]
    double2* tot = Yf;                                     // [P][L]  the joined sums, once the frames are done with
    double2* work = Xs + (size_t)N * n_t;
    double2* part = work;                                  // [S/2][P][L]
    double2* Gm = work;                                    // [M][ldg]  lower triangle
    double2* bm = Gm + (size_t)M * ldg;                    // [M][8]
    double* diag0 = reinterpret_cast<double*>(bm + (size_t)M * 8);   // [M]
    const int est = blockIdx.x, group = est / cp.est_per_group;
    const double scale = det_scale(N, cp.p_i[group]);
    const int side = 1 << (m / 2);
    const double norm = det_norm(side);

    ofdm_twiddles(om, N, N, -1.0);                         // (the lag sums read the upper half too)

    // the sum this thread owns: pair (b: t, r; lag: t, t') and k range
    const int seg = tid / P, pair = tid - seg * P;
    const bool owner = seg < S;
    const bool is_b = pair < PB;
    const int pa = is_b ? pair / n_r : (pair - PB) / n_t;                 // t
    const int pb = is_b ? pair - pa * n_r : (pair - PB) - pa * n_t;       // r, or t'
    const int k_lo = seg * (N / S), k_hi = k_lo + N / S;
    double2 acc[CT_MAX_ISI];
#pragma unroll
    for (int l = 0; l < CT_MAX_ISI; ++l) acc[l] = make_double2(0.0, 0.0);

    for (int w = 0; w < cp.window; ++w) {
        const size_t frame = (size_t)est * cp.window + w;
        const double2* y = reinterpret_cast<const double2*>(cp.y_cp) + (frame * T + cp.cp) * n_r;
        for (int e = tid; e < N * n_r; e += nthr) {        // rows cp .. cp + N - 1 are one contiguous run
            const int row = e / n_r, r = e - row * n_r;
            const int rv = (int)(__brev((unsigned)row) >> (32 - cp.log2n));
            Yf[r * ld + rv] = y[e];
        }
        if (cp.X_hat) {
            const double2* xh = reinterpret_cast<const double2*>(cp.X_hat) + frame * N * n_t;
            for (int e = tid; e < N * n_t; e += nthr) {
                const double2 v = xh[e];
                Xs[e] = make_double2(det_level(det_slice(v.x, norm, side), side, norm),
                                     det_level(det_slice(v.y, norm, side), side, norm));
            }
        } else {
            const uint8_t* bt = cp.bits + frame * N * m * n_t;
            for (int e = tid; e < N * n_t; e += nthr) {
                const int k = e / n_t, t = e - k * n_t;
                const int idx = det_bits_index(bt + (size_t)k * m * n_t + t, n_t, m);
                Xs[e] = make_double2(det_level(idx >> (m / 2), side, norm), det_level(idx & (side - 1), side, norm));
            }
        }
        __syncthreads();
        ofdm_fft_lds(Yf, n_r, ld, om, N, cp.log2n);        // (reads om[0 .. N/2))
        if (owner) {
            const double sgn = is_b ? -1.0 : 1.0;          // b takes w^{-kl}, the lag sums w^{kd}
            for (int k = k_lo; k < k_hi; ++k) {
                const double2 xa = Xs[k * n_t + pa];
                double2 o;
                if (is_b) {
                    const double2 yv = Yf[pb * ld + k];
                    o = make_double2(yv.x * scale, yv.y * scale);
                } else {
                    o = Xs[k * n_t + pb];
                }
                const double2 z = ct_cmul(make_double2(xa.x, -xa.y), o);
                int j = 0;
#pragma unroll
                for (int l = 0; l < CT_MAX_ISI; ++l) {
                    if (l < L) {
                        const double2 tw = om[j];
                        const double ty = sgn * tw.y;
                        acc[l].x = fma(-z.y, ty, fma(z.x, tw.x, acc[l].x));
                        acc[l].y = fma(z.y, tw.x, fma(z.x, ty, acc[l].y));
                        j = (j + k) & mask;
                    }
                }
            }
        }
        __syncthreads();
    }

    // join the k ranges: range s + h into range s
    for (int h = S >> 1; h >= 1; h >>= 1) {
        if (owner && seg >= h && seg < 2 * h) {
#pragma unroll
            for (int l = 0; l < CT_MAX_ISI; ++l)
                if (l < L) part[((size_t)(seg - h) * P + pair) * L + l] = acc[l];
        }
        __syncthreads();
        if (owner && seg < h) {
#pragma unroll
            for (int l = 0; l < CT_MAX_ISI; ++l) {
                if (l < L) {
                    const double2 v = part[((size_t)seg * P + pair) * L + l];
                    acc[l].x += v.x; acc[l].y += v.y;
                }
            }
        }
        __syncthreads();
    }
    if (owner && seg == 0) {
#pragma unroll
        for (int l = 0; l < CT_MAX_ISI; ++l)
            if (l < L) tot[pair * L + l] = acc[l];
    }
    __syncthreads();

    // G (lower triangle) from the lag sums, the right-hand sides, the diagonal as it stood
    const double* reg = cp.reg + (size_t)group * L;
    for (int e = tid; e < M2 * M2; e += nthr) {
        const int i = e >> lg, c = e & (M2 - 1);
        if (c <= i && i < M) {
            const int t = i / L, l = i - t * L, t2 = c / L, l2 = c - t2 * L;
            double2 v;
            if (l2 >= l) {
                v = tot[(PB + t * n_t + t2) * L + (l2 - l)];
            } else {
                v = tot[(PB + t2 * n_t + t) * L + (l - l2)];
                v.y = -v.y;
            }
            if (c == i) {
                v.x += reg[l];
                diag0[i] = v.x;
            }
            Gm[i * ldg + c] = v;
        }
    }
    for (int e = tid; e < M * 8; e += nthr) {
        const int i = e >> 3, r = e & 7;
        if (r < n_r) {
            const int t = i / L, l = i - t * L;
            bm[e] = tot[(t * n_r + r) * L + l];
        }
    }
    __syncthreads();

    // G = L D L^H column by column; the stored column j is L[:, j] D_j; the right-hand sides ride along
    // (forward substitution).  Every thread reads the same pivot, so the exit is uniform.
    int fail = 0;
    for (int j = 0; j < M; ++j) {
        const double d = Gm[j * ldg + j].x;
        if (!(fabs(d) <= 1.7976931348623157e308) || !(d > 64.0 * 2.220446049250313e-16 * diag0[j])) {
            fail = 1;
            break;
        }
        const double inv = 1.0 / d;
        for (int e = tid; e < M2 * M2; e += nthr) {
            const int i = e >> lg, c = e & (M2 - 1);
            if (j < c && c <= i && i < M) {
                const double2 a = Gm[i * ldg + j], q = Gm[c * ldg + j];
                ct_csub(Gm[i * ldg + c], ct_cmul(make_double2(a.x * inv, a.y * inv), make_double2(q.x, -q.y)));
            }
        }
        for (int e = tid; e < M * 8; e += nthr) {
            const int i = e >> 3, r = e & 7;
            if (i > j && r < n_r) {
                const double2 a = Gm[i * ldg + j];
                ct_csub(bm[e], ct_cmul(make_double2(a.x * inv, a.y * inv), bm[j * 8 + r]));
            }
        }
        __syncthreads();
    }
    if (!fail) {
        // L^H c = D^-1 z, column-oriented from the last row up: bm[j] holds D_j (z_j / D_j - sum_{i>j} conj(L[i][j]) c_i)
        for (int i = M - 1; i > 0; --i) {
            const double inv = 1.0 / Gm[i * ldg + i].x;
            for (int e = tid; e < i * 8; e += nthr) {
                const int j = e >> 3, r = e & 7;
                if (r < n_r) {
                    const double2 z = bm[i * 8 + r], a = Gm[i * ldg + j];
                    ct_csub(bm[e], ct_cmul(make_double2(a.x, -a.y), make_double2(z.x * inv, z.y * inv)));
                }
            }
            __syncthreads();
        }
    }

    // taps and H: thread = (r, t) fixed, its isi taps in registers; consecutive lanes cover the [r][t] entries of a
    // subcarrier, 16 bytes each
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const int RT = n_r * n_t, per = nthr / RT;
    if (tid < per * RT) {
        const int k0 = tid / RT, rt = tid - k0 * RT;
        const int r = rt / n_t, t = rt - r * n_t;
        double2 c[CT_MAX_ISI];
#pragma unroll
        for (int l = 0; l < CT_MAX_ISI; ++l) {
            c[l] = make_double2(qnan, qnan);
            if (l < L && !fail) {
                const int i = t * L + l;
                const double inv = 1.0 / Gm[i * ldg + i].x;
                const double2 z = bm[i * 8 + r];
                c[l] = make_double2(z.x * inv, z.y * inv);
            }
        }
        if (cp.taps && k0 == 0) {
            double2* tp = reinterpret_cast<double2*>(cp.taps) + ((size_t)est * RT + rt) * L;
#pragma unroll
            for (int l = 0; l < CT_MAX_ISI; ++l)
                if (l < L) tp[l] = c[l];
        }
        double2* Ho = reinterpret_cast<double2*>(cp.H) + (size_t)est * N * RT + rt;
        for (int k = k0; k < N; k += per) {
            double2 h = make_double2(0.0, 0.0);
            int j = 0;
#pragma unroll
            for (int l = 0; l < CT_MAX_ISI; ++l) {
                if (l < L) {
                    const double2 tw = om[j];
                    h.x = fma(-c[l].y, tw.y, fma(c[l].x, tw.x, h.x));
                    h.y = fma(c[l].y, tw.x, fma(c[l].x, tw.y, h.y));
                    j = (j + k) & mask;
                }
            }
            if (fail) h = make_double2(qnan, qnan);
            Ho[(size_t)k * RT] = h;
        }
    }
    if (tid == 0) cp.status[est] = fail;
}

int launch_channel_track(const ChanTrackParams& cp_in, hipStream_t stream) {
    ChanTrackParams cp = cp_in;
    const size_t lds = chantrack_lds_bytes(cp.n_sub, cp.n_t, cp.n_r, cp.isi);
    if (lds > CT_MAX_LDS || cp.isi > CT_MAX_ISI) return -1;
    cp.n_seg = chantrack_segments(cp.n_sub, cp.n_t, cp.n_r);
    int lg = 0;
    while ((1 << lg) < cp.n_t * cp.isi) ++lg;
    cp.log2m2 = lg;
    int threads = round_up(ct_pairs(cp.n_t, cp.n_r) * cp.n_seg, 64);
    if (threads > CT_MAX_THREADS) return -1;
    // the LDS ceiling is raised once per device, to the most any shape may ask for: the tracking loop launches per symbol
    static std::atomic<unsigned long long> raised{0};
    const int e = raise_dynamic_lds_once(reinterpret_cast<const void*>(channel_track_kernel), CT_MAX_LDS, raised);
    if (e) return e;
    hipLaunchKernelGGL(channel_track_kernel, dim3(cp.n_est), dim3(threads), lds, stream, cp);
    return (int)hipGetLastError();
}

}  // namespace esn
