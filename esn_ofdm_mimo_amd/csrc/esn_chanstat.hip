// Channel rank / condition / capacity record of the block-fading drivers (OFDM_MIMO_2-2_NBF_LDPC.py:369-385), float64:
// per subcarrier k of every coherence block the singular values S of the true channel H_k [n_r][n_t], then
//
//   thr   = max(1e-2 s1^2, 10 No/Pi)         rank_k = #{ s_i^2 >= thr }                      (:379-380)
//   cond_k = s1 / max(s_min, 1e-12)                                                           (:381)
//   cap_k  = sum_i log2(1 + (Pi/No/n_t) s_i^2),   cap[b] = mean_k cap_k                       (:372,382-383)
//
//   channel_metrics_kernel<NT, NR>   one wave per coherence block, one matrix per lane.  The singular values come from
//       one-sided (Hestenes) complex Jacobi on the min(n_t, n_r) columns of H_k (of H_k^T when n_r < n_t: same singular
//       values) -- never from the eigenvalues of H^H H, which square the condition number s_min is read through.  The
//       matrix (at most 8 x 4 complex = 64 doubles) lives in registers.  A lane's matrix is 16 n_t n_r contiguous bytes,
//       so the wave's 64 matrices are staged through LDS: 16-byte loads, consecutive lanes on consecutive 16 bytes, at
//       most 256 bytes of every matrix per pass, rows padded by 16 bytes for the per-lane read-back.
//       <0, 0> is the generic instance (any n_t, n_r <= 8 with min <= 4): a zero-padded 8 x 4 problem read by strided
//       per-lane loads.
//
// Every lane's result depends on its own matrix only: a rotation is skipped, not blended, when the pair is orthogonal to
// working precision, so the sweeps a lane runs after it has converged (because another lane of the wave has not) leave
// it bitwise unchanged; the sweep count is bounded by MAX_SWEEPS whatever the input.  cap[b] is summed per lane in
// subcarrier order and then across the wave by a fixed butterfly: the same bits for a block alone or inside any batch.
#include "esn_common.h"
#include "esn_launch.h"

namespace esn {

constexpr int CS_MAX_SWEEPS = 16;        // 4 columns converge in 5-7 sweeps; the bound is what guarantees termination
constexpr double CS_TOL2 = 1e-30;        // rotate while |a_p^H a_q|^2 > TOL2 |a_p|^2 |a_q|^2

template <int NT, int NR>
struct ChanStatShape {
    static constexpr bool GENERIC = (NT == 0);
    static constexpr bool TRANSPOSED = !GENERIC && NR < NT;              // work on the columns of H^T
    static constexpr int C = GENERIC ? 4 : (NR < NT ? NR : NT);          // columns rotated
    static constexpr int R = GENERIC ? 8 : (NR < NT ? NT : NR);          // rows
    static constexpr int M = GENERIC ? 2 : 2 * NT * NR;                  // doubles per matrix
    static constexpr int SLAB = M < 32 ? M : 32;                         // doubles of a matrix staged per pass
    static constexpr int NSLAB = M / SLAB;
    static constexpr int STRIDE = SLAB + 2;                              // LDS row, padded by one 16-byte access
};

template <int NT, int NR>
__global__ __launch_bounds__(64) void channel_metrics_kernel(ChanStatParams cp) {
    using Sh = ChanStatShape<NT, NR>;
    constexpr int C = Sh::C, R = Sh::R;
    __shared__ __attribute__((aligned(16))) double stage[Sh::GENERIC ? 2 : 64 * Sh::STRIDE];
    const int lane = threadIdx.x, blk = blockIdx.x, N = cp.n_sub;
    const int n_t = Sh::GENERIC ? cp.n_t : NT, n_r = Sh::GENERIC ? cp.n_r : NR;
    const int n_s = n_t < n_r ? n_t : n_r;                               // singular values per matrix
    const double p_i = cp.p_i[blk];
    const double gam = (p_i / cp.no) / (double)n_t;
    const double thr_floor = 10.0 * (cp.no / p_i);
    const double* Hb = cp.H + (size_t)blk * N * (2 * n_t * n_r);
    double cap_acc = 0.0;

    for (int k0 = 0; k0 < N; k0 += 64) {
        const int k = k0 + lane;
        double ar[C][R], ai[C][R];
        if constexpr (Sh::GENERIC) {
            const bool tr = n_r < n_t;
            const int rows = tr ? n_t : n_r;
#pragma unroll
            for (int j = 0; j < C; ++j)
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const bool in = k < N && j < n_s && i < rows;
                    const int rx = tr ? j : i, tx = tr ? i : j;
                    const double* h = Hb + ((size_t)(k < N ? k : N - 1) * n_r * n_t + (in ? rx * n_t + tx : 0)) * 2;
                    ar[j][i] = in ? h[0] : 0.0;
                    ai[j][i] = in ? h[1] : 0.0;
                }
        } else {
            constexpr int CH = Sh::SLAB / 2;                             // 16-byte chunks of a matrix per pass
#pragma unroll
            for (int s = 0; s < Sh::NSLAB; ++s) {
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int c = i * 64 + lane, mtx = c / CH, off = c % CH;
                    double2 v = make_double2(0.0, 0.0);
                    if (k0 + mtx < N)
                        v = *reinterpret_cast<const double2*>(Hb + (size_t)(k0 + mtx) * Sh::M + s * Sh::SLAB + off * 2);
                    *reinterpret_cast<double2*>(stage + mtx * Sh::STRIDE + off * 2) = v;
                }
                __syncthreads();
#pragma unroll
                for (int e = 0; e < CH; ++e) {
                    const double2 v = *reinterpret_cast<const double2*>(stage + lane * Sh::STRIDE + e * 2);
                    const int idx = s * CH + e;                          // complex element of H_k: (rx, tx) = (idx / NT, idx % NT)
                    const int rx = idx / NT, tx = idx % NT;
                    if (Sh::TRANSPOSED) { ar[rx][tx] = v.x; ai[rx][tx] = v.y; }
                    else { ar[tx][rx] = v.x; ai[tx][rx] = v.y; }
                }
                __syncthreads();
            }
        }

        // exact power-of-two prescale to [1, 2): norms and products below neither overflow nor underflow
        double big = 0.0;
#pragma unroll
        for (int j = 0; j < C; ++j)
#pragma unroll
            for (int i = 0; i < R; ++i) big = fmax(big, fmax(fabs(ar[j][i]), fabs(ai[j][i])));
        int ex = 0;
        if (big > 0.0 && big < HUGE_VAL) {
            ex = ilogb(big);
#pragma unroll
            for (int j = 0; j < C; ++j)
#pragma unroll
                for (int i = 0; i < R; ++i) { ar[j][i] = ldexp(ar[j][i], -ex); ai[j][i] = ldexp(ai[j][i], -ex); }
        }

        if constexpr (C > 1) {
            for (int sweep = 0; sweep < CS_MAX_SWEEPS; ++sweep) {
                bool rotated = false;
#pragma unroll
                for (int p = 0; p < C - 1; ++p)
#pragma unroll
                    for (int q = p + 1; q < C; ++q) {
                        double alpha = 0.0, beta = 0.0, gr = 0.0, gi = 0.0;
#pragma unroll
                        for (int i = 0; i < R; ++i) {
                            alpha += ar[p][i] * ar[p][i] + ai[p][i] * ai[p][i];
                            beta += ar[q][i] * ar[q][i] + ai[q][i] * ai[q][i];
                            gr += ar[p][i] * ar[q][i] + ai[p][i] * ai[q][i];      // a_p^H a_q
                            gi += ar[p][i] * ai[q][i] - ai[p][i] * ar[q][i];
                        }
                        const double g2 = gr * gr + gi * gi;
                        if (g2 > CS_TOL2 * alpha * beta) {             // false for a zero column and for NaN: no division by 0
                            rotated = true;
                            const double g = sqrt(g2);
                            const double er = gr / g, ei = gi / g;     // a_q <- e^{-i theta} a_q makes the inner product real
                            const double zeta = (beta - alpha) / (2.0 * g);
                            const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                            const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
#pragma unroll
                            for (int i = 0; i < R; ++i) {
                                const double qr = er * ar[q][i] + ei * ai[q][i], qi = er * ai[q][i] - ei * ar[q][i];
                                const double pr = ar[p][i], pi = ai[p][i];
                                ar[p][i] = c * pr - sn * qr; ai[p][i] = c * pi - sn * qi;
                                ar[q][i] = sn * pr + c * qr; ai[q][i] = sn * pi + c * qi;
                            }
                        }
                    }
                if (__ballot(rotated) == 0) break;                     // wave-uniform exit
            }
        }

        double sv[C];
#pragma unroll
        for (int j = 0; j < C; ++j) {
            double a = 0.0;
#pragma unroll
            for (int i = 0; i < R; ++i) a += ar[j][i] * ar[j][i] + ai[j][i] * ai[j][i];
            sv[j] = ldexp(sqrt(a), ex);
        }
        // non-finite input: every output of this matrix is NaN (comparisons with NaN would leave the sort undefined)
        double tot = 0.0;
#pragma unroll
        for (int j = 0; j < C; ++j) tot += sv[j];
        if (!(tot < HUGE_VAL)) {
#pragma unroll
            for (int j = 0; j < C; ++j) sv[j] = tot - tot;
        }
        // descending
#pragma unroll
        for (int a = 0; a < C - 1; ++a)
#pragma unroll
            for (int b = 0; b < C - 1 - a; ++b) {
                const double hi = sv[b], lo = sv[b + 1];
                const bool sw = lo > hi;
                sv[b] = sw ? lo : hi; sv[b + 1] = sw ? hi : lo;
            }
        const double s1 = sv[0];
        double smin = sv[0];
#pragma unroll
        for (int j = 1; j < C; ++j) smin = (j < n_s) ? sv[j] : smin;
        const double thr = fmax(1e-2 * (s1 * s1), thr_floor);
        int rank = 0;
        double capk = 0.0;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            if (j < n_s) {
                const double s2 = sv[j] * sv[j];
                rank += (s2 >= thr) ? 1 : 0;
                capk += log2(1.0 + gam * s2);
            }
        }
        if (k < N) {
            const size_t o = (size_t)blk * N + k;
            cp.cond[o] = s1 / fmax(smin, 1e-12);
            cp.rank[o] = (uint8_t)rank;
            if (cp.S) {
#pragma unroll
                for (int j = 0; j < C; ++j)
                    if (j < n_s) cp.S[o * n_s + j] = sv[j];
            }
            cap_acc += capk;
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) cap_acc += __shfl_xor(cap_acc, off);
    if (lane == 0) cp.cap[blk] = cap_acc / (double)N;
}

template <int NT, int NR>
static int launch_one(const ChanStatParams& cp, hipStream_t stream) {
    hipLaunchKernelGGL((channel_metrics_kernel<NT, NR>), dim3(cp.n_blocks), dim3(64), 0, stream, cp);
    return (int)hipGetLastError();
}

int launch_channel_metrics(const ChanStatParams& cp, hipStream_t stream) {
    const int lo = cp.n_t < cp.n_r ? cp.n_t : cp.n_r, hi = cp.n_t < cp.n_r ? cp.n_r : cp.n_t;
    if (lo < 1 || lo > 4 || hi > 8) return -1;
    if (cp.n_t == 1 && cp.n_r == 1) return launch_one<1, 1>(cp, stream);
    if (cp.n_t == 1 && cp.n_r == 2) return launch_one<1, 2>(cp, stream);
    if (cp.n_t == 2 && cp.n_r == 2) return launch_one<2, 2>(cp, stream);
    if (cp.n_t == 4 && cp.n_r == 8) return launch_one<4, 8>(cp, stream);
    return launch_one<0, 0>(cp, stream);
}

}  // namespace esn
