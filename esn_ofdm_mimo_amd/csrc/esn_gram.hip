// The primal form of the read-out fit: a read-out kept as running normal equations
//
//   Gm = sum_s gamma^age(s) E_s^T E_s   [cols][cols],      Cm = sum_s gamma^age(s) D_s^T E_s   [n_out][cols],
//
// whose size does not depend on how many pilots or data symbols went into it, and the solve of
// (Gm + lambda I) W^T = Cm^T for several lambdas from the one Gm.  Two kernels, float64 on the matrix pipe
// (v_mfma_f64_16x16x4_f64):
//
//   gram_accumulate_kernel   Gm <- decay Gm + E^T E, Cm <- decay Cm + D_s^T E over rows [transient, T).  One workgroup
//       per (group, band of GA_BAND tile rows): it owns the lower tiles of its tile rows and their 16 columns of Cm,
//       streams the rows of E through LDS in chunks of GA_KC, keeps every tile in accumulator registers over all
//       chunks and touches each state element once -- one read (none when decay == 0: the <true> instance holds no
//       load of the state) and one write, the mirror image of an off-diagonal element written from the same register.
//   gram_solve_kernel        one workgroup per group, the candidates one after the other over one factor buffer in the
//       caller's workspace: left-looking blocked Cholesky of Gm + lambda I, panel products, diagonal block and panel
//       solve by chol_panel_factor (esn_chol_panel.h, shared with readout_chol_big_kernel; Gm itself is only read: a
//       left-looking factorisation never updates the trailing matrix), then the substitutions, one wave per right-hand
//       side, as in esn_solve_chol_big.hip.
//
// Every sum runs in an order fixed by the shape alone (the row chunks in order, one accumulator per element), there are
// no atomics and a group's result does not depend on the batch it is in.  Loads of E, D_s, Gm and Cm do not sit behind a
// branch: addresses are clamped and what lies outside is a select.  The factor columns of the substitutions are
// predicated loads, as in esn_solve_chol_big.hip (a third faster than the clamped form: profiles/chol_panel_time.txt).
#include "esn_chol_panel.h"
#include "esn_stage.h"

namespace esn {

constexpr int GR_NMAX = 544;                // largest cols served: N_res 512 + 32 inputs, 34 tiles
constexpr int GR_TMAX = GR_NMAX / 16;

// ---- accumulate -----------------------------------------------------------------------------------------------------
constexpr int GA_NT = 512;                  // 8 waves
constexpr int GA_NW = GA_NT / 64;
constexpr int GA_BAND = 2;                  // tile rows per workgroup
constexpr int GA_KC = 8;                    // rows of E per chunk
// LDS row: the columns of E [0, GR_NMAX) and the 16 columns of D_s behind them ("tile" GR_TMAX); the stride % 32 == 16
// puts the two 16-lane groups of a half wave (two consecutive k) on different banks
constexpr int GA_LD = GR_NMAX + 16;
constexpr int GA_TPW = (GA_BAND * (GR_TMAX + 1) + GA_NW - 1) / GA_NW;      // tiles per wave: 9
static_assert(GR_NMAX % 16 == 0 && GA_LD % 32 == 16 && GA_KC % 4 == 0 && GA_KC * 16 <= GA_NT, "layout");

typedef double gr_f64x4 __attribute__((ext_vector_type(4)));

struct GramAccParams {
    const double* E; const float* E32; const double* D;
    int T, transient, cols, n_out;
    const double* t_scale; const double* t_shift;
    double decay; double* Gm; double* Cm;
};

template <typename TE, bool VEC, bool FRESH>
__global__ __launch_bounds__(GA_NT) void gram_accumulate_kernel(GramAccParams sp) {
    __shared__ __attribute__((aligned(16))) double Es[GA_KC * GA_LD];      // 35 840 B
    constexpr int V = StageUnit<TE, VEC>::V;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int rows = sp.T - sp.transient, cols = sp.cols, nrhs = sp.n_out;
    const int ntile = (cols + 15) / 16, nband = (ntile + GA_BAND - 1) / GA_BAND;
    const int g = blockIdx.x / nband, band = blockIdx.x - g * nband;
    const TE* Eg = stage_src(sp, (TE*)nullptr) + ((size_t)g * sp.T + sp.transient) * cols;    // [rows][cols]
    const double* Dg = sp.D + ((size_t)g * sp.T + sp.transient) * nrhs;
    double* Gg = sp.Gm + (size_t)g * cols * cols;
    double* Cg = sp.Cm + (size_t)g * nrhs * cols;

    // This workgroup's tiles: for each of its tile rows ti the lower tiles (ti, 0 .. ti), then the tile of Cm (tj =
    // GR_TMAX: the D_s columns of the LDS row).  Tile t of that list goes to wave t % GA_NW.
    const int ti0 = band * GA_BAND;
    const int ti_end = ti0 + GA_BAND < ntile ? ti0 + GA_BAND : ntile;
    const int need = ti_end * 16 < cols ? ti_end * 16 : cols;              // columns of E this band reads
    int my_ti[GA_TPW], my_tj[GA_TPW];
#pragma unroll
    for (int q = 0; q < GA_TPW; ++q) {
        int t = wv + GA_NW * q, ti = ti0;
        while (ti < ti_end && t >= ti + 2) { t -= ti + 2; ++ti; }
        const bool ok = ti < ti_end;
        my_ti[q] = ok ? ti : 0;
        my_tj[q] = ok ? (t <= ti ? t : GR_TMAX) : -1;
    }
    gr_f64x4 acc[GA_TPW];
#pragma unroll
    for (int q = 0; q < GA_TPW; ++q) acc[q] = gr_f64x4{0.0, 0.0, 0.0, 0.0};

    // this thread's element of the D_s chunk (threads below 16 GA_KC): row tid / 16, output tid % 16
    const int dk = tid >> 4, dO = tid & 15;
    const bool d_on = tid < GA_KC * 16 && dO < nrhs;
    const int dOc = dO < nrhs ? dO : 0;
    const double d_sc = (d_on && sp.t_scale) ? sp.t_scale[(size_t)g * nrhs + dOc] : 1.0;
    const double d_sh = (d_on && sp.t_shift) ? sp.t_shift[(size_t)g * nrhs + dOc] : 0.0;

    const int upr = (need + V - 1) / V, total = GA_KC * upr;               // units per row, per chunk
    for (int e = tid; e < GA_KC * GA_LD; e += GA_NT) Es[e] = 0.0;          // (columns past `need` stay zero)
    __syncthreads();
    for (int r0 = 0; r0 < rows; r0 += GA_KC) {
        // rows [r0, r0 + GA_KC) x columns [0, need) of E into LDS as float64, zero past `rows`
        for (int e0 = 0; e0 < total; e0 += GA_NT) {
            const int e = e0 + tid, ec = e < total ? e : 0;
            const int kk = ec / upr, c = (ec - kk * upr) * V, r = r0 + kk;
            double v[V];
            stage_fetch(Eg + (size_t)(r < rows ? r : rows - 1) * cols + c, v);
            if (e < total) {
#pragma unroll
                for (int x = 0; x < V; ++x) Es[kk * GA_LD + c + x] = r < rows ? v[x] : 0.0;
            }
        }
        {
            const int r = r0 + (dk < GA_KC ? dk : 0);
            const double d = Dg[(size_t)(r < rows ? r : rows - 1) * nrhs + dOc] * d_sc + d_sh;
            if (tid < GA_KC * 16) Es[dk * GA_LD + GR_NMAX + dO] = (d_on && r < rows) ? d : 0.0;
        }
        __syncthreads();
        // v_mfma_f64_16x16x4_f64: A[l % 16][l / 16], B[l / 16][l % 16], C reg i: row 4 i + l / 16, col l % 16
#pragma unroll
        for (int k4 = 0; k4 < GA_KC; k4 += 4) {
            const double* slab = Es + (k4 + lq) * GA_LD + lr;
#pragma unroll
            for (int q = 0; q < GA_TPW; ++q)
                if (my_tj[q] >= 0)
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(slab[my_ti[q] * 16], slab[my_tj[q] * 16], acc[q], 0, 0, 0);
        }
        __syncthreads();
    }

    // the state: element (row, col) of tile (ti, tj) is register i of lane l with row = 16 ti + 4 i + l / 16,
    // col = 16 tj + l % 16.  Of a diagonal tile only row >= col is taken and mirrored, so Gm is symmetric bit for bit.
#pragma unroll
    for (int q = 0; q < GA_TPW; ++q) {
        if (my_tj[q] < 0) continue;
        const bool is_c = my_tj[q] == GR_TMAX;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = my_ti[q] * 16 + 4 * i + lq;                    // a column of E
            if (is_c) {
                const bool in = row < cols && lr < nrhs;
                double* at = Cg + (size_t)(in ? lr : 0) * cols + (in ? row : 0);
                double v = acc[q][i];
                if constexpr (!FRESH) v = sp.decay * *at + v;
                if (in) *at = v;
            } else {
                const int col = my_tj[q] * 16 + lr;
                const bool in = row < cols && col <= row;
                double* at = Gg + (size_t)(in ? row : 0) * cols + (in ? col : 0);
                double v = acc[q][i];
                if constexpr (!FRESH) v = sp.decay * *at + v;
                if (in) {
                    *at = v;
                    Gg[(size_t)col * cols + row] = v;
                }
            }
        }
    }
}

template <typename TE>
static int gram_accumulate_launch(const GramAccArgs& a) {
    const GramAccParams sp = {a.E, a.E32, a.D, a.T, a.transient, a.cols, a.n_out, a.t_scale, a.t_shift, a.decay,
                              a.Gm, a.Cm};
    const bool vec = a.cols % 4 == 0, fresh = a.decay == 0.0;
    void (*fn)(GramAccParams) =
        vec ? (fresh ? gram_accumulate_kernel<TE, true, true> : gram_accumulate_kernel<TE, true, false>)
            : (fresh ? gram_accumulate_kernel<TE, false, true> : gram_accumulate_kernel<TE, false, false>);
    const int ntile = (a.cols + 15) / 16;
    hipLaunchKernelGGL(fn, dim3((unsigned)((ntile + GA_BAND - 1) / GA_BAND * a.n_groups)), dim3(GA_NT), 0, a.stream, sp);
    return (int)hipGetLastError();
}

int gram_max_cols() { return GR_NMAX; }

int launch_gram_accumulate(const GramAccArgs& a) {
    if (a.cols > GR_NMAX || a.n_out > 16) return -1;
    return a.E32 ? gram_accumulate_launch<float>(a) : gram_accumulate_launch<double>(a);
}

// ---- solve ----------------------------------------------------------------------------------------------------------
constexpr int GS_NT = CP_NT;                // 8 waves, as the workspace Cholesky kernel
constexpr int GS_NW = CP_NW;
constexpr int GS_PLD = CP_PLD;              // LDS row stride of the panel (doubles)
constexpr int GS_RHS = 16;                  // right-hand sides at most
constexpr int GS_NS = (GR_NMAX + 63) / 64;  // rows per lane in the substitutions
constexpr size_t GS_LDS = sizeof(double) * ((size_t)GS_RHS * GR_NMAX + (size_t)GR_NMAX * GS_PLD);         // 143 616 B
static_assert(GS_LDS + sizeof(double) * (GR_NMAX + 16 * 17 + GS_NW) + 64 <= 160 * 1024, "the LDS of a CU");

struct GramSolveParams {
    const double* Gm; const double* Cm; int cols, n_out;
    const double* ridge; int n_ridge;
    double* W_out; int* status; double* work; size_t work_stride;
};

size_t gram_solve_work_doubles(int cols) {
    const size_t np = (size_t)round_up(cols, 16);
    return np * np;
}

__global__ __launch_bounds__(GS_NT) void gram_solve_kernel(GramSolveParams sp) {
    extern __shared__ __attribute__((aligned(16))) char gs_smem[];
    __shared__ int sh_bad;
    __shared__ double sh_invd[GR_NMAX];
    __shared__ double sh_linv[16][17];
    __shared__ double sh_red[GS_NW];
    double* Bs = reinterpret_cast<double*>(gs_smem);                    // [nrhs][np] right-hand sides, then solutions
    double* P = Bs + (size_t)GS_RHS * GR_NMAX;                          // [np][GS_PLD] panel
    const int g = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int wvu = __builtin_amdgcn_readfirstlane(wv);
    const int lr = lane & 15, lq = lane >> 4;
    const int n = sp.cols, nrhs = sp.n_out;
    const int np = round_up(n, 16), ntile = np / 16, ld = np;
    const double* Gg = sp.Gm + (size_t)g * n * n;                       // row-major, symmetric, read only
    const double* Cg = sp.Cm + (size_t)g * nrhs * n;
    double* Lw = sp.work + (size_t)g * sp.work_stride;                  // [np][np] column-major factor, lower part

    const CholPanelLds lds = {P, sh_invd, sh_linv, &sh_bad};
    // the largest diagonal entry of Gm (the candidates add their lambda to it)
    const double gmax = chol_diag_max([&](int i) { return Gg[(size_t)i * n + i]; }, n, sh_red);

    for (int l = 0; l < sp.n_ridge; ++l) {
        const int slot = g * sp.n_ridge + l;
        double* wo = sp.W_out + (size_t)slot * nrhs * n;
        const double lam = sp.ridge[slot];
        if (!(lam >= 0.0 && lam <= 1.7976931348623157e308)) {           // (uniform) as the ridge solves: status 2
            for (int i = tid; i < nrhs * n; i += GS_NT) wo[i] = 0.0;
            if (tid == 0) sp.status[slot] = 2;
            continue;
        }
        const double piv_tol = 1e-14 * (gmax + lam);
        if (tid == 0) sh_bad = 0;
        for (int e = tid; e < nrhs * np; e += GS_NT) {
            const int o = e / np, i = e - o * np;
            const double v = Cg[(size_t)o * n + (i < n ? i : 0)];
            Bs[e] = i < n ? v : 0.0;
        }
        __syncthreads();

        // ---- left-looking panel Cholesky of Gm + lambda I; element (row, col) of Gm is read as (col, row), which is the
        // same number and puts a lane group's 16 rows on one 128-byte segment; the address is clamped, padding a select
        for (int j = 0; j < ntile; ++j)
            chol_panel_factor(Lw, ld, n, np, piv_tol, lds, wvu, j, [&](int rt, int j0, int i) {
                const int row = rt * 16 + 4 * i + lq, col = j0 + lr;
                const bool in = row < n && col < n;
                const double v = Gg[(size_t)(in ? col : 0) * n + (in ? row : 0)];
                return in ? (row == col ? v + lam : v) : 0.0;
            });

        // ---- L L^T x = b, one wave per right-hand side at a time; lane holds rows lane + 64 s ----------------------
        for (int o = wvu; o < nrhs; o += GS_NW) {
            double* xb = Bs + (size_t)o * np;
            const int ns = (np + 63) / 64;
            double b[GS_NS], lc[GS_NS], lnext[GS_NS];
#pragma unroll
            for (int s2 = 0; s2 < GS_NS; ++s2) b[s2] = (s2 < ns && lane + 64 * s2 < np) ? xb[lane + 64 * s2] : 0.0;
            auto load_col = [&](double (&dst)[GS_NS], int jc) {
#pragma unroll
                for (int s2 = 0; s2 < GS_NS; ++s2) {
                    const int i = lane + 64 * s2;
                    dst[s2] = (s2 < ns && jc >= 0 && jc < n && i < n) ? Lw[(size_t)jc * ld + i] : 0.0;
                }
            };
            auto pick = [&](const double (&v)[GS_NS], int jc) -> double {      // element jc of the distributed vector
                double own = 0.0;
#pragma unroll
                for (int s2 = 0; s2 < GS_NS; ++s2) own = ((jc >> 6) == s2) ? v[s2] : own;
                return __shfl(own, jc & 63);
            };
            load_col(lc, 0);
            for (int jc = 0; jc < n; ++jc) {                                   // forward: L z = b
                load_col(lnext, jc + 1);
                const double zj = pick(b, jc) * sh_invd[jc];
#pragma unroll
                for (int s2 = 0; s2 < GS_NS; ++s2) {
                    const int i = lane + 64 * s2;
                    b[s2] = (i == jc) ? zj : ((i > jc) ? fma(-lc[s2], zj, b[s2]) : b[s2]);
                }
#pragma unroll
                for (int s2 = 0; s2 < GS_NS; ++s2) lc[s2] = lnext[s2];
            }
            load_col(lc, n - 1);
            for (int jc = n - 1; jc >= 0; --jc) {                              // backward: L^T x = z
                load_col(lnext, jc - 1);
                double part = 0.0;
#pragma unroll
                for (int s2 = 0; s2 < GS_NS; ++s2) {
                    const int i = lane + 64 * s2;
                    part = (i > jc && i < n) ? fma(lc[s2], b[s2], part) : part;
                }
                part = wave_sum(part);
                const double xj = (pick(b, jc) - part) * sh_invd[jc];
#pragma unroll
                for (int s2 = 0; s2 < GS_NS; ++s2) b[s2] = (lane + 64 * s2 == jc) ? xj : b[s2];
#pragma unroll
                for (int s2 = 0; s2 < GS_NS; ++s2) lc[s2] = lnext[s2];
            }
#pragma unroll
            for (int s2 = 0; s2 < GS_NS; ++s2)
                if (s2 < ns && lane + 64 * s2 < np) xb[lane + 64 * s2] = b[s2];
        }
        __syncthreads();
        // a rejected pivot flags this (group, candidate) and leaves its W_out zero; nothing is repaired here
        const bool bad = sh_bad != 0;
        for (int e = tid; e < nrhs * n; e += GS_NT) {
            const int o = e / n, c = e - o * n;
            wo[e] = bad ? 0.0 : Bs[o * np + c];
        }
        if (tid == 0) sp.status[slot] = bad ? 1 : 0;
        __syncthreads();                                                // (Bs, sh_bad and the factor are free again)
    }
}

int launch_gram_solve(const GramSolveArgs& a) {
    if (a.cols > GR_NMAX || a.n_out > GS_RHS || a.n_ridge > 16) return -1;
    const GramSolveParams sp = {a.Gm, a.Cm, a.cols, a.n_out, a.ridge, a.n_ridge, a.W_out, a.status,
                                reinterpret_cast<double*>(a.workspace), gram_solve_work_doubles(a.cols)};
    // the LDS ceiling is raised once per device: the tracked loop launches per symbol
    static std::atomic<unsigned long long> raised{0};
    const int e = raise_dynamic_lds_once(reinterpret_cast<const void*>(gram_solve_kernel), GS_LDS, raised);
    if (e) return e;
    hipLaunchKernelGGL(gram_solve_kernel, dim3(a.n_groups), dim3(GS_NT), GS_LDS, a.stream, sp);
    return (int)hipGetLastError();
}

}  // namespace esn
