// C ABI entry points (include/esn_hip.h): argument validation, geometry choice,
// kernel launches.  No allocation, no synchronisation, no global state besides
// the thread-local error string -- every call is capturable into a hipGraph.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <string.h>
#include "esn_launch.h"
#include "esn_solve.h"      // the workspace sizes of the read-out solves

using namespace esn;

static thread_local char g_err[512] = "";

namespace esn {
// for esn_host.hip: same error string, same conventions
int api_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace esn
static int (&fail)(int, const char*, ...) = api_fail;

// ---- the knobs (esn_common.h: Knobs): ONE row each, walked by knobs() (initial values from the environment, read
// once) and by esn_debug_set.  How a value string becomes the knob:
enum KnobRule {
    KNOB_FLAG,       // first character '0' / '1', whichever the default is not, flips it; anything else: the default
    KNOB_INT,        // atoi
    KNOB_TRIPLE      // "a,b,c", all positive; anything else: {0, 0, 0}
};
struct KnobRow {
    const char* key;     // esn_debug_set
    const char* env;     // environment variable, or nullptr
    size_t field;        // offset in Knobs (an int; three for KNOB_TRIPLE)
    KnobRule rule;
    int dflt;            // value without a string (variable unset, esn_debug_set(key, NULL)) where the rule names none
};
static const KnobRow kKnobTable[] = {
    {"skew", "ESN_SKEW", offsetof(Knobs, skew), KNOB_FLAG, 1},
    {"mfma_geom", "ESN_MFMA_GEOM", offsetof(Knobs, geom16), KNOB_TRIPLE, 0},
    {"mfma_geom_f32", "ESN_MFMA_GEOM_F32", offsetof(Knobs, geom32), KNOB_TRIPLE, 0},
    {"chol_skip", "ESN_CHOL_SKIP", offsetof(Knobs, chol_skip), KNOB_INT, 0},
    {"chol_dma", "ESN_CHOL_DMA", offsetof(Knobs, chol_dma), KNOB_FLAG, 1},
    {"f64_mfma", "ESN_F64_MFMA", offsetof(Knobs, f64_mfma), KNOB_FLAG, 1},
    {"big_gemm", "ESN_BIG_GEMM", offsetof(Knobs, big_gemm), KNOB_FLAG, 1},
    {"cluster", "ESN_CLUSTER", offsetof(Knobs, cluster), KNOB_FLAG, 1},
    {"gen_ko", nullptr, offsetof(Knobs, gen_ko), KNOB_INT, 0},
    {"s16", "ESN_S16", offsetof(Knobs, s16), KNOB_FLAG, 1},
    {"hcluster", "ESN_HCLUSTER", offsetof(Knobs, hcluster), KNOB_FLAG, 1},
    {"detect_fixed", "ESN_DETECT_FIXED", offsetof(Knobs, detect_fixed), KNOB_FLAG, 1},
};

static void knob_parse(const KnobRow& r, const char* v, Knobs& k) {
    int* out = reinterpret_cast<int*>(reinterpret_cast<char*>(&k) + r.field);
    switch (r.rule) {
        case KNOB_FLAG: *out = (v && v[0] == '0' + !r.dflt) ? !r.dflt : r.dflt; break;
        case KNOB_INT: *out = v ? atoi(v) : r.dflt; break;
        case KNOB_TRIPLE: {
            int t[3];
            const bool ok = v && sscanf(v, "%d,%d,%d", &t[0], &t[1], &t[2]) == 3 && t[0] > 0 && t[1] > 0 && t[2] > 0;
            for (int i = 0; i < 3; ++i) out[i] = ok ? t[i] : 0;
            break;
        }
    }
}

namespace esn {
Knobs& knobs() {
    static Knobs k = [] {
        Knobs x{};
        for (const KnobRow& r : kKnobTable) knob_parse(r, r.env ? getenv(r.env) : nullptr, x);
        return x;
    }();
    return k;
}
}  // namespace esn

static int hip_fail(int e, const char* what) {
    if (e == 0) return 0;
    if (e > 0) return fail(-1000 - e, "%s: HIP error %d (%s)", what, e, hipGetErrorString((hipError_t)e));
    return fail(-2, "%s: no kernel instance for this shape", what);
}

static bool check_shape(const esn_shape_t* s) {
    return s && s->n_res > 0 && s->n_in > 0 && s->n_out > 0 && s->n_wsets > 0;
}

// Geometry for a precision; for ESN_F64 only Bt (frames per tile) is meaningful.
static bool geometry_for(int precision, const esn_shape_t* s, Geometry* g, bool harvest = false) {
    memset(g, 0, sizeof(*g));
    if (precision == ESN_F64) {
        int fb = 8;
        while (fb > 1 && recur_f64_lds_bytes(fb, s->n_res, s->n_in, s->n_out) > 150 * 1024) fb >>= 1;
        if (recur_f64_lds_bytes(fb, s->n_res, s->n_in, s->n_out) > 160 * 1024) return false;
        // the matrix-pipe kernel where it fits (predict AND harvest must fit: one packed image serves both)
        Geometry gp, gh;
        memset(&gp, 0, sizeof(gp)); memset(&gh, 0, sizeof(gh));
        if (f64_mfma_geometry(s->n_res, s->n_in, s->n_out, false, &gp) &&
            f64_mfma_geometry(s->n_res, s->n_in, s->n_out, true, &gh))
            *g = harvest ? gh : gp;
        g->Bt = fb;
        return true;
    }
    if (precision < ESN_F64 || precision > ESN_BF16) return false;
    return mfma_geometry(precision, s->n_res, s->n_in, s->n_out, harvest, g);
}

// the fields CnnParams and LstmParams have under the same names, for esn_{cnn,lstm}_{train,predict} below (templates have
// C++ linkage, so they stand ahead of the extern "C" block): the sequence, the scalings, three weight and three bias
// arrays in (W0, b0), and the workspace
template <typename P>
static void sequence_params(P& p, int T_in, int T, int transient, const double* const (&W0)[3],
                            const double* const (&b0)[3], const double* in_scale, const double* in_shift,
                            const double* t_scale, const double* t_shift, const double* U, void* workspace) {
    memset(&p, 0, sizeof(p));
    p.T_in = T_in; p.T = T; p.transient = transient;
    for (int l = 0; l < 3; ++l) { p.W0[l] = W0[l]; p.b0[l] = b0[l]; }
    p.in_scale = in_scale; p.in_shift = in_shift; p.t_scale = t_scale; p.t_shift = t_shift; p.U = U;
    p.workspace = reinterpret_cast<double*>(workspace);
}

// ... and those of a training beside them
template <typename P>
static void training_params(P& p, int n_isets, int n_groups, uint64_t group_offset, int epochs, double lr, double beta1,
                            double beta2, double eps, const double* D, double* const (&W)[3], double* const (&b)[3],
                            double* loss) {
    p.n_isets = n_isets; p.n_groups = n_groups; p.group_offset = group_offset; p.epochs = epochs;
    p.lr = lr; p.beta1 = beta1; p.beta2 = beta2; p.eps = eps; p.D = D; p.loss = loss;
    for (int l = 0; l < 3; ++l) { p.W[l] = W[l]; p.b[l] = b[l]; }
}

#ifdef ESN_STAMPS
static unsigned long long* g_stamp_buf = nullptr;
extern "C" void esn_debug_set_stamp_buffer(void* dev) { g_stamp_buf = (unsigned long long*)dev; }
namespace esn { unsigned long long* stamp_buffer() { return g_stamp_buf; } }
#define ESN_SET_STAMPS(p) (p).stamps = g_stamp_buf
#else
#define ESN_SET_STAMPS(p) (p).stamps = nullptr
#endif

extern "C" {

const char* esn_last_error(void) { return g_err; }

int esn_abi_version(void) { return ESN_ABI_VERSION; }

int esn_debug_set(const char* key, const char* value) {
    if (!key) return fail(-1, "esn_debug_set: null key");
    for (const KnobRow& r : kKnobTable)
        if (!strcmp(key, r.key)) { knob_parse(r, value, knobs()); return 0; }
    return fail(-1, "esn_debug_set: unknown key '%s'", key);
}

int esn_device_info(int* cu_count, int* lds_bytes_per_cu, int* clock_khz, char* arch_name, int arch_name_len) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail((int)e, "hipGetDevice");
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return hip_fail((int)e, "hipGetDeviceProperties");
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (lds_bytes_per_cu) *lds_bytes_per_cu = (int)prop.maxSharedMemoryPerMultiProcessor;
    if (clock_khz) *clock_khz = prop.clockRate;
    if (arch_name && arch_name_len > 0) {
        strncpy(arch_name, prop.gcnArchName, arch_name_len - 1);
        arch_name[arch_name_len - 1] = 0;
    }
    return 0;
}

int esn_tile_frames(int precision, const esn_shape_t* shape) {
    Geometry g;
    if (!check_shape(shape)) return fail(-1, "esn_tile_frames: invalid shape");
    if (!geometry_for(precision, shape, &g)) return fail(-2, "esn_tile_frames: unsupported shape/precision");
    return g.Bt;
}

size_t esn_packed_weights_bytes(int precision, const esn_shape_t* shape) {
    Geometry g;
    if (!check_shape(shape) || !geometry_for(precision, shape, &g)) return 0;
    return packed_w_bytes(precision, shape->n_res, shape->n_in, shape->n_out, g);
}

size_t esn_packed_readout_bytes(int precision, const esn_shape_t* shape) {
    Geometry g;
    if (!check_shape(shape) || !geometry_for(precision, shape, &g)) return 0;
    return packed_wout_bytes(precision, shape->n_res, shape->n_in, shape->n_out, g);
}

int esn_pack_weights(int precision, const esn_shape_t* shape, const double* W, const double* W_in,
                     const double* W_fb, void* packed, void* stream) {
    Geometry g;
    if (!check_shape(shape)) return fail(-1, "esn_pack_weights: invalid shape");
    if (!W || !W_in || !W_fb || !packed) return fail(-1, "esn_pack_weights: null pointer");
    if (!geometry_for(precision, shape, &g)) return fail(-2, "esn_pack_weights: unsupported shape/precision");
    return hip_fail(launch_pack_weights(precision, shape, g, W, W_in, W_fb, packed, (hipStream_t)stream),
                    "esn_pack_weights");
}

int esn_pack_readout(int precision, const esn_shape_t* shape, int n_groups, const double* W_out,
                     void* packed, void* stream) {
    Geometry g;
    if (!check_shape(shape) || n_groups <= 0) return fail(-1, "esn_pack_readout: invalid shape");
    if (!W_out || !packed) return fail(-1, "esn_pack_readout: null pointer");
    if (!geometry_for(precision, shape, &g)) return fail(-2, "esn_pack_readout: unsupported shape/precision");
    return hip_fail(launch_pack_readout(precision, shape, g, n_groups, W_out, packed, (hipStream_t)stream),
                    "esn_pack_readout");
}

// float64: the matrix-pipe kernel for batches (more slots than one vector-ALU tile holds), the
// vector-ALU kernel for the 2-D drop-in's single sequence and for shapes the MFMA tiling does not cover
static bool use_f64_mfma(int precision, const RecurParams& p) {
    return precision == ESN_F64 && p.g.m64 && p.n_frames > 8 && knobs().f64_mfma;
}

static int fill_common(RecurParams& p, int precision, const esn_shape_t* shape, const char* who,
                       bool harvest = false) {
    memset(&p, 0, sizeof(p));
    if (!check_shape(shape)) return fail(-1, "%s: invalid shape", who);
    if (!geometry_for(precision, shape, &p.g, harvest)) return fail(-2, "%s: unsupported shape/precision", who);
    p.n_res = shape->n_res; p.n_in = shape->n_in; p.n_out = shape->n_out;
    p.teacher_forcing = shape->teacher_forcing ? 1 : 0;
    p.n_wsets = shape->n_wsets;
    p.wset_stride = packed_w_bytes(precision, p.n_res, p.n_in, p.n_out, p.g);
    p.wout_stride = packed_wout_bytes(precision, p.n_res, p.n_in, p.n_out, p.g);
    p.leak = (shape->leak_rate == 0.0) ? 1.0 : shape->leak_rate;
    if (!(p.leak > 0.0 && p.leak <= 1.0)) return fail(-1, "%s: leak_rate %g outside (0, 1]", who, shape->leak_rate);
    if (p.leak != 1.0 && precision != ESN_F64)
        return fail(-2, "%s: leak_rate != 1 is an extension of the float64 kernels (precision ESN_F64)", who);
    p.w16_off = (size_t)p.g.Mp * p.g.Kp * 2;
    p.wo16_off = wout_big_offset(precision, p.n_out, p.g);
    p.w64_off = f64_w_offset(p.n_res, p.n_in, p.n_out);
    p.wo64_off = f64_wout_offset(p.n_res, p.n_in, p.n_out);
    p.harvest = harvest ? 1 : 0;
    return 0;
}

// The batch of one call and its slot axis (esn_common.h: Fpad, spw, n_tiles), after fill_common.  Predict: n_frames
// sequences in groups of F.  Harvest: one pilot per group (n_frames = n_groups, F = 1), tiles span groups.
static void fill_batch(RecurParams& p, int precision, int n_frames, int frames_per_group) {
    p.n_frames = n_frames;
    p.F = frames_per_group;
    p.n_groups = (n_frames + frames_per_group - 1) / frames_per_group;
    const bool m64 = use_f64_mfma(precision, p);
    // slots per group: one pilot (harvest); the readout's 16-frame column granularity (MFMA kernels) or no padding at
    // all (float64 vector-ALU kernel)
    p.Fpad = p.harvest ? 1 : (precision == ESN_F64 && !m64) ? p.F : round_up(p.F, 16);
    // float64 vector-ALU kernel: every frame slot of a tile costs its share of FMAs whether it holds a frame or not,
    // so a batch smaller than the tile (the 2-D drop-in is ONE sequence) gets a smaller tile
    // (Tried for the harvest: leaving slots empty so that 2048 pilots spread over 256 tiles of 8 instead of 64 tiles of
    //  32 -- the harvest is bound by the AGGREGATE L2 weight stream, 4x the workgroups stream 4x the bytes: 1.14 -> 1.23 ms.)
    if (precision == ESN_F64 && !m64 && (!p.harvest || p.n_wsets == 1)) {
        const long long slots = (long long)p.n_groups * p.Fpad;
        while (p.g.Bt > 1 && p.g.Bt / 2 >= slots) p.g.Bt >>= 1;
    }
    const int tile = m64 ? p.g.Bt64 : p.g.Bt;
    // with several weight sets the slot axis is set-major (esn_common.h: spw), so a tile packs the groups of ONE set
    // back to back instead of padding every group to a whole tile
    if (p.n_wsets > 1) {
        const int gpw = (p.n_groups + p.n_wsets - 1) / p.n_wsets;
        p.spw = round_up(gpw * p.Fpad, tile);
        p.n_tiles = p.n_wsets * (p.spw / tile);
    } else {
        p.n_tiles = (int)(((long long)p.n_groups * p.Fpad + tile - 1) / tile);
    }
}

// ---- THE dispatch rule: which kernel serves a recurrence call (an esn_path) and how much workspace the size
// queries advertise for it.  The launches, esn_*_workspace_bytes and esn_recur_path all ask here; the order of the
// ladder is the specification.  `p` is filled by fill_common + fill_batch.
struct Plan {
    int path;                  // enum esn_path
    size_t workspace_bytes;    // what the size query answers; the path reads that many bytes iff path_uses_workspace
};
static bool path_uses_workspace(int path) {
    return path == ESN_PATH_CLUSTER_F64 || path == ESN_PATH_BIG_PREDICT || path == ESN_PATH_BIG_HARVEST ||
           path == ESN_PATH_HARVEST_CLUSTER;
}

static Plan plan_recur(int precision, const RecurParams& p, bool workspace_lent) {
    const Knobs& k = knobs();
    const bool half = precision == ESN_F16 || precision == ESN_BF16;
    Plan pl = {ESN_PATH_MFMA, 0};
    if (workspace_lent) {
        // ONE float64 sequence (the reference's own call pattern): the matrix resident in the LDS of a cluster of
        // workgroups that exchange the state through L2 every step (esn_recur_cluster.hip)
        if (k.cluster && cluster_applies(precision, p))
            return {ESN_PATH_CLUSTER_F64, cluster_workspace_bytes(p.n_res, p.n_in, p.n_out, p.harvest != 0)};
        // harvest, 257..512 units, fp16/bf16: pairs of workgroups with the matrix resident in registers / LDS
        if (p.harvest && k.hcluster && harvest_cluster_applies(precision, p))
            return {ESN_PATH_HARVEST_CLUSTER, harvest_cluster_workspace_bytes(p.n_groups, p.n_wsets)};
        // large reservoirs: one GEMM launch per step
        if (p.harvest ? big_harvest_applies(precision, p) : (p.g.big && big_path_applies(precision, p))) {
            pl.workspace_bytes = p.harvest ? big_harvest_workspace_bytes(p.n_groups, p.g.Kp)
                                           : big_workspace_bytes(big_slots(p), p.g.Mp, p.g.Kp);
            if (k.big_gemm) { pl.path = p.harvest ? ESN_PATH_BIG_HARVEST : ESN_PATH_BIG_PREDICT; return pl; }
            // Kept as found: with big_gemm = 0 the size queries still advertise the GEMM paths' workspace although
            // the persistent kernel below serves the call and reads none of it (tests/test_dispatch_cpu.py names
            // this exception).  Making the queries follow the knob changes their answers: a change of its own.
        }
    }
    if (!p.harvest) {
        // N_res 257..512, fp16/bf16: the skewed schedule on 16x16x32 MFMAs (the chip holds a higher clock on that shape)
        if (p.g.s16 && p.g.skew && k.s16 && half) { pl.path = ESN_PATH_SKEW16; return pl; }
    }
    pl.path = use_f64_mfma(precision, p) ? ESN_PATH_F64_MFMA : precision == ESN_F64 ? ESN_PATH_F64_VALU : ESN_PATH_MFMA;
    return pl;
}

// plan, the ONE workspace check, launch
static int launch_plan(const char* who, const char* size_query, int precision, RecurParams& p, bool io32,
                       void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const Plan pl = plan_recur(precision, p, workspace != nullptr);
    if (path_uses_workspace(pl.path) && workspace_bytes < pl.workspace_bytes)
        return fail(-1, "%s: workspace holds %zu bytes, %s says %zu", who, workspace_bytes, size_query,
                    pl.workspace_bytes);
    int e = -1;
    switch (pl.path) {
        case ESN_PATH_CLUSTER_F64: e = launch_recur_cluster(p, workspace, stream); break;
        case ESN_PATH_HARVEST_CLUSTER: e = launch_harvest_cluster(precision, p, workspace, stream); break;
        case ESN_PATH_BIG_HARVEST: e = launch_harvest_big(precision, p, workspace, stream); break;
        case ESN_PATH_BIG_PREDICT: e = launch_recur_big(precision, p, workspace, stream, io32); break;
        case ESN_PATH_SKEW16: e = launch_recur_skew16(precision, p, stream, io32); break;
        case ESN_PATH_F64_MFMA: e = launch_recur_f64_mfma(p, stream); break;
        case ESN_PATH_F64_VALU: e = launch_recur_f64(p, stream); break;
        case ESN_PATH_MFMA: e = launch_recur_mfma(precision, p, stream, io32); break;   // in-step or 32x32x16 skewed: g.skew
    }
    return hip_fail(e, who);
}

// esn_predict_batch and esn_predict_batch_f32: io32 = float32 U / Y (fp32/fp16/bf16 precisions only)
static int predict_common(const char* who, bool io32, int precision, const esn_shape_t* shape, const void* packed_w,
                          const void* packed_wout, const double* in_scale, const double* in_shift,
                          const double* t_scale, const double* t_shift, const void* U, int n_frames,
                          int frames_per_group, int T_in, int T, int transient, const double* x0, const double* y0,
                          double noise, int noise_mode, const double* noise_u, uint64_t seed, uint64_t group_offset,
                          void* Y, void* workspace, size_t workspace_bytes, void* stream) {
    if (io32 && precision == ESN_F64)
        return fail(-2, "%s: float32 I/O is served for precisions f32 / f16 / bf16; ESN_F64 reads and writes float64 "
                    "(esn_predict_batch)", who);
    RecurParams p;
    int rc = fill_common(p, precision, shape, who);
    if (rc) return rc;
    if (!packed_w || !packed_wout || !U || !Y) return fail(-1, "%s: null pointer", who);
    if (n_frames <= 0 || frames_per_group <= 0 || T <= 0 || T_in < 0 || T_in > T || transient < 0 || transient >= T)
        return fail(-1, "%s: invalid sizes (n_frames=%d F=%d T_in=%d T=%d transient=%d)",
                    who, n_frames, frames_per_group, T_in, T, transient);
    if (noise_mode == ESN_NOISE_TENSOR && !noise_u) return fail(-1, "%s: noise tensor missing", who);
    if (noise_mode < ESN_NOISE_NONE || noise_mode > ESN_NOISE_COUNTER) return fail(-1, "%s: bad noise mode", who);
    // (float32 rows are staged in 16-byte chunks of four inputs when n_in is a multiple of 4, else in 4-byte ones)
    if (io32 && ((uintptr_t)U & ((shape->n_in & 3) == 0 ? 15 : 3)) != 0)
        return fail(-1, "%s: U must be %d-byte aligned", who, (shape->n_in & 3) == 0 ? 16 : 4);
    fill_batch(p, precision, n_frames, frames_per_group);
    p.T_in = T_in; p.S = T; p.in_row_off = 0; p.transient = transient;
    p.packed_w = packed_w; p.packed_wout = packed_wout;
    p.in_scale = in_scale; p.in_shift = in_shift; p.t_scale = t_scale; p.t_shift = t_shift;
    if (io32) p.U32 = static_cast<const float*>(U); else p.U = static_cast<const double*>(U);
    p.x0 = x0; p.y0 = y0; p.noise_u = noise_u;
    p.noise = noise; p.noise_mode = (noise == 0.0) ? ESN_NOISE_NONE : noise_mode; p.seed = seed;
    p.frame_off = (uint32_t)(group_offset * (uint64_t)frames_per_group);
    p.wset_rot = (int)(group_offset % (uint64_t)p.n_wsets);
    if (((uintptr_t)Y & 15) != 0) return fail(-1, "%s: Y must be 16-byte aligned", who);
    if (io32) p.Y32 = static_cast<float*>(Y); else p.Y = static_cast<double*>(Y);
    ESN_SET_STAMPS(p);
    return launch_plan(who, "esn_predict_workspace_bytes", precision, p, io32, workspace, workspace_bytes,
                       (hipStream_t)stream);
}

int esn_predict_batch(int precision, const esn_shape_t* shape, const void* packed_w, const void* packed_wout,
                      const double* in_scale, const double* in_shift, const double* t_scale,
                      const double* t_shift, const double* U, int n_frames, int frames_per_group, int T_in,
                      int T, int transient, const double* x0, const double* y0, double noise, int noise_mode,
                      const double* noise_u, uint64_t seed, uint64_t group_offset, double* Y, void* workspace,
                      size_t workspace_bytes, void* stream) {
    return predict_common("esn_predict_batch", false, precision, shape, packed_w, packed_wout, in_scale, in_shift,
                          t_scale, t_shift, U, n_frames, frames_per_group, T_in, T, transient, x0, y0, noise,
                          noise_mode, noise_u, seed, group_offset, Y, workspace, workspace_bytes, stream);
}

int esn_predict_batch_f32(int precision, const esn_shape_t* shape, const void* packed_w, const void* packed_wout,
                          const double* in_scale, const double* in_shift, const double* t_scale,
                          const double* t_shift, const float* U, int n_frames, int frames_per_group, int T_in,
                          int T, int transient, const double* x0, const double* y0, double noise, int noise_mode,
                          const double* noise_u, uint64_t seed, uint64_t group_offset, float* Y, void* workspace,
                          size_t workspace_bytes, void* stream) {
    return predict_common("esn_predict_batch_f32", true, precision, shape, packed_w, packed_wout, in_scale, in_shift,
                          t_scale, t_shift, U, n_frames, frames_per_group, T_in, T, transient, x0, y0, noise,
                          noise_mode, noise_u, seed, group_offset, Y, workspace, workspace_bytes, stream);
}

size_t esn_predict_workspace_bytes(int precision, const esn_shape_t* shape, int n_frames, int frames_per_group) {
    RecurParams p;
    if (n_frames <= 0 || frames_per_group <= 0) return 0;
    if (fill_common(p, precision, shape, "esn_predict_workspace_bytes")) return 0;
    fill_batch(p, precision, n_frames, frames_per_group);
    return plan_recur(precision, p, true).workspace_bytes;
}

size_t esn_harvest_workspace_bytes(int precision, const esn_shape_t* shape, int n_groups) {
    RecurParams p;
    if (n_groups <= 0) return 0;
    if (fill_common(p, precision, shape, "esn_harvest_workspace_bytes", true)) return 0;
    fill_batch(p, precision, n_groups, 1);
    return plan_recur(precision, p, true).workspace_bytes;
}

int esn_recur_path(int harvest, int precision, const esn_shape_t* shape, int n_sequences, int frames_per_group,
                   int have_workspace) {
    RecurParams p;
    int rc = fill_common(p, precision, shape, "esn_recur_path", harvest != 0);
    if (rc) return rc;
    if (harvest) frames_per_group = 1;
    if (n_sequences <= 0 || frames_per_group <= 0)
        return fail(-1, "esn_recur_path: invalid sizes (n_sequences=%d F=%d)", n_sequences, frames_per_group);
    fill_batch(p, precision, n_sequences, frames_per_group);
    return plan_recur(precision, p, have_workspace != 0).path;
}

static int harvest_common(int precision, const esn_shape_t* shape, const void* packed_w, const double* in_scale,
                      const double* in_shift, const double* t_scale, const double* t_shift, const double* U,
                      const double* D, int n_groups, int T, double noise, int noise_mode, const double* noise_u,
                      uint64_t seed, uint64_t group_offset, double* E, float* E32, void* workspace,
                      size_t workspace_bytes, void* stream) {
    RecurParams p;
    int rc = fill_common(p, precision, shape, "esn_harvest_batch", true);
    if (rc) return rc;
    if (!packed_w || !U || !D || (!E && !E32)) return fail(-1, "esn_harvest_batch: null pointer");
    if (E32 && precision == ESN_F64) return fail(-2, "esn_harvest_batch_f32: float32 states are an MFMA-kernel option (precision f32/f16/bf16)");
    if (n_groups <= 0 || T < 2) return fail(-1, "esn_harvest_batch: invalid sizes (n_groups=%d T=%d)", n_groups, T);
    if (noise_mode == ESN_NOISE_TENSOR && !noise_u) return fail(-1, "esn_harvest_batch: noise tensor missing");
    if (noise_mode < ESN_NOISE_NONE || noise_mode > ESN_NOISE_COUNTER) return fail(-1, "esn_harvest_batch: bad noise mode");
    fill_batch(p, precision, n_groups, 1);
    p.T_in = T; p.S = T - 1; p.in_row_off = 1; p.transient = 0;
    p.packed_w = packed_w;
    p.in_scale = in_scale; p.in_shift = in_shift; p.t_scale = t_scale; p.t_shift = t_shift;
    p.U = U; p.D = D; p.noise_u = noise_u;
    p.noise = noise; p.noise_mode = (noise == 0.0) ? ESN_NOISE_NONE : noise_mode; p.seed = seed;
    p.frame_off = (uint32_t)group_offset;
    p.wset_rot = (int)(group_offset % (uint64_t)p.n_wsets);
    if ((((uintptr_t)E) | ((uintptr_t)E32)) & 15) return fail(-1, "esn_harvest_batch: E must be 16-byte aligned");
    p.E = E; p.E32 = E32;
    ESN_SET_STAMPS(p);
    return launch_plan("esn_harvest_batch", "esn_harvest_workspace_bytes", precision, p, false, workspace,
                       workspace_bytes, (hipStream_t)stream);
}

int esn_harvest_batch(int precision, const esn_shape_t* shape, const void* packed_w, const double* in_scale,
                      const double* in_shift, const double* t_scale, const double* t_shift, const double* U,
                      const double* D, int n_groups, int T, double noise, int noise_mode, const double* noise_u,
                      uint64_t seed, uint64_t group_offset, double* E, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (!E) return fail(-1, "esn_harvest_batch: null pointer");
    return harvest_common(precision, shape, packed_w, in_scale, in_shift, t_scale, t_shift, U, D, n_groups, T, noise,
                          noise_mode, noise_u, seed, group_offset, E, nullptr, workspace, workspace_bytes, stream);
}

int esn_harvest_batch_f32(int precision, const esn_shape_t* shape, const void* packed_w, const double* in_scale,
                          const double* in_shift, const double* t_scale, const double* t_shift, const double* U,
                          const double* D, int n_groups, int T, double noise, int noise_mode,
                          const double* noise_u, uint64_t seed, uint64_t group_offset, float* E, void* workspace,
                          size_t workspace_bytes, void* stream) {
    if (!E) return fail(-1, "esn_harvest_batch_f32: null pointer");
    return harvest_common(precision, shape, packed_w, in_scale, in_shift, t_scale, t_shift, U, D, n_groups, T, noise,
                          noise_mode, noise_u, seed, group_offset, nullptr, E, workspace, workspace_bytes, stream);
}

// ---- read-out solves: QR, Cholesky and leave-one-out; pinv and ridge (an extension: the reference fits with pinv only)
size_t esn_readout_solve_workspace_bytes(int n_groups, int rows, int cols, int n_out) {
    if (n_groups <= 0 || rows <= 0 || cols <= 0 || n_out <= 0) return 0;
    return sizeof(double) * solve_work_doubles(rows, cols, n_out) * (size_t)n_groups;
}

size_t esn_readout_solve_ridge_workspace_bytes(int n_groups, int n_ridge, int rows, int cols, int n_out) {
    if (n_groups <= 0 || n_ridge <= 0 || rows <= 0 || cols <= 0 || n_out <= 0) return 0;
    return sizeof(double) * solve_ridge_work_doubles(rows, cols, n_out) * (size_t)n_groups * (size_t)n_ridge;
}

size_t esn_readout_chol_workspace_bytes(int n_groups, int rows, int cols) {
    if (n_groups <= 0 || rows <= 0 || cols <= 0) return 0;
    const int n = rows < cols ? rows : cols;
    if (n <= 128 || n > 512) return 0;             // LDS-resident kernel / not served
    return sizeof(double) * chol_big_work_doubles(n) * (size_t)n_groups;
}

size_t esn_readout_chol_ridge_workspace_bytes(int n_groups, int n_ridge, int rows, int cols) {
    if (n_ridge <= 0) return 0;
    return esn_readout_chol_workspace_bytes(n_groups, rows, cols) * (size_t)n_ridge;
}

size_t esn_readout_ridge_loo_workspace_bytes(int n_groups, int n_ridge, int rows, int cols) {
    if (n_groups <= 0 || n_ridge <= 0 || rows <= 0 || cols <= 0) return 0;
    return sizeof(double) * ridge_loo_work_doubles() * (size_t)n_groups;
}

// What an entry point requires of its arguments (esn_launch.h: ReadoutArgs).
enum ReadoutKernel { kQr, kChol, kLoo };
struct ReadoutRule {
    ReadoutKernel kernel;
    bool ridge;                                 // lambdas: mandatory, or absent (the pinv solve)
    int max_gram;                               // largest min(rows, cols) served; 0: any
    int max_ridge;                              // 1 .. max_ridge lambdas per group; 0: any number
    size_t (*need)(int, int, int, int);         // workspace query (n_groups, n_ridge, rows, cols); nullptr: QR, which
    const char* query;                          //   takes no size (its pointer is mandatory); the query's own name
    int align;                                  // 16: E and the workspace; 8: the workspace
};
static const int kCholLds = 128;                // the Cholesky kernel keeps Gram matrices up to this in LDS (no workspace)
static const ReadoutRule
    kQrPinv = {kQr, false, 0, 0, nullptr, nullptr, 0}, kQrRidge = {kQr, true, 0, 0, nullptr, nullptr, 0},
    kCholPinv = {kChol, false, 512, 0, esn_readout_chol_ridge_workspace_bytes, "esn_readout_chol_workspace_bytes", 16},
    kCholRidge = {kChol, true, 512, 0, esn_readout_chol_ridge_workspace_bytes, "esn_readout_chol_ridge_workspace_bytes", 16},
    kLooRidge = {kLoo, true, 128, 16, esn_readout_ridge_loo_workspace_bytes, "esn_readout_ridge_loo_workspace_bytes", 8};

// Null pointers, sizes, "not served", workspace size, alignment -- in that order for every entry point -- then the launch.
static int readout_call(const char* who, const ReadoutArgs& c, const ReadoutRule& r) {
    const bool loo = r.kernel == kLoo;
    if ((!c.E && !c.E32) || !c.D || !c.W_out || !c.status || (r.ridge && !c.ridge) || (loo && (!c.score || !c.choice))
        || (!r.need && !c.workspace))
        return fail(-1, "%s: null pointer", who);
    if (c.n_groups <= 0 || (!r.max_ridge && c.n_ridge <= 0) || c.T <= 0 || c.transient < 0 || c.transient >= c.T
        || c.cols <= 0 || c.n_out <= 0)
        return fail(-1, "%s: invalid sizes", who);
    const int rows = c.T - c.transient, n = rows < c.cols ? rows : c.cols;
    const bool big = r.kernel == kChol && n > kCholLds;     // Gram matrix and factor in the caller's workspace
    if (r.max_ridge && (c.n_ridge < 1 || c.n_ridge > r.max_ridge))
        return fail(-1, "%s: n_ridge = %d, 1 to %d candidates are served", who, c.n_ridge, r.max_ridge);
    if (loo && c.n_out > 8) return fail(-1, "%s: n_out = %d, at most 8 outputs are served", who, c.n_out);
    if (loo && n > r.max_gram)
        return fail(-2, "%s: min(rows, cols) = %d, the limit is %d (the factor stays in LDS)", who, n, r.max_gram);
    // (the pinv Cholesky entry points leave n_out > 8 at an LDS shape to the launcher, which has no instance for it)
    if (r.kernel == kChol && (n > r.max_gram || (c.n_out > 8 && (r.ridge || big))))
        return fail(-2, "%s: no kernel instance for this shape", who);
    if (loo || big) {
        const size_t need = r.need(c.n_groups, c.n_ridge, rows, c.cols);
        if (!c.workspace || c.workspace_bytes < need)
            return fail(-1, "%s: workspace holds %zu bytes, %s says %zu", who, c.workspace ? c.workspace_bytes : (size_t)0,
                        r.query, need);
        const uintptr_t e = (uintptr_t)(c.E ? (const void*)c.E : (const void*)c.E32), w = (uintptr_t)c.workspace;
        if (r.align == 16 && ((e | w) & 15)) return fail(-1, "%s: E and the workspace must be 16-byte aligned", who);
        if (r.align == 8 && (w & 7)) return fail(-1, "%s: the workspace must be 8-byte aligned", who);
    }
    if (loo) return hip_fail(launch_ridge_loo(c), who);
    if (r.kernel == kQr) return hip_fail(launch_readout_solve(c), who);
    return hip_fail(big ? launch_readout_chol_big(c) : launch_readout_chol(c), who);
}

int esn_readout_solve_batch(const double* E, const double* D, int n_groups, int T, int transient, int cols,
                            int n_out, const double* t_scale, const double* t_shift, double* W_out,
                            int* status, void* workspace, void* stream) {
    return readout_call("esn_readout_solve_batch",
                        {E, nullptr, D, n_groups, T, transient, cols, n_out, t_scale, t_shift, nullptr, 1, W_out,
                         nullptr, nullptr, status, workspace, 0, (hipStream_t)stream}, kQrPinv);
}

int esn_readout_solve_ridge_batch(const double* E, const double* D, int n_groups, int T, int transient, int cols,
                                  int n_out, const double* t_scale, const double* t_shift, const double* ridge,
                                  int n_ridge, double* W_out, int* status, void* workspace, void* stream) {
    return readout_call("esn_readout_solve_ridge_batch",
                        {E, nullptr, D, n_groups, T, transient, cols, n_out, t_scale, t_shift, ridge, n_ridge, W_out,
                         nullptr, nullptr, status, workspace, 0, (hipStream_t)stream}, kQrRidge);
}

int esn_readout_solve_chol_batch(const double* E, const double* D, int n_groups, int T, int transient, int cols,
                                 int n_out, const double* t_scale, const double* t_shift, double* W_out,
                                 int* status, void* workspace, size_t workspace_bytes, void* stream) {
    return readout_call("esn_readout_solve_chol_batch",
                        {E, nullptr, D, n_groups, T, transient, cols, n_out, t_scale, t_shift, nullptr, 1, W_out,
                         nullptr, nullptr, status, workspace, workspace_bytes, (hipStream_t)stream}, kCholPinv);
}

int esn_readout_solve_chol_batch_f32(const float* E, const double* D, int n_groups, int T, int transient, int cols,
                                     int n_out, const double* t_scale, const double* t_shift, double* W_out,
                                     int* status, void* workspace, size_t workspace_bytes, void* stream) {
    return readout_call("esn_readout_solve_chol_batch_f32",
                        {nullptr, E, D, n_groups, T, transient, cols, n_out, t_scale, t_shift, nullptr, 1, W_out,
                         nullptr, nullptr, status, workspace, workspace_bytes, (hipStream_t)stream}, kCholPinv);
}

int esn_readout_solve_chol_ridge_batch(const double* E, const double* D, int n_groups, int T, int transient, int cols,
                                       int n_out, const double* t_scale, const double* t_shift, const double* ridge,
                                       int n_ridge, double* W_out, int* status, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return readout_call("esn_readout_solve_chol_ridge_batch",
                        {E, nullptr, D, n_groups, T, transient, cols, n_out, t_scale, t_shift, ridge, n_ridge, W_out,
                         nullptr, nullptr, status, workspace, workspace_bytes, (hipStream_t)stream}, kCholRidge);
}

int esn_readout_solve_chol_ridge_batch_f32(const float* E, const double* D, int n_groups, int T, int transient,
                                           int cols, int n_out, const double* t_scale, const double* t_shift,
                                           const double* ridge, int n_ridge, double* W_out, int* status,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    return readout_call("esn_readout_solve_chol_ridge_batch_f32",
                        {nullptr, E, D, n_groups, T, transient, cols, n_out, t_scale, t_shift, ridge, n_ridge, W_out,
                         nullptr, nullptr, status, workspace, workspace_bytes, (hipStream_t)stream}, kCholRidge);
}

int esn_readout_ridge_loo_batch(const double* E, const double* D, int n_groups, int T, int transient, int cols,
                                int n_out, const double* t_scale, const double* t_shift, const double* ridge,
                                int n_ridge, double* W_out, double* score, int* choice, int* status, void* workspace,
                                size_t workspace_bytes, void* stream) {
    return readout_call("esn_readout_ridge_loo_batch",
                        {E, nullptr, D, n_groups, T, transient, cols, n_out, t_scale, t_shift, ridge, n_ridge, W_out,
                         score, choice, status, workspace, workspace_bytes, (hipStream_t)stream}, kLooRidge);
}

int esn_readout_ridge_loo_batch_f32(const float* E, const double* D, int n_groups, int T, int transient, int cols,
                                    int n_out, const double* t_scale, const double* t_shift, const double* ridge,
                                    int n_ridge, double* W_out, double* score, int* choice, int* status,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    return readout_call("esn_readout_ridge_loo_batch_f32",
                        {nullptr, E, D, n_groups, T, transient, cols, n_out, t_scale, t_shift, ridge, n_ridge, W_out,
                         score, choice, status, workspace, workspace_bytes, (hipStream_t)stream}, kLooRidge);
}

// ---- hold-out score of the candidates of a multi-lambda solve (esn_holdout.hip) -----------------------------------------
// Null pointers, sizes, "not served", alignment -- the order of readout_call -- then the launch.
static int holdout_call(const char* who, const HoldoutArgs& c) {
    if ((!c.E && !c.E32) || !c.D || !c.W || !c.score || !c.choice) return fail(-1, "%s: null pointer", who);
    if (c.n_groups <= 0 || c.T <= 0 || c.transient < 0 || c.transient >= c.T || c.cols <= 0 || c.n_out <= 0)
        return fail(-1, "%s: invalid sizes (need n_groups, cols, n_out >= 1 and 0 <= transient < T)", who);
    if (c.n_ridge < 1 || c.n_ridge > 16)
        return fail(-1, "%s: n_ridge = %d, 1 to 16 candidates are served", who, c.n_ridge);
    if (c.n_out > 8) return fail(-1, "%s: n_out = %d, at most 8 outputs are served", who, c.n_out);
    const uintptr_t e = (uintptr_t)(c.E ? (const void*)c.E : (const void*)c.E32);
    if ((e | (uintptr_t)c.W) & 15) return fail(-1, "%s: E and W must be 16-byte aligned", who);
    return hip_fail(launch_holdout_score(c), who);
}

int esn_readout_holdout_score(const double* E, const double* D, const double* W, int n_groups, int T, int transient,
                              int cols, int n_out, const double* t_scale, const double* t_shift, int n_ridge,
                              const int* status_in, double* score, int* choice, void* stream) {
    return holdout_call("esn_readout_holdout_score",
                        {E, nullptr, D, W, n_groups, T, transient, cols, n_out, n_ridge, t_scale, t_shift, status_in,
                         score, choice, (hipStream_t)stream});
}

int esn_readout_holdout_score_f32(const float* E, const double* D, const double* W, int n_groups, int T, int transient,
                                  int cols, int n_out, const double* t_scale, const double* t_shift, int n_ridge,
                                  const int* status_in, double* score, int* choice, void* stream) {
    return holdout_call("esn_readout_holdout_score_f32",
                        {nullptr, E, D, W, n_groups, T, transient, cols, n_out, n_ridge, t_scale, t_shift, status_in,
                         score, choice, (hipStream_t)stream});
}

// ---- running normal equations (esn_gram.hip) ----------------------------------------------------------------------------
// Null pointers, sizes, "not served", workspace size, alignment -- the order of readout_call -- then the launch.
static int gram_accumulate_call(const char* who, const GramAccArgs& c) {
    if ((!c.E && !c.E32) || !c.D || !c.Gm || !c.Cm) return fail(-1, "%s: null pointer", who);
    if (c.n_groups <= 0 || c.T <= 0 || c.transient < 0 || c.transient >= c.T || c.cols <= 0 || c.n_out <= 0)
        return fail(-1, "%s: invalid sizes (need n_groups, cols, n_out >= 1 and 0 <= transient < T)", who);
    if (!(c.decay >= 0.0 && c.decay <= 1.0)) return fail(-1, "%s: decay = %g, it must lie in [0, 1]", who, c.decay);
    if (c.n_out > 16) return fail(-1, "%s: n_out = %d, at most 16 outputs are served", who, c.n_out);
    if (c.cols > gram_max_cols()) return fail(-2, "%s: cols = %d, the limit is %d", who, c.cols, gram_max_cols());
    const uintptr_t e = (uintptr_t)(c.E ? (const void*)c.E : (const void*)c.E32);
    if (e & 15) return fail(-1, "%s: E must be 16-byte aligned", who);
    return hip_fail(launch_gram_accumulate(c), who);
}

int esn_gram_accumulate(const double* E, const double* D, int n_groups, int T, int transient, int cols, int n_out,
                        const double* t_scale, const double* t_shift, double decay, double* Gm, double* Cm,
                        void* stream) {
    return gram_accumulate_call("esn_gram_accumulate", {E, nullptr, D, n_groups, T, transient, cols, n_out, t_scale,
                                                        t_shift, decay, Gm, Cm, (hipStream_t)stream});
}

int esn_gram_accumulate_f32(const float* E, const double* D, int n_groups, int T, int transient, int cols, int n_out,
                            const double* t_scale, const double* t_shift, double decay, double* Gm, double* Cm,
                            void* stream) {
    return gram_accumulate_call("esn_gram_accumulate_f32", {nullptr, E, D, n_groups, T, transient, cols, n_out, t_scale,
                                                            t_shift, decay, Gm, Cm, (hipStream_t)stream});
}

size_t esn_gram_solve_workspace_bytes(int n_groups, int n_ridge, int cols) {
    if (n_groups <= 0 || n_ridge <= 0 || cols <= 0 || cols > gram_max_cols()) return 0;
    return sizeof(double) * gram_solve_work_doubles(cols) * (size_t)n_groups;      // one factor per group, any n_ridge
}

int esn_gram_solve(const double* Gm, const double* Cm, int n_groups, int cols, int n_out, const double* ridge,
                   int n_ridge, double* W_out, int* status, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "esn_gram_solve";
    if (!Gm || !Cm || !ridge || !W_out || !status || !workspace) return fail(-1, "%s: null pointer", who);
    if (n_groups <= 0 || cols <= 0 || n_out <= 0)
        return fail(-1, "%s: invalid sizes (need n_groups, cols, n_out >= 1)", who);
    if (n_ridge < 1 || n_ridge > 16) return fail(-1, "%s: n_ridge = %d, 1 to 16 candidates are served", who, n_ridge);
    if (n_out > 16) return fail(-1, "%s: n_out = %d, at most 16 outputs are served", who, n_out);
    if (cols > gram_max_cols()) return fail(-2, "%s: cols = %d, the limit is %d", who, cols, gram_max_cols());
    const size_t need = esn_gram_solve_workspace_bytes(n_groups, n_ridge, cols);
    if (workspace_bytes < need)
        return fail(-1, "%s: workspace holds %zu bytes, esn_gram_solve_workspace_bytes says %zu", who, workspace_bytes,
                    need);
    if ((uintptr_t)workspace & 15) return fail(-1, "%s: the workspace must be 16-byte aligned", who);
    return hip_fail(launch_gram_solve({Gm, Cm, n_groups, cols, n_out, ridge, n_ridge, W_out, status, workspace,
                                       workspace_bytes, (hipStream_t)stream}), who);
}

// ---- reservoirs drawn on the device (esn_reservoir.hip) ------------------------------------------------------------
static const int kResMaxN = 4096;           // n_res: element counters of the draw and the tile grid stay far inside int

int esn_gen_reservoirs(int n_res, int n_in, int n_out, double sparsity, uint64_t seed, uint64_t first_set, int n_sets,
                       const double* uniforms, double* W, double* W_in, double* W_fb, void* stream) {
    const char* who = "esn_gen_reservoirs";
    if (!W || !W_in || !W_fb) return fail(-1, "%s: null pointer", who);
    if (n_res <= 0 || n_in <= 0 || n_out <= 0 || n_sets <= 0) return fail(-1, "%s: invalid sizes", who);
    if (n_res > kResMaxN || n_in > kResMaxN || n_out > kResMaxN)
        return fail(-1, "%s: n_res, n_in and n_out are served up to %d", who, kResMaxN);
    if (!(sparsity >= 0.0 && sparsity <= 1.0)) return fail(-1, "%s: sparsity = %g is outside [0, 1]", who, sparsity);
    return hip_fail(launch_gen_reservoirs(n_res, n_in, n_out, sparsity, seed, first_set, n_sets, uniforms, W, W_in,
                                          W_fb, (hipStream_t)stream), who);
}

size_t esn_spectral_radius_workspace_bytes(int n_sets, int n_res) {
    if (n_sets <= 0 || n_res <= 0) return 0;
    if (n_res > kResMaxN) {
        fail(-1, "esn_spectral_radius_workspace_bytes: n_res = %d, served up to %d", n_res, kResMaxN);
        return 0;
    }
    return sizeof(double) * specrad_work_doubles(n_res) * (size_t)n_sets;
}

int esn_spectral_radius_batch(const double* W, int n_sets, int n_res, int n_squarings, double* radius, int* status,
                              void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "esn_spectral_radius_batch";
    if (!W || !radius || !status) return fail(-1, "%s: null pointer", who);
    if (n_sets <= 0 || n_res <= 0) return fail(-1, "%s: invalid sizes", who);
    if (n_res > kResMaxN) return fail(-1, "%s: n_res = %d, served up to %d", who, n_res, kResMaxN);
    if (n_squarings < 4 || n_squarings > 32)
        return fail(-1, "%s: n_squarings = %d, 4 to 32 are served", who, n_squarings);
    const size_t need = esn_spectral_radius_workspace_bytes(n_sets, n_res);
    if (!workspace || workspace_bytes < need)
        return fail(-1, "%s: workspace holds %zu bytes, esn_spectral_radius_workspace_bytes says %zu", who,
                    workspace ? workspace_bytes : (size_t)0, need);
    if ((uintptr_t)workspace & 7) return fail(-1, "%s: the workspace must be 8-byte aligned", who);
    return hip_fail(launch_spectral_radius(W, n_sets, n_res, n_squarings, radius, status, workspace,
                                           (hipStream_t)stream), who);
}

// (16 bytes more than the images take: the 8-byte aligned workspace of the caller is rounded up to the 16 bytes the
//  kernel's loads want)
size_t esn_spectral_radius_split_workspace_bytes(int n_sets, int n_res) {
    if (n_sets <= 0 || n_res <= 0) return 0;
    if (n_res > kResMaxN) {
        fail(-1, "esn_spectral_radius_split_workspace_bytes: n_res = %d, served up to %d", n_res, kResMaxN);
        return 0;
    }
    return specrad_split_work_bytes(n_res) * (size_t)n_sets + 16;
}

int esn_spectral_radius_split_batch(const double* W, int n_sets, int n_res, int n_squarings, double* radius,
                                    int* status, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "esn_spectral_radius_split_batch";
    if (!W || !radius || !status) return fail(-1, "%s: null pointer", who);
    if (n_sets <= 0 || n_res <= 0) return fail(-1, "%s: invalid sizes", who);
    if (n_res > kResMaxN) return fail(-1, "%s: n_res = %d, served up to %d", who, n_res, kResMaxN);
    if (n_squarings < 4 || n_squarings > 32)
        return fail(-1, "%s: n_squarings = %d, 4 to 32 are served", who, n_squarings);
    const size_t need = specrad_split_work_bytes(n_res) * (size_t)n_sets + 16;
    if (!workspace || workspace_bytes < need)
        return fail(-1, "%s: workspace holds %zu bytes, esn_spectral_radius_split_workspace_bytes says %zu", who,
                    workspace ? workspace_bytes : (size_t)0, need);
    if ((uintptr_t)workspace & 7) return fail(-1, "%s: the workspace must be 8-byte aligned", who);
    void* aligned = reinterpret_cast<void*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
    return hip_fail(launch_spectral_radius_split(W, n_sets, n_res, n_squarings, radius, status, aligned,
                                                 (hipStream_t)stream), who);
}

int esn_scale_reservoirs(double* W, int n_sets, int n_res, double rho, const double* radius, const int* status,
                         void* stream) {
    const char* who = "esn_scale_reservoirs";
    if (!W || !radius || !status) return fail(-1, "%s: null pointer", who);
    if (n_sets <= 0 || n_res <= 0) return fail(-1, "%s: invalid sizes", who);
    if (n_res > kResMaxN) return fail(-1, "%s: n_res = %d, served up to %d", who, n_res, kResMaxN);
    if (!(rho > 0.0 && rho <= 1.7976931348623157e308)) return fail(-1, "%s: rho = %g must be positive and finite", who, rho);
    return hip_fail(launch_scale_reservoirs(W, n_sets, n_res, rho, radius, status, (hipStream_t)stream), who);
}

static int pow2_log(int n) { int l = 0; while ((1 << l) < n) ++l; return ((1 << l) == n) ? l : -1; }

// the checks the OFDM entry points share: 0 (and *log2n = log2 N), or the failure recorded
static int check_n_sub(const char* who, int n_sub, int* log2n) {
    *log2n = pow2_log(n_sub);
    if (*log2n < 1 || n_sub > 2048) return fail(-1, "%s: N=%d must be a power of two in [2, 2048]", who, n_sub);
    return 0;
}
static int check_square_qam(const char* who, int bits_per_sym) {
    if (bits_per_sym < 2 || bits_per_sym > 10 || (bits_per_sym & 1))
        return fail(-1, "%s: bits_per_sym=%d must be even (square QAM)", who, bits_per_sym);
    return 0;
}

static int detect_common(const char* who, bool io32, const void* Y, int n_frames, int frames_per_group, int n_sub,
                         int n_t, int bits_per_sym, const double* p_i, const uint8_t* tx_bits, long long* err_count,
                         long long* bit_count, double* X_hat, void* stream) {
    if (!Y || !p_i || !tx_bits || !err_count || !bit_count) return fail(-1, "%s: null pointer", who);
    if (n_frames <= 0 || frames_per_group <= 0 || n_t <= 0) return fail(-1, "%s: invalid sizes", who);
    int log2n;
    if (int rc = check_n_sub(who, n_sub, &log2n)) return rc;
    if (int rc = check_square_qam(who, bits_per_sym)) return rc;
    if (io32 && ((uintptr_t)Y & 7) != 0) return fail(-1, "%s: Y must be 8-byte aligned", who);
    DetectParams dp;
    if (io32) dp.Y32 = static_cast<const float*>(Y); else dp.Y = static_cast<const double*>(Y);
    dp.n_frames = n_frames; dp.frames_per_group = frames_per_group; dp.n_sub = n_sub;
    dp.log2n = log2n; dp.n_t = n_t; dp.m = bits_per_sym; dp.p_i = p_i; dp.tx_bits = tx_bits;
    dp.err = err_count; dp.bits = bit_count; dp.X_hat = X_hat;
    return hip_fail(launch_detect_count(dp, (hipStream_t)stream, io32), who);
}

int esn_detect_count(const double* Y, int n_frames, int frames_per_group, int n_sub, int n_t, int bits_per_sym,
                     const double* p_i, const uint8_t* tx_bits, long long* err_count, long long* bit_count,
                     double* X_hat, void* stream) {
    return detect_common("esn_detect_count", false, Y, n_frames, frames_per_group, n_sub, n_t, bits_per_sym, p_i,
                         tx_bits, err_count, bit_count, X_hat, stream);
}

int esn_detect_count_f32(const float* Y, int n_frames, int frames_per_group, int n_sub, int n_t, int bits_per_sym,
                         const double* p_i, const uint8_t* tx_bits, long long* err_count, long long* bit_count,
                         double* X_hat, void* stream) {
    return detect_common("esn_detect_count_f32", true, Y, n_frames, frames_per_group, n_sub, n_t, bits_per_sym, p_i,
                         tx_bits, err_count, bit_count, X_hat, stream);
}

static int detect_ens_common(const char* who, bool io32, const void* Y, int n_members, int n_frames,
                             int frames_per_group, int n_sub, int n_t, int bits_per_sym, const double* p_i,
                             const double* weights, const uint8_t* tx_bits, long long* err_count, long long* bit_count,
                             long long* member_err, double* X_hat, void* stream) {
    if (!Y || !p_i || !tx_bits || !err_count || !bit_count) return fail(-1, "%s: null pointer", who);
    if (n_members < 1 || n_members > 16) return fail(-1, "%s: n_members=%d, 1 to 16 are served", who, n_members);
    if (n_frames <= 0 || frames_per_group <= 0 || n_t <= 0) return fail(-1, "%s: invalid sizes", who);
    if (n_t > 16) return fail(-1, "%s: n_t=%d, served up to 16", who, n_t);
    int log2n;
    if (int rc = check_n_sub(who, n_sub, &log2n)) return rc;
    if (int rc = check_square_qam(who, bits_per_sym)) return rc;
    if (((uintptr_t)Y & (io32 ? 7 : 15)) != 0) return fail(-1, "%s: Y must be %d-byte aligned", who, io32 ? 8 : 16);
    EnsParams ep;
    DetectParams& dp = ep.d;
    if (io32) dp.Y32 = static_cast<const float*>(Y); else dp.Y = static_cast<const double*>(Y);
    dp.n_frames = n_frames; dp.frames_per_group = frames_per_group; dp.n_sub = n_sub;
    dp.log2n = log2n; dp.n_t = n_t; dp.m = bits_per_sym; dp.p_i = p_i; dp.tx_bits = tx_bits;
    dp.err = err_count; dp.bits = bit_count; dp.X_hat = X_hat; dp.na_wg = 0;
    ep.n_members = n_members; ep.weights = weights; ep.member_err = member_err;
    return hip_fail(launch_detect_count_ens(ep, (hipStream_t)stream, io32), who);
}

int esn_detect_count_ens(const double* Y, int n_members, int n_frames, int frames_per_group, int n_sub, int n_t,
                         int bits_per_sym, const double* p_i, const double* weights, const uint8_t* tx_bits,
                         long long* err_count, long long* bit_count, long long* member_err, double* X_hat,
                         void* stream) {
    return detect_ens_common("esn_detect_count_ens", false, Y, n_members, n_frames, frames_per_group, n_sub, n_t,
                             bits_per_sym, p_i, weights, tx_bits, err_count, bit_count, member_err, X_hat, stream);
}

int esn_detect_count_ens_f32(const float* Y, int n_members, int n_frames, int frames_per_group, int n_sub, int n_t,
                             int bits_per_sym, const double* p_i, const double* weights, const uint8_t* tx_bits,
                             long long* err_count, long long* bit_count, long long* member_err, double* X_hat,
                             void* stream) {
    return detect_ens_common("esn_detect_count_ens_f32", true, Y, n_members, n_frames, frames_per_group, n_sub, n_t,
                             bits_per_sym, p_i, weights, tx_bits, err_count, bit_count, member_err, X_hat, stream);
}

int esn_detect_remod(const double* Y, int n_frames, int frames_per_group, int n_sub, int cp, int delay, int n_t,
                     int bits_per_sym, const double* p_i, const uint8_t* tx_bits, long long* err_count,
                     long long* bit_count, double* X_hat, uint8_t* dec_bits, double* D_hat, void* stream) {
    const char* who = "esn_detect_remod";
    if (!Y || !p_i || !D_hat) return fail(-1, "%s: null pointer", who);
    if (tx_bits && (!err_count || !bit_count)) return fail(-1, "%s: tx_bits given without err_count / bit_count", who);
    if (n_frames <= 0 || frames_per_group <= 0 || n_t <= 0) return fail(-1, "%s: invalid sizes", who);
    if (n_t > 16) return fail(-1, "%s: n_t=%d, served up to 16", who, n_t);
    int log2n;
    if (int rc = check_n_sub(who, n_sub, &log2n)) return rc;
    if (int rc = check_square_qam(who, bits_per_sym)) return rc;
    if (cp < 0 || cp >= n_sub) return fail(-1, "%s: cp=%d must be in [0, N) with N=%d", who, cp, n_sub);
    if (delay < 0 || delay > (1 << 20)) return fail(-1, "%s: delay=%d must be in [0, %d]", who, delay, 1 << 20);
    RemodParams rp;
    rp.d.Y = Y;
    rp.d.n_frames = n_frames; rp.d.frames_per_group = frames_per_group; rp.d.n_sub = n_sub;
    rp.d.log2n = log2n; rp.d.n_t = n_t; rp.d.m = bits_per_sym; rp.d.p_i = p_i; rp.d.tx_bits = tx_bits;
    rp.d.err = tx_bits ? err_count : nullptr; rp.d.bits = tx_bits ? bit_count : nullptr; rp.d.X_hat = X_hat;
    rp.d.na_wg = 0;
    rp.cp = cp; rp.delay = delay; rp.dec_bits = dec_bits; rp.D_hat = D_hat;
    return hip_fail(launch_detect_remod(rp, (hipStream_t)stream), who);
}

static const double kTdlbDelay[23] = {0.0000, 0.1072, 0.2155, 0.2095, 0.2870, 0.2986, 0.3752, 0.5055, 0.3681,
                                      0.3697, 0.5700, 0.5283, 1.1021, 1.2756, 1.5474, 1.7842, 2.0169, 2.8294,
                                      3.0219, 3.6187, 4.1067, 4.2790, 4.7834};
static const double kTdlbPowDb[23] = {0.0, -2.2, -4.0, -3.2, -9.8, -1.2, -3.4, -5.2, -7.6, -3.0, -8.9, -9.0,
                                      -4.8, -5.7, -7.5, -1.9, -7.6, -12.2, -9.8, -11.4, -14.9, -9.2, -11.3};

// kind, isi, paths, powers and delays of a TapParams (kinds 0 and 1 shared with esn_gen_taps_doppler)
static void tap_tables(TapParams& tp, int kind, int isi, double fs_hz, double ds_ns) {
    tp.kind = kind; tp.isi = isi;
    if (kind == 0) {
        tp.n_paths = 23;
        double sum = 0.0;
        for (int i = 0; i < 23; ++i) sum += pow(10.0, kTdlbPowDb[i] / 10.0);
        for (int i = 0; i < 23; ++i) {
            tp.path_sqrt_pow[i] = sqrt(pow(10.0, kTdlbPowDb[i] / 10.0) / sum);
            tp.path_delay_samples[i] = kTdlbDelay[i] * ds_ns * 1e-9 * fs_hz;
        }
    } else if (kind == 1) {
        tp.n_paths = isi;
        const int cp = isi - 1;
        const double tc = (cp / 9.0 > 1e-12) ? cp / 9.0 : 1e-12;
        double sum = 0.0;
        for (int i = 0; i < isi; ++i) sum += exp(-(double)i / tc);
        for (int i = 0; i < isi; ++i) tp.path_sqrt_pow[i] = sqrt(exp(-(double)i / tc) / sum);
    } else {
        tp.n_paths = 1;
        tp.path_sqrt_pow[0] = 1.0;
    }
}

int esn_gen_taps(int kind, int n_blocks, int n_r, int n_t, int isi, double fs_hz, double ds_ns,
                 const double* gains_in, uint64_t seed, uint64_t link_offset, double* taps, void* stream) {
    if (!taps) return fail(-1, "esn_gen_taps: null pointer");
    if (kind < 0 || kind > 2 || n_blocks <= 0 || n_r <= 0 || n_t <= 0 || isi <= 0 || isi > 16)
        return fail(-1, "esn_gen_taps: invalid arguments (kind=%d isi=%d)", kind, isi);
    TapParams tp;
    memset(&tp, 0, sizeof(tp));
    tap_tables(tp, kind, isi, fs_hz, ds_ns);
    tp.n_links = n_blocks * n_r * n_t;
    tp.gains_in = gains_in; tp.seed = seed; tp.link_offset = link_offset; tp.taps = taps;
    return hip_fail(launch_gen_taps(tp, (hipStream_t)stream), "esn_gen_taps");
}

int esn_gen_taps_doppler(int kind, int n_blocks, int n_sym, int n_r, int n_t, int isi, double fs_hz, double ds_ns,
                         double fd_tsym, const double* angles_in, uint64_t seed, uint64_t link_offset, double* taps,
                         void* stream) {
    const char* who = "esn_gen_taps_doppler";
    if (!taps) return fail(-1, "%s: null pointer", who);
    if (kind < 0 || kind > 1) return fail(-1, "%s: kind=%d must be 0 (TDL-B) or 1 (exponential PDP)", who, kind);
    if (n_blocks <= 0 || n_r <= 0 || n_t <= 0) return fail(-1, "%s: invalid sizes", who);
    if (n_sym < 1 || n_sym > 4096) return fail(-1, "%s: n_sym=%d must be in [1, 4096]", who, n_sym);
    if (isi < 1 || isi > 16) return fail(-1, "%s: isi=%d must be in [1, 16]", who, isi);
    if (!(fd_tsym >= 0.0 && fd_tsym <= 0.5))
        return fail(-1, "%s: fd_tsym=%g must be in [0, 0.5] cycles per symbol", who, fd_tsym);
    if ((long long)n_blocks * n_r * n_t > 0x7fffffffLL) return fail(-1, "%s: more than 2^31 - 1 links", who);
    DopplerParams dp;
    memset(&dp, 0, sizeof(dp));
    tap_tables(dp.tp, kind, isi, fs_hz, ds_ns);
    dp.tp.n_links = n_blocks * n_r * n_t;
    dp.tp.seed = seed; dp.tp.link_offset = link_offset; dp.tp.taps = taps;
    dp.n_sym = n_sym; dp.links_per_block = n_r * n_t; dp.fd_tsym = fd_tsym; dp.angles_in = angles_in;
    return hip_fail(launch_gen_taps_doppler(dp, (hipStream_t)stream), who);
}

static int gen_common(const char* who, bool c64, int n_frames, int frames_per_block, int n_sub, int cp, int n_t,
                      int n_r, int isi, int bits_per_sym, int ls_pattern, const double* p_i, const double* a_clip,
                      double no, const double* taps, const uint8_t* bits_in, const double* noise_in, uint64_t seed,
                      uint64_t frame_offset, uint8_t* bits, void* x_cp, void* y_cp, void* stream) {
    if (!p_i || !a_clip || !taps || !bits || !y_cp) return fail(-1, "%s: null pointer", who);
    int log2n;
    if (int rc = check_n_sub(who, n_sub, &log2n)) return rc;
    if (int rc = check_square_qam(who, bits_per_sym)) return rc;
    if (n_frames <= 0 || frames_per_block <= 0 || cp < 0 || cp >= n_sub || n_t <= 0 || n_r <= 0 || isi <= 0)
        return fail(-1, "%s: invalid sizes", who);
    if (c64 && ((((uintptr_t)y_cp) | ((uintptr_t)x_cp)) & 7) != 0)
        return fail(-1, "%s: x_cp / y_cp must be 8-byte aligned (complex64)", who);
    FrameGenParams fp;
    fp.n_frames = n_frames; fp.frames_per_block = frames_per_block; fp.n_sub = n_sub; fp.log2n = log2n;
    fp.cp = cp; fp.n_t = n_t; fp.n_r = n_r; fp.isi = isi; fp.m = bits_per_sym;
    fp.p_i = p_i; fp.a_clip = a_clip; fp.no = no; fp.taps = taps; fp.bits_in = bits_in; fp.noise_in = noise_in;
    fp.seed = seed; fp.frame_offset = frame_offset; fp.bits = bits;
    if (c64) { fp.x_cp32 = static_cast<float*>(x_cp); fp.y_cp32 = static_cast<float*>(y_cp); }
    else { fp.x_cp = static_cast<double*>(x_cp); fp.y_cp = static_cast<double*>(y_cp); }
    fp.ls_pattern = ls_pattern ? 1 : 0;
    fp.ko = knobs().gen_ko;
    int e = launch_gen_frames(fp, (hipStream_t)stream, c64);
    if (e == -1) return fail(-2, "%s: frame does not fit LDS", who);
    return hip_fail(e, who);
}

int esn_gen_frames(int n_frames, int frames_per_block, int n_sub, int cp, int n_t, int n_r, int isi,
                   int bits_per_sym, int ls_pattern, const double* p_i, const double* a_clip, double no, const double* taps,
                   const uint8_t* bits_in, const double* noise_in, uint64_t seed, uint64_t frame_offset,
                   uint8_t* bits, double* x_cp, double* y_cp, void* stream) {
    return gen_common("esn_gen_frames", false, n_frames, frames_per_block, n_sub, cp, n_t, n_r, isi, bits_per_sym,
                      ls_pattern, p_i, a_clip, no, taps, bits_in, noise_in, seed, frame_offset, bits, x_cp, y_cp, stream);
}

int esn_gen_frames_c64(int n_frames, int frames_per_block, int n_sub, int cp, int n_t, int n_r, int isi,
                       int bits_per_sym, int ls_pattern, const double* p_i, const double* a_clip, double no,
                       const double* taps, const uint8_t* bits_in, const double* noise_in, uint64_t seed,
                       uint64_t frame_offset, uint8_t* bits, float* x_cp, float* y_cp, void* stream) {
    return gen_common("esn_gen_frames_c64", true, n_frames, frames_per_block, n_sub, cp, n_t, n_r, isi, bits_per_sym,
                      ls_pattern, p_i, a_clip, no, taps, bits_in, noise_in, seed, frame_offset, bits, x_cp, y_cp, stream);
}

int esn_channel_estimate(int n_blocks, int n_sub, int cp, int n_t, int n_r, int isi, int bits_per_sym,
                         const double* p_i, double no, const uint8_t* pilot_bits, const double* y_ls_cp,
                         int ls_only, double* H, void* stream) {
    if (!p_i || !pilot_bits || !y_ls_cp || !H) return fail(-1, "esn_channel_estimate: null pointer");
    int l2;
    if (int rc = check_n_sub("esn_channel_estimate", n_sub, &l2)) return rc;
    if (n_blocks <= 0 || cp < 0 || cp >= n_sub || n_t <= 0 || n_r <= 0 || isi <= 0 || isi > 64 || n_sub / n_t < 2 ||
        bits_per_sym < 2 || (bits_per_sym & 1))
        return fail(-1, "esn_channel_estimate: invalid sizes");
    ChanEstParams c;
    c.n_blocks = n_blocks; c.n_sub = n_sub; c.log2n = l2; c.cp = cp; c.n_t = n_t; c.n_r = n_r; c.isi = isi;
    c.m = bits_per_sym; c.p_i = p_i; c.no = no; c.pilot_bits = pilot_bits; c.y_ls_cp = y_ls_cp; c.H = H;
    c.ls_only = ls_only ? 1 : 0;
    int e = launch_channel_estimate(c, (hipStream_t)stream);
    if (e == -1)
        return fail(-2, "esn_channel_estimate: N=%d n_t=%d isi=%d needs %zu bytes of LDS, %zu are served", n_sub, n_t, isi,
                    channel_estimate_lds_bytes(n_sub, n_t, isi), MMSE_LDS_MAX);
    return hip_fail(e, "esn_channel_estimate");
}

static int linear_detect(const char* who, int zf, int n_frames, int frames_per_group, int n_sub, int cp, int n_t, int n_r,
                         int bits_per_sym, const double* p_i, double no, const double* H, const double* y_cp,
                         const uint8_t* tx_bits, long long* err_count, long long* bit_count, double* X_hat,
                         void* stream) {
    if (!p_i || !H || !y_cp || !tx_bits || !err_count || !bit_count)
        return fail(-1, "%s: null pointer", who);
    int l2;
    if (int rc = check_n_sub(who, n_sub, &l2)) return rc;
    if (n_frames <= 0 || frames_per_group <= 0 || cp < 0 || cp >= n_sub || n_t <= 0 || n_r <= 0 ||
        bits_per_sym < 2 || (bits_per_sym & 1))
        return fail(-1, "%s: invalid sizes", who);
    MmseParams m;
    m.n_frames = n_frames; m.frames_per_group = frames_per_group; m.n_sub = n_sub; m.log2n = l2; m.cp = cp;
    m.n_t = n_t; m.n_r = n_r; m.m = bits_per_sym; m.zf = zf; m.p_i = p_i; m.no = no; m.H = H; m.y_cp = y_cp;
    m.tx_bits = tx_bits; m.err = err_count; m.bits = bit_count; m.X_hat = X_hat;
    int e = launch_mmse_detect(m, (hipStream_t)stream);
    if (e == -1) return fail(-2, "%s: needs n_t <= 4 and n_r * N * 16 bytes of LDS", who);
    return hip_fail(e, who);
}

int esn_mmse_detect_count(int n_frames, int frames_per_group, int n_sub, int cp, int n_t, int n_r, int bits_per_sym,
                          const double* p_i, double no, const double* H, const double* y_cp,
                          const uint8_t* tx_bits, long long* err_count, long long* bit_count, double* X_hat,
                          void* stream) {
    return linear_detect("esn_mmse_detect_count", 0, n_frames, frames_per_group, n_sub, cp, n_t, n_r, bits_per_sym, p_i,
                         no, H, y_cp, tx_bits, err_count, bit_count, X_hat, stream);
}

int esn_zf_detect_count(int n_frames, int frames_per_group, int n_sub, int cp, int n_t, int n_r, int bits_per_sym,
                        const double* p_i, const double* H, const double* y_cp, const uint8_t* tx_bits,
                        long long* err_count, long long* bit_count, double* X_hat, void* stream) {
    return linear_detect("esn_zf_detect_count", 1, n_frames, frames_per_group, n_sub, cp, n_t, n_r, bits_per_sym, p_i,
                         0.0, H, y_cp, tx_bits, err_count, bit_count, X_hat, stream);
}

static int equalize_rows(const char* who, bool io32, int n_frames, int frames_per_group, int n_sub, int cp, int pad,
                         int n_t, int n_r, const double* p_i, double no, const double* H, const double* y_cp,
                         void* U_eq, double* X_hat, void* stream) {
    if (!p_i || !H || !y_cp || !U_eq) return fail(-1, "%s: null pointer", who);
    int l2;
    if (int rc = check_n_sub(who, n_sub, &l2)) return rc;
    if (n_frames <= 0 || frames_per_group <= 0 || n_t <= 0 || n_r <= 0) return fail(-1, "%s: invalid sizes", who);
    if (n_t > 4) return fail(-1, "%s: n_t=%d, served up to 4", who, n_t);
    if (cp < 0 || cp >= n_sub) return fail(-1, "%s: cp=%d must be in [0, N) with N=%d", who, cp, n_sub);
    if (pad < 0 || pad > (1 << 20)) return fail(-1, "%s: pad=%d must be in [0, %d]", who, pad, 1 << 20);
    if (equalize_rows_lds_bytes(n_sub, n_t, n_r) > MMSE_LDS_MAX)
        return fail(-1, "%s: n_r=%d needs 16 (max(n_r, n_t) N + N/2) = %zu bytes of LDS; N=%d serves n_r up to %d (%zu bytes)",
                    who, n_r, equalize_rows_lds_bytes(n_sub, n_t, n_r), n_sub,
                    (int)((MMSE_LDS_MAX - (size_t)n_sub * 8) / ((size_t)n_sub * 16)), MMSE_LDS_MAX);
    if (((uintptr_t)U_eq & (io32 ? 7 : 15)) != 0)
        return fail(-1, "%s: U_eq must be %d-byte aligned", who, io32 ? 8 : 16);
    EqRowsParams ep;
    ep.n_frames = n_frames; ep.frames_per_group = frames_per_group; ep.n_sub = n_sub; ep.log2n = l2; ep.cp = cp;
    ep.pad = pad; ep.n_t = n_t; ep.n_r = n_r; ep.p_i = p_i; ep.no = no; ep.H = H; ep.y_cp = y_cp; ep.U_eq = U_eq;
    ep.X_hat = X_hat;
    return hip_fail(launch_equalize_rows(ep, (hipStream_t)stream, io32), who);
}

int esn_mmse_equalize_rows(int n_frames, int frames_per_group, int n_sub, int cp, int pad, int n_t, int n_r,
                           const double* p_i, double no, const double* H, const double* y_cp, double* U_eq,
                           double* X_hat, void* stream) {
    return equalize_rows("esn_mmse_equalize_rows", false, n_frames, frames_per_group, n_sub, cp, pad, n_t, n_r, p_i, no,
                         H, y_cp, U_eq, X_hat, stream);
}

int esn_mmse_equalize_rows_f32(int n_frames, int frames_per_group, int n_sub, int cp, int pad, int n_t, int n_r,
                               const double* p_i, double no, const double* H, const double* y_cp, float* U_eq,
                               double* X_hat, void* stream) {
    return equalize_rows("esn_mmse_equalize_rows_f32", true, n_frames, frames_per_group, n_sub, cp, pad, n_t, n_r, p_i,
                         no, H, y_cp, U_eq, X_hat, stream);
}

// ---- amplifier-aware LS-MMSE (esn_dcc.hip): every refusal below comes before any HIP call
size_t esn_mmse_dcc_lds_bytes(int n_sub, int n_t, int n_r) {
    if (n_sub <= 0 || n_t <= 0 || n_r <= 0) return 0;
    return mmse_dcc_lds_bytes(n_sub, n_t, n_r);
}

int esn_mmse_dcc_detect_count(int n_frames, int frames_per_group, int n_sub, int cp, int n_t, int n_r, int bits_per_sym,
                              int n_iter, const double* p_i, const double* a_clip, double no, const double* H,
                              const double* y_cp, const uint8_t* tx_bits, long long* err_count, long long* bit_count,
                              long long* err_iter, double* X_hat, void* stream) {
    const char* who = "esn_mmse_dcc_detect_count";
    if (!p_i) return fail(-1, "%s: p_i is NULL", who);
    if (!a_clip) return fail(-1, "%s: a_clip is NULL", who);
    if (!H) return fail(-1, "%s: H is NULL", who);
    if (!y_cp) return fail(-1, "%s: y_cp is NULL", who);
    if (tx_bits && (!err_count || !bit_count)) return fail(-1, "%s: tx_bits needs err_count and bit_count", who);
    if (!tx_bits && !X_hat) return fail(-1, "%s: tx_bits and X_hat are both NULL: nothing to compute", who);
    int l2;
    if (int rc = check_n_sub(who, n_sub, &l2)) return rc;
    if (n_frames <= 0) return fail(-1, "%s: n_frames=%d must be positive", who, n_frames);
    if (frames_per_group <= 0) return fail(-1, "%s: frames_per_group=%d must be positive", who, frames_per_group);
    if (cp < 0 || cp >= n_sub) return fail(-1, "%s: cp=%d must be in [0, N) with N=%d", who, cp, n_sub);
    if (n_t < 1 || n_t > 4) return fail(-1, "%s: n_t=%d must be in [1, 4]", who, n_t);
    if (n_r < 1) return fail(-1, "%s: n_r=%d must be positive", who, n_r);
    if (int rc = check_square_qam(who, bits_per_sym)) return rc;
    if (mmse_dcc_lds_bytes(n_sub, n_t, n_r) > MMSE_LDS_MAX)
        return fail(-1, "%s: N=%d n_t=%d n_r=%d needs 16 ((n_r + 2 n_t) N + N/2) = %zu bytes of LDS, %zu are served", who,
                    n_sub, n_t, n_r, mmse_dcc_lds_bytes(n_sub, n_t, n_r), MMSE_LDS_MAX);
    if (n_iter < 0 || n_iter > DCC_MAX_ITER) return fail(-1, "%s: n_iter=%d must be in [0, %d]", who, n_iter, DCC_MAX_ITER);
    DccParams d;
    d.n_frames = n_frames; d.frames_per_group = frames_per_group; d.n_sub = n_sub; d.log2n = l2; d.cp = cp; d.n_t = n_t;
    d.n_r = n_r; d.m = bits_per_sym; d.n_iter = n_iter; d.p_i = p_i; d.a_clip = a_clip; d.no = no; d.H = H; d.y_cp = y_cp;
    d.tx_bits = tx_bits; d.err = err_count; d.bits = bit_count; d.err_iter = err_iter; d.X_hat = X_hat;
    return hip_fail(launch_mmse_dcc(d, (hipStream_t)stream), who);
}

int esn_channel_track(const double* y_cp, const double* X_hat, const uint8_t* bits, int n_est, int window,
                      int est_per_group, int n_sub, int cp, int n_t, int n_r, int isi, int bits_per_sym,
                      const double* p_i, const double* reg, double* taps, double* H, int* status, void* stream) {
    const char* who = "esn_channel_track";
    if (!y_cp || !p_i || !reg || !H || !status) return fail(-1, "%s: null pointer", who);
    if ((X_hat != nullptr) == (bits != nullptr)) return fail(-1, "%s: exactly one of X_hat and bits must be given", who);
    if (n_est <= 0 || est_per_group <= 0) return fail(-1, "%s: invalid sizes", who);
    if (window < 1 || window > 8) return fail(-1, "%s: window=%d must be in [1, 8]", who, window);
    if ((long long)n_est * window > 0x7fffffffLL) return fail(-1, "%s: more than 2^31 - 1 frames", who);
    int l2;
    if (int rc = check_n_sub(who, n_sub, &l2)) return rc;
    if (n_t < 1 || n_t > 4) return fail(-1, "%s: n_t=%d must be in [1, 4]", who, n_t);
    if (n_r < 1 || n_r > 8) return fail(-1, "%s: n_r=%d must be in [1, 8]", who, n_r);
    if (isi < 1 || isi > 16) return fail(-1, "%s: isi=%d must be in [1, 16]", who, isi);
    if (n_t * isi > 64 || n_t * isi > n_sub)
        return fail(-1, "%s: n_t * isi = %d unknowns, served up to min(64, N) with N=%d", who, n_t * isi, n_sub);
    if (cp < 0 || cp >= n_sub) return fail(-1, "%s: cp=%d must be in [0, N) with N=%d", who, cp, n_sub);
    if (bits_per_sym < 2 || bits_per_sym > 10 || (bits_per_sym & 1))
        return fail(-1, "%s: bits_per_sym=%d must be even (square QAM) in [2, 10]", who, bits_per_sym);
    const size_t lds = chantrack_lds_bytes(n_sub, n_t, n_r, isi);
    if (lds > 150 * 1024)
        return fail(-1, "%s: N=%d n_t=%d n_r=%d isi=%d needs %zu bytes of LDS, served up to %d", who, n_sub, n_t, n_r,
                    isi, lds, 150 * 1024);
    if ((((uintptr_t)y_cp) | ((uintptr_t)X_hat) | ((uintptr_t)taps) | ((uintptr_t)H)) & 15)
        return fail(-1, "%s: y_cp, X_hat, taps and H must be 16-byte aligned", who);
    ChanTrackParams c;
    c.n_est = n_est; c.window = window; c.est_per_group = est_per_group; c.n_sub = n_sub; c.log2n = l2; c.cp = cp;
    c.n_t = n_t; c.n_r = n_r; c.isi = isi; c.m = bits_per_sym; c.y_cp = y_cp; c.X_hat = X_hat; c.bits = bits;
    c.p_i = p_i; c.reg = reg; c.taps = taps; c.H = H; c.status = status; c.n_seg = 0; c.log2m2 = 0;
    return hip_fail(launch_channel_track(c, (hipStream_t)stream), who);
}

// n_out ahead of elm_check, where esn_elm_predict and the FNN pair call with it (elm_check reads n_out = 0 as "features")
static int n_out_check(const char* who, int n_out) {
    if (n_out < 1 || n_out > 8) return fail(-1, "%s: n_out=%d must be in [1, 8]", who, n_out);
    return 0;
}

// the checks esn_elm_features and esn_elm_predict share; n_out = 0: features
static int elm_check(const char* who, int precision, int n_in, int n_hidden, int window, int bias_col, int n_wsets,
                     int n_out, int e_cols, int n_seq, int seq_per_group, int T_in, int T, int transient) {
    if (precision == ESN_F32 || precision == ESN_BF16)
        return fail(-2, "%s: precision %d is not built: ESN_F64 and (predict) ESN_F16 are", who, precision);
    if (precision != ESN_F64 && precision != ESN_F16) return fail(-1, "%s: unknown precision %d", who, precision);
    if (n_in < 1) return fail(-1, "%s: n_in=%d must be positive", who, n_in);
    if (window < 1 || window > 16) return fail(-1, "%s: window=%d must be in [1, 16]", who, window);
    if ((long long)window * n_in > 256)
        return fail(-1, "%s: window * n_in = %lld, served up to K = 256", who, (long long)window * n_in);
    if (n_hidden < 1 || n_hidden > 1024) return fail(-1, "%s: n_hidden=%d must be in [1, 1024]", who, n_hidden);
    if (bias_col != 0 && bias_col != 1) return fail(-1, "%s: bias_col=%d must be 0 or 1", who, bias_col);
    if (n_wsets < 1) return fail(-1, "%s: n_wsets=%d must be positive", who, n_wsets);
    if (n_out && (n_out < 1 || n_out > 8)) return fail(-1, "%s: n_out=%d must be in [1, 8]", who, n_out);
    if (e_cols < n_hidden + bias_col || e_cols > n_hidden + 4)
        return fail(-1, "%s: e_cols=%d must be in [n_hidden + bias_col, n_hidden + 4] = [%d, %d]", who, e_cols,
                    n_hidden + bias_col, n_hidden + 4);
    if (n_seq < 1 || seq_per_group < 1) return fail(-1, "%s: invalid sizes (sequences, frames per group)", who);
    if (T_in < 1 || T_in > T || T > (1 << 20))
        return fail(-1, "%s: need 1 <= T_in <= T <= 2^20 (T_in=%d, T=%d)", who, T_in, T);
    if (window > T) return fail(-1, "%s: window=%d exceeds T=%d", who, window, T);
    if (transient < 0 || transient >= T) return fail(-1, "%s: transient=%d must be in [0, T) with T=%d", who, transient, T);
    if ((long long)n_seq * ((T + 15) / 16) > 0x7fffffffLL)
        return fail(-1, "%s: more than 2^31 - 1 tiles of 16 rows", who);
    return 0;
}

int esn_elm_features(int precision, int n_in, int n_hidden, int window, int bias_col, int n_wsets, const double* W_in,
                     const double* b, const double* in_scale, const double* in_shift, const double* U, int n_groups,
                     int T_in, int T, uint64_t group_offset, void* E, int e_f32, int e_cols, void* stream) {
    const char* who = "esn_elm_features";
    if (!W_in || !b || !U || !E) return fail(-1, "%s: null pointer", who);
    const int rc = elm_check(who, precision, n_in, n_hidden, window, bias_col, n_wsets, 0, e_cols, n_groups, 1, T_in, T, 0);
    if (rc) return rc;
    if (precision != ESN_F64)
        return fail(-2, "%s: features are float64 arithmetic (ESN_F64); ESN_F16 is served by esn_elm_predict", who);
    if ((uintptr_t)E & 15) return fail(-1, "%s: E must be 16-byte aligned", who);
    ElmParams p;
    memset(&p, 0, sizeof(p));
    p.n_in = n_in; p.n_hidden = n_hidden; p.window = window; p.bias_col = bias_col; p.n_wsets = n_wsets; p.n_out = 1;
    p.e_cols = e_cols; p.n_seq = n_groups; p.seq_per_group = 1; p.T_in = T_in; p.T = T; p.transient = 0;
    p.group_offset = group_offset; p.W_in = W_in; p.b = b; p.in_scale = in_scale; p.in_shift = in_shift; p.U = U;
    p.E = E; p.e_f32 = e_f32 ? 1 : 0;
    return hip_fail(launch_elm_features(p, (hipStream_t)stream), who);
}

int esn_elm_predict(int precision, int n_in, int n_hidden, int window, int bias_col, int n_wsets, int n_out,
                    const double* W_in, const double* b, const double* W_out, int e_cols, const double* in_scale,
                    const double* in_shift, const double* t_scale, const double* t_shift, const double* U, int n_frames,
                    int frames_per_group, int T_in, int T, int transient, uint64_t group_offset, double* Y, void* stream) {
    const char* who = "esn_elm_predict";
    if (!W_in || !b || !W_out || !U || !Y) return fail(-1, "%s: null pointer", who);
    if (int rc = n_out_check(who, n_out)) return rc;
    const int rc = elm_check(who, precision, n_in, n_hidden, window, bias_col, n_wsets, n_out, e_cols, n_frames,
                             frames_per_group, T_in, T, transient);
    if (rc) return rc;
    if ((uintptr_t)Y & 15) return fail(-1, "%s: Y must be 16-byte aligned", who);
    ElmParams p;
    memset(&p, 0, sizeof(p));
    p.n_in = n_in; p.n_hidden = n_hidden; p.window = window; p.bias_col = bias_col; p.n_wsets = n_wsets; p.n_out = n_out;
    p.e_cols = e_cols; p.n_seq = n_frames; p.seq_per_group = frames_per_group; p.T_in = T_in; p.T = T;
    p.transient = transient; p.group_offset = group_offset; p.W_in = W_in; p.b = b; p.W_out = W_out;
    p.in_scale = in_scale; p.in_shift = in_shift; p.t_scale = t_scale; p.t_shift = t_shift; p.U = U; p.Y = Y;
    return hip_fail(launch_elm_predict(precision, p, (hipStream_t)stream), who);
}

// ---- the Adam-trained comparators (FNN, CNN, LSTM): the checks their six entry points share

// the optimiser's arguments; n_isets = 1 where another check has already answered for it
static int adam_check(const char* who, int n_isets, int epochs, double lr, double beta1, double beta2, double eps) {
    if (n_isets < 1) return fail(-1, "%s: n_isets=%d must be positive", who, n_isets);
    if (epochs < 1) return fail(-1, "%s: epochs=%d must be positive", who, epochs);
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps > 0.0))
        return fail(-1, "%s: need lr >= 0, 0 <= beta1, beta2 < 1 and eps > 0", who);
    return 0;
}

// the workspace against what `query` (the name of the entry point that says it) answers for the call
static int workspace_check(const char* who, const char* query, const void* workspace, size_t workspace_bytes, size_t need) {
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7))
        return fail(-1, "%s: workspace of %zu bytes (8-byte aligned) needed, %s; got %zu", who, need, query,
                    workspace ? workspace_bytes : (size_t)0);
    return 0;
}

// what the train and predict entry points of the sequence models (CNN, LSTM) check alike.  shape: the call's sizes as
// the message gives them; why: the answer of the model's *_shape_limit; n_seq: groups or frames
static int sequence_check(const char* who, int precision, const char* shape, const char* why, int n_seq, int T_in, int T,
                          int transient) {
    if (precision != ESN_F64 && precision != ESN_F32 && precision != ESN_F16 && precision != ESN_BF16)
        return fail(-1, "%s: unknown precision %d", who, precision);
    if (why) return fail(-1, "%s: %s: %s", who, shape, why);
    if (n_seq < 1) return fail(-1, "%s: invalid sizes (groups, frames)", who);
    if (T_in < 1 || T_in > T) return fail(-1, "%s: need 1 <= T_in <= T (T_in=%d, T=%d)", who, T_in, T);
    if (transient < 0 || transient >= T) return fail(-1, "%s: transient=%d must be in [0, T) with T=%d", who, transient, T);
    if (precision != ESN_F64) return fail(-2, "%s: float64 (ESN_F64) only; precision %d is not built", who, precision);
    return 0;
}

struct ShapeText { char text[160]; };
static ShapeText cnn_shape_text(int n_in, int c1, int c2, int n_out, int kernel, int T) {
    ShapeText s;
    snprintf(s.text, sizeof(s.text), "n_in=%d c1=%d c2=%d n_out=%d kernel=%d T=%d", n_in, c1, c2, n_out, kernel, T);
    return s;
}
static ShapeText lstm_shape_text(int n_in, int n_hidden, int n_out, int T) {
    ShapeText s;
    snprintf(s.text, sizeof(s.text), "n_in=%d n_hidden=%d n_out=%d T=%d", n_in, n_hidden, n_out, T);
    return s;
}

size_t esn_fnn_workspace_bytes(int n_in, int n_hidden, int window, int n_out, int n_groups, int T) {
    (void)n_out; (void)T;
    if (n_in < 1 || n_hidden < 1 || window < 1 || n_groups < 1) return 0;
    return fnn_train_workspace_bytes(n_in, n_hidden, window, n_groups);      // Adam's moments of W1
}

int esn_fnn_train(int precision, int n_in, int n_hidden, int window, int n_out, int n_isets, const double* W1_0,
                  const double* b1_0, const double* W2_0, const double* b2_0, const double* in_scale,
                  const double* in_shift, const double* t_scale, const double* t_shift, const double* U, const double* D,
                  int n_groups, int T_in, int T, int transient, uint64_t group_offset, int epochs, double lr, double beta1,
                  double beta2, double eps, double* W1, double* b1, double* W2, double* b2, double* loss, void* workspace,
                  size_t workspace_bytes, void* stream) {
    const char* who = "esn_fnn_train";
    if (!W1_0 || !b1_0 || !W2_0 || !b2_0 || !U || !D || !W1 || !b1 || !W2 || !b2) return fail(-1, "%s: null pointer", who);
    if (int rc = n_out_check(who, n_out)) return rc;
    if (int rc = elm_check(who, precision == ESN_F16 ? ESN_F64 : precision, n_in, n_hidden, window, 1, n_isets, n_out,
                           n_hidden + 1, n_groups, 1, T_in, T, transient))
        return rc;
    if (precision != ESN_F64) return fail(-2, "%s: the training is float64 (ESN_F64); precision %d is not built", who, precision);
    const int K = window * n_in;
    if (n_hidden > 512 || n_out * n_hidden > 1024 || ((n_hidden + 3) / 4) * ((K + 7) / 8) > 512)
        return fail(-1, "%s: n_hidden=%d K=%d n_out=%d: served up to n_hidden <= 512, n_out n_hidden <= 1024 and "
                    "ceil(n_hidden / 4) ceil(K / 8) <= 512 (n_hidden K <= 16384)", who, n_hidden, K, n_out);
    const size_t lds = fnn_train_lds_bytes(n_in, n_hidden, window, n_out, T);
    if (lds > 160 * 1024)
        return fail(-1, "%s: n_hidden=%d K=%d T=%d n_out=%d needs more than the served %d bytes of LDS "
                    "(8 (n_hidden (K | 1) + T n_in + n_out n_hidden + n_hidden + n_out + 32 (n_hidden | 1) + 257))", who,
                    n_hidden, K, T, n_out, 160 * 1024);
    if (int rc = adam_check(who, 1, epochs, lr, beta1, beta2, eps)) return rc;      // (n_isets: elm_check's n_wsets)
    if (int rc = workspace_check(who, "esn_fnn_workspace_bytes", workspace, workspace_bytes,
                                 fnn_train_workspace_bytes(n_in, n_hidden, window, n_groups)))
        return rc;
    FnnTrainParams p;
    memset(&p, 0, sizeof(p));
    p.n_in = n_in; p.n_hidden = n_hidden; p.window = window; p.n_out = n_out; p.n_isets = n_isets; p.n_groups = n_groups;
    p.T_in = T_in; p.T = T; p.transient = transient; p.epochs = epochs; p.group_offset = group_offset;
    p.lr = lr; p.beta1 = beta1; p.beta2 = beta2; p.eps = eps;
    p.W1_0 = W1_0; p.b1_0 = b1_0; p.W2_0 = W2_0; p.b2_0 = b2_0;
    p.in_scale = in_scale; p.in_shift = in_shift; p.t_scale = t_scale; p.t_shift = t_shift; p.U = U; p.D = D;
    p.W1 = W1; p.b1 = b1; p.W2 = W2; p.b2 = b2; p.loss = loss;
    p.workspace = reinterpret_cast<double*>(workspace);
    return hip_fail(launch_fnn_train(p, (hipStream_t)stream), who);
}

int esn_fnn_predict(int precision, int n_in, int n_hidden, int window, int n_out, const double* W1, const double* b1,
                    const double* W2, const double* b2, const double* in_scale, const double* in_shift,
                    const double* t_scale, const double* t_shift, const double* U, int n_frames, int frames_per_group,
                    int T_in, int T, int transient, double* Y, void* stream) {
    const char* who = "esn_fnn_predict";
    if (!W1 || !b1 || !W2 || !b2 || !U || !Y) return fail(-1, "%s: null pointer", who);
    if (int rc = n_out_check(who, n_out)) return rc;
    if (int rc = elm_check(who, precision, n_in, n_hidden, window, 1, 1, n_out, n_hidden + 1, n_frames, frames_per_group,
                           T_in, T, transient))
        return rc;
    if ((uintptr_t)Y & 15) return fail(-1, "%s: Y must be 16-byte aligned", who);
    ElmParams p;
    memset(&p, 0, sizeof(p));
    // the ELM's parameter block: one weight set per group, the bias column's weights in b_out beside W_out = W2
    p.n_in = n_in; p.n_hidden = n_hidden; p.window = window; p.bias_col = 1; p.n_out = n_out; p.e_cols = n_hidden;
    p.n_wsets = (n_frames + frames_per_group - 1) / frames_per_group;
    p.n_seq = n_frames; p.seq_per_group = frames_per_group; p.T_in = T_in; p.T = T; p.transient = transient;
    p.group_offset = 0; p.W_in = W1; p.b = b1; p.W_out = W2; p.b_out = b2;
    p.in_scale = in_scale; p.in_shift = in_shift; p.t_scale = t_scale; p.t_shift = t_shift; p.U = U; p.Y = Y;
    return hip_fail(launch_fnn_predict(precision, p, (hipStream_t)stream), who);
}

size_t esn_cnn_workspace_bytes(int n_in, int c1, int c2, int n_out, int kernel, int n_groups, int n_frames, int T) {
    if (cnn_shape_limit(n_in, c1, c2, n_out, kernel, T) || n_groups < 0 || n_frames < 0) return 0;
    return cnn_workspace_bytes(n_in, c1, c2, n_out, kernel, n_groups, n_frames, T);
}

int esn_cnn_train(int precision, int n_in, int c1, int c2, int n_out, int kernel, int n_isets, const double* W1_0,
                  const double* b1_0, const double* W2_0, const double* b2_0, const double* W3_0, const double* b3_0,
                  const double* in_scale, const double* in_shift, const double* t_scale, const double* t_shift,
                  const double* U, const double* D, int n_groups, int T_in, int T, int transient, uint64_t group_offset,
                  int epochs, double lr, double beta1, double beta2, double eps, double* W1, double* b1, double* W2,
                  double* b2, double* W3, double* b3, double* loss, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "esn_cnn_train";
    if (!W1_0 || !b1_0 || !W2_0 || !b2_0 || !W3_0 || !b3_0 || !U || !D || !W1 || !b1 || !W2 || !b2 || !W3 || !b3)
        return fail(-1, "%s: null pointer", who);
    if (int rc = adam_check(who, n_isets, epochs, lr, beta1, beta2, eps)) return rc;
    if (int rc = sequence_check(who, precision, cnn_shape_text(n_in, c1, c2, n_out, kernel, T).text,
                                cnn_shape_limit(n_in, c1, c2, n_out, kernel, T), n_groups, T_in, T, transient))
        return rc;
    if (int rc = workspace_check(who, "esn_cnn_workspace_bytes", workspace, workspace_bytes,
                                 cnn_workspace_bytes(n_in, c1, c2, n_out, kernel, n_groups, 0, T)))
        return rc;
    CnnParams p;
    sequence_params(p, T_in, T, transient, {W1_0, W2_0, W3_0}, {b1_0, b2_0, b3_0}, in_scale, in_shift, t_scale, t_shift, U,
                    workspace);
    training_params(p, n_isets, n_groups, group_offset, epochs, lr, beta1, beta2, eps, D, {W1, W2, W3}, {b1, b2, b3}, loss);
    p.n_in = n_in; p.c1 = c1; p.c2 = c2; p.n_out = n_out; p.kernel = kernel;
    return hip_fail(launch_cnn_train(p, (hipStream_t)stream), who);
}

int esn_cnn_predict(int precision, int n_in, int c1, int c2, int n_out, int kernel, const double* W1, const double* b1,
                    const double* W2, const double* b2, const double* W3, const double* b3, const double* in_scale,
                    const double* in_shift, const double* t_scale, const double* t_shift, const double* U, int n_frames,
                    int frames_per_group, int T_in, int T, int transient, double* Y, void* workspace,
                    size_t workspace_bytes, void* stream) {
    const char* who = "esn_cnn_predict";
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !U || !Y) return fail(-1, "%s: null pointer", who);
    if (frames_per_group < 1) return fail(-1, "%s: frames_per_group=%d must be positive", who, frames_per_group);
    if (int rc = sequence_check(who, precision, cnn_shape_text(n_in, c1, c2, n_out, kernel, T).text,
                                cnn_shape_limit(n_in, c1, c2, n_out, kernel, T), n_frames, T_in, T, transient))
        return rc;
    if (int rc = workspace_check(who, "esn_cnn_workspace_bytes", workspace, workspace_bytes,
                                 cnn_workspace_bytes(n_in, c1, c2, n_out, kernel, 0, n_frames, T)))
        return rc;
    CnnParams p;
    sequence_params(p, T_in, T, transient, {W1, W2, W3}, {b1, b2, b3}, in_scale, in_shift, t_scale, t_shift, U, workspace);
    p.n_in = n_in; p.c1 = c1; p.c2 = c2; p.n_out = n_out; p.kernel = kernel;
    p.n_frames = n_frames; p.frames_per_group = frames_per_group; p.Y = Y;
    return hip_fail(launch_cnn_predict(p, (hipStream_t)stream), who);
}

size_t esn_lstm_workspace_bytes(int n_in, int n_hidden, int n_out, int n_groups, int n_frames, int T) {
    if (lstm_shape_limit(n_in, n_hidden, n_out, T) || n_groups < 0 || n_frames < 0) return 0;
    return lstm_workspace_bytes(n_in, n_hidden, n_out, n_groups, n_frames, T);
}

int esn_lstm_train(int precision, int n_in, int n_hidden, int n_out, int n_isets, const double* W_ih_0,
                   const double* W_hh_0, const double* b_ih_0, const double* b_hh_0, const double* W_fc_0,
                   const double* b_fc_0, const double* in_scale, const double* in_shift, const double* t_scale,
                   const double* t_shift, const double* U, const double* D, int n_groups, int T_in, int T, int transient,
                   uint64_t group_offset, int epochs, double lr, double beta1, double beta2, double eps, double* W_ih,
                   double* W_hh, double* b_ih, double* b_hh, double* W_fc, double* b_fc, double* loss, void* workspace,
                   size_t workspace_bytes, void* stream) {
    const char* who = "esn_lstm_train";
    if (!W_ih_0 || !W_hh_0 || !b_ih_0 || !b_hh_0 || !W_fc_0 || !b_fc_0 || !U || !D || !W_ih || !W_hh || !b_ih || !b_hh ||
        !W_fc || !b_fc)
        return fail(-1, "%s: null pointer", who);
    if (int rc = adam_check(who, n_isets, epochs, lr, beta1, beta2, eps)) return rc;
    if (int rc = sequence_check(who, precision, lstm_shape_text(n_in, n_hidden, n_out, T).text,
                                lstm_shape_limit(n_in, n_hidden, n_out, T), n_groups, T_in, T, transient))
        return rc;
    if (int rc = workspace_check(who, "esn_lstm_workspace_bytes", workspace, workspace_bytes,
                                 lstm_workspace_bytes(n_in, n_hidden, n_out, n_groups, 0, T)))
        return rc;
    LstmParams p;
    sequence_params(p, T_in, T, transient, {W_ih_0, W_hh_0, W_fc_0}, {b_ih_0, b_hh_0, b_fc_0}, in_scale, in_shift, t_scale,
                    t_shift, U, workspace);
    training_params(p, n_isets, n_groups, group_offset, epochs, lr, beta1, beta2, eps, D, {W_ih, W_hh, W_fc},
                    {b_ih, b_hh, b_fc}, loss);
    p.n_in = n_in; p.n_hidden = n_hidden; p.n_out = n_out;
    return hip_fail(launch_lstm_train(p, (hipStream_t)stream), who);
}

int esn_lstm_predict(int precision, int n_in, int n_hidden, int n_out, const double* W_ih, const double* W_hh,
                     const double* b_ih, const double* b_hh, const double* W_fc, const double* b_fc,
                     const double* in_scale, const double* in_shift, const double* t_scale, const double* t_shift,
                     const double* U, int n_frames, int frames_per_group, int T_in, int T, int transient, double* Y,
                     void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "esn_lstm_predict";
    if (!W_ih || !W_hh || !b_ih || !b_hh || !W_fc || !b_fc || !U || !Y) return fail(-1, "%s: null pointer", who);
    if (frames_per_group < 1) return fail(-1, "%s: frames_per_group=%d must be positive", who, frames_per_group);
    if (int rc = sequence_check(who, precision, lstm_shape_text(n_in, n_hidden, n_out, T).text,
                                lstm_shape_limit(n_in, n_hidden, n_out, T), n_frames, T_in, T, transient))
        return rc;
    if (int rc = workspace_check(who, "esn_lstm_workspace_bytes", workspace, workspace_bytes,
                                 lstm_workspace_bytes(n_in, n_hidden, n_out, 0, n_frames, T)))
        return rc;
    LstmParams p;
    sequence_params(p, T_in, T, transient, {W_ih, W_hh, W_fc}, {b_ih, b_hh, b_fc}, in_scale, in_shift, t_scale, t_shift, U,
                    workspace);
    p.n_in = n_in; p.n_hidden = n_hidden; p.n_out = n_out;
    p.n_frames = n_frames; p.frames_per_group = frames_per_group; p.Y = Y;
    return hip_fail(launch_lstm_predict(p, (hipStream_t)stream), who);
}

int esn_taps_to_freq(int n_blocks, int n_sub, int n_t, int n_r, int isi, const double* taps, double* H, void* stream) {
    if (!taps || !H) return fail(-1, "esn_taps_to_freq: null pointer");
    if (n_blocks <= 0 || n_sub <= 0 || n_t <= 0 || n_r <= 0 || isi <= 0 || isi > n_sub)
        return fail(-1, "esn_taps_to_freq: invalid sizes");
    TapsFreqParams tp;
    tp.n_blocks = n_blocks; tp.n_sub = n_sub; tp.n_t = n_t; tp.n_r = n_r; tp.isi = isi; tp.taps = taps; tp.H = H;
    return hip_fail(launch_taps_to_freq(tp, (hipStream_t)stream), "esn_taps_to_freq");
}

int esn_channel_metrics(int n_blocks, int n_sub, int n_t, int n_r, const double* H, const double* p_i, double no,
                        double* S, double* cond, uint8_t* rank, double* cap, void* stream) {
    if (!H || !p_i || !cond || !rank || !cap) return fail(-1, "esn_channel_metrics: null pointer");
    if (n_blocks <= 0 || n_sub <= 0 || n_t <= 0 || n_r <= 0) return fail(-1, "esn_channel_metrics: invalid sizes");
    if (!((n_t <= 4 && n_r <= 8) || (n_r <= 4 && n_t <= 8)))
        return fail(-1, "esn_channel_metrics: unsupported n_t=%d n_r=%d (needs min <= 4 and max <= 8)", n_t, n_r);
    if ((uintptr_t)H & 15) return fail(-1, "esn_channel_metrics: H must be 16-byte aligned");
    ChanStatParams c;
    c.n_blocks = n_blocks; c.n_sub = n_sub; c.n_t = n_t; c.n_r = n_r; c.H = H; c.p_i = p_i; c.no = no;
    c.S = S; c.cond = cond; c.rank = rank; c.cap = cap;
    return hip_fail(launch_channel_metrics(c, (hipStream_t)stream), "esn_channel_metrics");
}

int esn_ldpc_encode(int n_frames, int n_t, int k, int n, const uint8_t* P, const uint8_t* u, uint8_t* bits,
                    void* stream) {
    if (!P || !u || !bits) return fail(-1, "esn_ldpc_encode: null pointer");
    if (n_frames <= 0 || n_t <= 0 || k <= 0 || k >= n || k > 60000) return fail(-1, "esn_ldpc_encode: invalid sizes");
    LdpcEncodeParams ep;
    ep.n_frames = n_frames; ep.n_t = n_t; ep.k = k; ep.n = n; ep.P = P; ep.u = u; ep.bits = bits;
    return hip_fail(launch_ldpc_encode(ep, (hipStream_t)stream), "esn_ldpc_encode");
}

int esn_qam_llr(int n_frames, int n_sub, int n_t, int bits_per_sym, const double* X_hat, double* llr,
                double* sigma2, void* stream) {
    if (!X_hat || !llr) return fail(-1, "esn_qam_llr: null pointer");
    if (n_frames <= 0 || n_sub <= 0 || n_t <= 0 || bits_per_sym < 2 || bits_per_sym > 10 || (bits_per_sym & 1))
        return fail(-1, "esn_qam_llr: invalid sizes");
    LlrParams lp;
    lp.n_frames = n_frames; lp.n_sub = n_sub; lp.n_t = n_t; lp.m = bits_per_sym; lp.X_hat = X_hat; lp.llr = llr;
    lp.sigma2 = sigma2;
    return hip_fail(launch_qam_llr(lp, (hipStream_t)stream), "esn_qam_llr");
}

// ---- SINR-weighted soft outputs (esn_soft.hip): every refusal below comes before any HIP call
static int check_soft_shape(const char* who, int n_sub, int n_t, int* log2n) {
    if (int rc = check_n_sub(who, n_sub, log2n)) return rc;
    if (n_t < 1 || n_t > 4) return fail(-1, "%s: n_t=%d, 1 to 4 are served", who, n_t);
    return 0;
}
static int check_soft_frames(const char* who, int n_frames, int frames_per_group, int bits_per_sym) {
    if (n_frames <= 0) return fail(-1, "%s: n_frames=%d must be positive", who, n_frames);
    if (frames_per_group <= 0) return fail(-1, "%s: frames_per_group=%d must be positive", who, frames_per_group);
    return check_square_qam(who, bits_per_sym);
}

int esn_mmse_sinr(int n_blocks, int n_sub, int n_t, int n_r, const double* p_i, double no, const double* H, double* w,
                  double* mu, double* gamma_mean, void* stream) {
    const char* who = "esn_mmse_sinr";
    int l2;
    if (int rc = check_soft_shape(who, n_sub, n_t, &l2)) return rc;
    if (n_blocks <= 0 || n_r <= 0) return fail(-1, "%s: n_blocks=%d and n_r=%d must be positive", who, n_blocks, n_r);
    if (!p_i || !H) return fail(-1, "%s: p_i or H is null", who);
    if (!w || !mu) return fail(-1, "%s: w or mu is null", who);
    SinrParams sp;
    sp.n_blocks = n_blocks; sp.n_sub = n_sub; sp.n_t = n_t; sp.n_r = n_r; sp.p_i = p_i; sp.no = no; sp.H = H;
    sp.w = w; sp.mu = mu; sp.gamma_mean = gamma_mean;
    return hip_fail(launch_mmse_sinr(sp, (hipStream_t)stream), who);
}

int esn_qam_llr_weighted(int n_frames, int frames_per_group, int n_sub, int n_t, int bits_per_sym, const double* X_hat,
                         const double* w, const double* mu, double* llr, double* sigma2, void* stream) {
    const char* who = "esn_qam_llr_weighted";
    int l2;
    if (int rc = check_soft_shape(who, n_sub, n_t, &l2)) return rc;
    if (int rc = check_soft_frames(who, n_frames, frames_per_group, bits_per_sym)) return rc;
    if (!X_hat) return fail(-1, "%s: X_hat is null", who);
    if (!llr) return fail(-1, "%s: llr is null", who);
    SoftLlrParams sp;
    sp.l.n_frames = n_frames; sp.l.n_sub = n_sub; sp.l.n_t = n_t; sp.l.m = bits_per_sym; sp.l.X_hat = X_hat;
    sp.l.llr = llr; sp.l.sigma2 = sigma2; sp.frames_per_group = frames_per_group; sp.w = w; sp.mu = mu;
    return hip_fail(launch_qam_llr_weighted(sp, (hipStream_t)stream), who);
}

size_t esn_detect_llr_lds_bytes(int n_sub, int n_t) {
    return (n_sub > 0 && n_t > 0) ? detect_llr_lds_bytes(n_sub, n_t) : 0;
}

static int detect_llr_common(const char* who, bool io32, const void* Y, int n_frames, int frames_per_group, int n_sub,
                             int n_t, int bits_per_sym, const double* p_i, const uint8_t* tx_bits, long long* err_count,
                             long long* bit_count, const double* w, const double* mu, double* llr, double* sigma2,
                             double* X_hat, void* stream) {
    int l2;
    if (int rc = check_soft_shape(who, n_sub, n_t, &l2)) return rc;
    if (int rc = check_soft_frames(who, n_frames, frames_per_group, bits_per_sym)) return rc;
    if (!Y || !p_i) return fail(-1, "%s: Y or p_i is null", who);
    if (!llr) return fail(-1, "%s: llr is null", who);
    if (tx_bits && (!err_count || !bit_count)) return fail(-1, "%s: tx_bits given without err_count / bit_count", who);
    if (((uintptr_t)Y & (io32 ? 7 : 15)) != 0) return fail(-1, "%s: Y must be %d-byte aligned", who, io32 ? 8 : 16);
    if (X_hat && ((uintptr_t)X_hat & 15) != 0) return fail(-1, "%s: X_hat must be 16-byte aligned", who);
    DetectLlrParams lp;
    DetectParams& dp = lp.d;
    if (io32) dp.Y32 = static_cast<const float*>(Y); else dp.Y = static_cast<const double*>(Y);
    dp.n_frames = n_frames; dp.frames_per_group = frames_per_group; dp.n_sub = n_sub; dp.log2n = l2; dp.n_t = n_t;
    dp.m = bits_per_sym; dp.p_i = p_i; dp.tx_bits = tx_bits; dp.err = err_count; dp.bits = bit_count; dp.X_hat = X_hat;
    dp.na_wg = n_t;
    lp.w = w; lp.mu = mu; lp.llr = llr; lp.sigma2 = sigma2;
    const int e = launch_detect_llr(lp, (hipStream_t)stream, io32);
    if (e == -1)                                             // the launcher's check; no served shape reaches it
        return fail(-2, "%s: N=%d n_t=%d needs 16 (n_t (N + 1) + N/2) = %zu bytes of LDS, %zu are served: use "
                    "esn_detect_count with X_hat and esn_qam_llr_weighted", who, n_sub, n_t,
                    detect_llr_lds_bytes(n_sub, n_t), MMSE_LDS_MAX);
    return hip_fail(e, who);
}

int esn_detect_llr(const double* Y, int n_frames, int frames_per_group, int n_sub, int n_t, int bits_per_sym,
                   const double* p_i, const uint8_t* tx_bits, long long* err_count, long long* bit_count,
                   const double* w, const double* mu, double* llr, double* sigma2, double* X_hat, void* stream) {
    return detect_llr_common("esn_detect_llr", false, Y, n_frames, frames_per_group, n_sub, n_t, bits_per_sym, p_i,
                             tx_bits, err_count, bit_count, w, mu, llr, sigma2, X_hat, stream);
}

int esn_detect_llr_f32(const float* Y, int n_frames, int frames_per_group, int n_sub, int n_t, int bits_per_sym,
                       const double* p_i, const uint8_t* tx_bits, long long* err_count, long long* bit_count,
                       const double* w, const double* mu, double* llr, double* sigma2, double* X_hat, void* stream) {
    return detect_llr_common("esn_detect_llr_f32", true, Y, n_frames, frames_per_group, n_sub, n_t, bits_per_sym, p_i,
                             tx_bits, err_count, bit_count, w, mu, llr, sigma2, X_hat, stream);
}

int esn_ldpc_decode_count(int n_cw, int n, int k, int m_checks, int n_edges, const int* chk_ptr, const int* edge_var,
                          const int* var_ptr, const int* var_edge, const double* y, double snr_db, int maxiter,
                          const uint8_t* u_true, int cw_per_group, uint8_t* x_out, long long* err_count,
                          long long* bit_count, void* stream) {
    if (!chk_ptr || !edge_var || !var_ptr || !var_edge || !y) return fail(-1, "esn_ldpc_decode_count: null pointer");
    if (u_true && (!err_count || !bit_count)) return fail(-1, "esn_ldpc_decode_count: counters missing");
    if (n_cw <= 0 || n <= 0 || k <= 0 || k > n || m_checks <= 0 || n_edges <= 0 || maxiter <= 0 || cw_per_group <= 0)
        return fail(-1, "esn_ldpc_decode_count: invalid sizes");
    LdpcDecodeParams dp;
    dp.n_cw = n_cw; dp.n = n; dp.k = k; dp.m_checks = m_checks; dp.n_edges = n_edges; dp.maxiter = maxiter;
    dp.cw_per_group = cw_per_group; dp.var = pow(10.0, -snr_db / 10.0);
    dp.chk_ptr = chk_ptr; dp.edge_var = edge_var; dp.var_ptr = var_ptr; dp.var_edge = var_edge; dp.y = y;
    dp.u_true = u_true; dp.x_out = x_out; dp.err = err_count; dp.bits = bit_count;
    int e = launch_ldpc_decode(dp, (hipStream_t)stream);
    if (e == -1) return fail(-2, "esn_ldpc_decode_count: graph does not fit LDS (16 B per edge)");
    return hip_fail(e, "esn_ldpc_decode_count");
}

}  // extern "C"
