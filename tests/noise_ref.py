"""The counter state-noise stream of csrc/esn_common.h restated in numpy, and the table of cases that
tests/test_noise_reference_cpu.py (no GPU) and tests/test_gpu_noise_parity.py (MI355X) share.

The stream (all arithmetic modulo 2^32; carried here in uint64 and masked):

    mix32(x):        x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
    noise_key(seed, frame, step)
                   = mix32(mix32(lo32(seed) ^ frame * 0x9E3779B9) ^ hi32(seed) ^ (step * 0x85EBCA6B + 0x27d4eb2f))
    noise_mix(s):    s ^= s >> 16;  s = (s & 0xffffff) * 0x9E3779  (__umul24, low 32 bits);  s ^= s >> 16
    noise_quad(k, row4)    = noise_mix(k + row4 * 0x9E3779B9)
    noise_uniform(k, row)  = (byte (row & 3) of noise_quad(k, row >> 2) + 0.5) / 256

Conventions of the kernels (read from csrc/esn_recur_f64.hip and the two entry points of csrc/esn_api.hip):

    predict   step s in [0, T) produces x_{s+1}, the state behind output row s; the frame index of frame b of the
              call is  group_offset * F + b  (mod 2^32), F = frames per group;
    harvest   step s in [0, T - 1) produces row s + 1 of E (row 0 is never fed and stays zero); the frame index of
              pilot g of the call is  group_offset + g  (mod 2^32);
    the single-sequence float64 cluster kernel draws for frame  frame_off + 0, i.e. the same rule with b = g = 0.

Every state adds  noise * (uniform - 0.5).  In `tensor` mode the caller hands the uniforms in: predict reads
noise_u[b, s, row] (shape [B, T, n_res]), harvest noise_u[g, s, row] (shape [G, T - 1, n_res]); counter_uniforms
returns the counter stream in exactly that layout.

ReplayRng hands rows of such an array to oracle.esn_oracle.OracleESN through its replaceable `.rng`, one row per
state update, so the float64 oracle runs with the very draws a kernel used.
"""
import collections
import functools

import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def _u(x):
    return np.asarray(x, dtype=np.uint64) & M32


def mix32(x):
    x = _u(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> np.uint64(16))


def noise_key(seed, frame, step):
    seed = int(seed) & (2 ** 64 - 1)
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    k = mix32(lo ^ ((_u(frame) * np.uint64(0x9E3779B9)) & M32))
    return mix32(k ^ hi ^ ((_u(step) * np.uint64(0x85EBCA6B) + np.uint64(0x27d4eb2f)) & M32))


def noise_mix(s):
    s = _u(s)
    s = s ^ (s >> np.uint64(16))
    s = ((s & np.uint64(0xFFFFFF)) * np.uint64(0x9E3779)) & M32
    return s ^ (s >> np.uint64(16))


def noise_quad(k, row4):
    return noise_mix((_u(k) + _u(row4) * np.uint64(0x9E3779B9)) & M32)


def noise_byte(k, row):
    row = _u(row)
    return (noise_quad(k, row >> np.uint64(2)) >> (np.uint64(8) * (row & np.uint64(3)))) & np.uint64(0xFF)


def noise_uniform(k, row):
    return (noise_byte(k, row).astype(np.float64) + 0.5) / 256.0


def counter_bytes(seed, first_frame, n_frames, n_steps, n_res):
    """uint8 [n_frames, n_steps, n_res]: the byte behind every uniform; frame indices are taken mod 2^32."""
    frames = (int(first_frame) + np.arange(n_frames, dtype=np.uint64)) & M32
    keys = noise_key(seed, frames[:, None], np.arange(n_steps, dtype=np.uint64)[None, :])
    return noise_byte(keys[:, :, None], np.arange(n_res, dtype=np.uint64)[None, None, :]).astype(np.uint8)


def counter_uniforms(seed, first_frame, n_frames, n_steps, n_res):
    """float64 [n_frames, n_steps, n_res] in (0, 1): what counter mode draws for frames first_frame ... (mod 2^32)."""
    return (counter_bytes(seed, first_frame, n_frames, n_steps, n_res).astype(np.float64) + 0.5) / 256.0


class ReplayRng:
    """Stands in for the RandomState of OracleESN: .rand(n) hands out the rows of u2d [n_updates, n], in order."""

    def __init__(self, u2d):
        self.u = np.asarray(u2d, dtype=np.float64)
        self.i = 0

    def rand(self, n):
        row = self.u[self.i]
        assert row.shape == (n,), (row.shape, n)
        self.i += 1
        return row.copy()


# ---------------------------------------------------------------------------------------------------------------
# The shared table.  One row = one launch shape on one kernel.
#   kind      "predict" | "harvest"
#   groups    predict: groups of F frames, the last one holding `last` (< F: ragged, so padding slots exist);
#             harvest: pilots (F = last = 1)
#   knobs     esn_debug_set keys moved for the launch (back to their defaults afterwards)
#   path      what _lib.recur_path must answer for the launch (asserted on the CPU and again at the launch)
#   tol       tensor mode against the oracle, relative to max |expected| -- the bound of the project's noise-free test
#             of the same path (tests/test_gpu_parity.py, test_gpu_big.py, test_gpu_harvest_cluster.py): f64 1e-10,
#             f32 2e-5, f16 2e-2, bf16 harvest states 3e-2.  None: not compared with the oracle (bf16 predict: its
#             1e-1 .. 2e-1 bound cannot see a wrong stream through a dense read-out; counter-equals-tensor carries it)
#   noise     amplitude: an input, chosen so that every wrong stream moves the compared quantity by >= 2 tol
#   readback  also run the zero-weight, noise = 1 harvest whose states ARE the stream
# ---------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "id kind precision n_res n_in n_out groups F last knobs path tol noise readback")
T_STEPS, TRANSIENT = 12, 2
SEED = (7 << 32) + 12345                 # above 2^32: the high half of the seed enters the key
GROUP_OFFSET = 5
TOL = {"f64": 1e-10, "f32": 2e-5, "f16": 2e-2, "bf16": 3e-2}


def _p(id, prec, n_res, groups, F, last, path, knobs=None, tol="prec", noise=None, n_in=16, n_out=8):
    # fp16 outputs are compared at 2e-2 through a dense read-out of up to 1100 states: at noise 0.1 an exchange of 32
    # rows moves them by 1e-2 .. 3e-2 only (measured on the oracle), at 0.5 by 4e-2 .. 17e-2
    noise = (0.5 if prec in ("f16", "bf16") else 0.1) if noise is None else noise
    return Case(id, "predict", prec, n_res, n_in, n_out, groups, F, last, knobs or {}, path,
                TOL[prec] if tol == "prec" else tol, noise, False)


def _h(id, prec, n_res, groups, path, knobs=None, noise=0.1, readback=False, n_in=16, n_out=8):
    return Case(id, "harvest", prec, n_res, n_in, n_out, groups, 1, 1, knobs or {}, path, TOL[prec], noise, readback)


# Batches are sized so that the slot axis spans more than one workgroup tile wherever the path allows it (a predict
# group of 3 frames takes 16 slots on the matrix-pipe kernels; tiles hold 32 .. 256 slots), because the frame index of
# a slot in the second tile is where a wrong slot -> frame map would show.
CASES = [
    # float64: vector ALU (odd n_res: the lone last row of a thread's pair), matrix pipe, single-sequence cluster
    _p("p-f64-valu-71", "f64", 71, 3, 3, 2, "f64_valu"),
    _h("h-f64-valu-71", "f64", 71, 5, "f64_valu", readback=True),
    _p("p-f64-valu-71-tiles", "f64", 71, 4, 3, 2, "f64_valu", {"f64_mfma": "0"}),
    _h("h-f64-valu-71-tiles", "f64", 71, 11, "f64_valu", {"f64_mfma": "0"}, readback=True),
    _p("p-f64-mfma-71", "f64", 71, 5, 3, 2, "f64_mfma"),
    _h("h-f64-mfma-71", "f64", 71, 67, "f64_mfma", readback=True),
    _p("p-f64-cluster-71", "f64", 71, 1, 1, 1, "cluster_f64"),
    _h("h-f64-cluster-71", "f64", 71, 1, "cluster_f64", readback=True),
    # float32 on the matrix pipe
    _p("p-f32-48", "f32", 48, 5, 3, 2, "mfma"),
    _h("h-f32-48", "f32", 48, 67, "mfma", readback=True),
    _p("p-f32-300", "f32", 300, 5, 3, 2, "mfma"),
    _h("h-f32-300", "f32", 300, 67, "mfma", readback=True),
    _p("p-f32-600", "f32", 600, 3, 3, 2, "mfma"),
    _h("h-f32-600", "f32", 600, 35, "mfma", readback=True),
    # fp16: the persistent kernel in its tilings and schedules
    _p("p-f16-100", "f16", 100, 5, 3, 2, "mfma"),
    _h("h-f16-100", "f16", 100, 67, "mfma"),
    _p("p-f16-1024-skew", "f16", 1024, 5, 3, 2, "mfma"),
    _p("p-f16-1024-instep", "f16", 1024, 5, 3, 2, "mfma", {"skew": "0"}),
    _h("h-f16-1024", "f16", 1024, 67, "mfma"),
    _p("p-f16-1100-persistent", "f16", 1100, 3, 3, 2, "mfma", {"big_gemm": "0"}),
    _h("h-f16-1100-persistent", "f16", 1100, 35, "mfma", {"big_gemm": "0"}),
    # bf16
    _p("p-bf16-100", "bf16", 100, 5, 3, 2, "mfma", tol=None),
    _h("h-bf16-100", "bf16", 100, 67, "mfma"),
    # fp16 at 257..512 units: the 16x16x32 skewed kernel; s16 = 0: the 32x32x16 skewed kernel
    _p("p-f16-300-skew16", "f16", 300, 9, 3, 2, "skew16"),
    _p("p-f16-512-skew16", "f16", 512, 9, 3, 2, "skew16"),
    _p("p-f16-512-skew32", "f16", 512, 9, 3, 2, "mfma", {"s16": "0"}),
    # beyond 1024 units: one GEMM launch per step
    _p("p-f16-1100-big", "f16", 1100, 17, 3, 2, "big_predict"),
    _h("h-f16-1100-big", "f16", 1100, 67, "big_harvest"),
    # fp16 harvest at 257..512 units: clusters of two workgroups; 17 pilots leave a partial cluster
    _h("h-f16-512-hcluster17", "f16", 512, 17, "harvest_cluster"),
    _h("h-f16-300-hcluster17", "f16", 300, 17, "harvest_cluster"),
    _h("h-f16-512-hcluster1", "f16", 512, 1, "harvest_cluster"),
    _h("h-f16-300-persistent", "f16", 300, 67, "mfma", {"hcluster": "0"}),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def n_seq(c):
    """sequences of the launch: frames (predict) or pilots (harvest)"""
    return (c.groups - 1) * c.F + c.last


def n_steps(c):
    return T_STEPS if c.kind == "predict" else T_STEPS - 1


def first_frame(c, group_offset=GROUP_OFFSET):
    return (group_offset * c.F) & 0xFFFFFFFF


def frames_compared(c):
    """Sequences compared with the oracle: first, last of a group, first of the next, last (ragged) frame of a predict;
    first, middle and last pilot of a harvest."""
    n = n_seq(c)
    pick = [0, c.F - 1, c.F, n - 1] if c.kind == "predict" else [0, n // 2, n - 1]
    return sorted({min(max(i, 0), n - 1) for i in pick})


def sparse_gaussian(rs, n_res, density=0.1):
    """W without an eigenvalue pass: Gaussian entries on a `density` mask, scaled by 0.9 / sqrt(density n_res)."""
    w = rs.randn(n_res, n_res) * (rs.rand(n_res, n_res) < density)
    return w * (0.9 / np.sqrt(density * n_res))


@functools.lru_cache(maxsize=None)
def weights(n_res, n_in, n_out):
    rs = np.random.RandomState(1000 + n_res)
    return sparse_gaussian(rs, n_res), rs.rand(n_res, n_in) * 2 - 1, rs.rand(n_res, n_out) * 2 - 1


@functools.lru_cache(maxsize=None)
def case_data(case_id):
    """Everything a launch of the case reads (treat as read-only): per-group scalings, read-outs, inputs, teacher,
    initial state / feedback and the RandomState uniforms nz of tensor mode (one frame more than the launch has, so
    that "the next frame's draws" exist for the last one: the launch reads nz[:n])."""
    c = BY_ID[case_id]
    rs = np.random.RandomState(sum(map(ord, case_id)))
    w, w_in, w_fb = weights(c.n_res, c.n_in, c.n_out)
    G, n = c.groups, n_seq(c)
    d = dict(W=w, W_in=w_in, W_fb=w_fb,
             in_scale=rs.rand(G, c.n_in) * 0.2 + 0.1, in_shift=rs.randn(G, c.n_in) * 0.05,
             t_scale=rs.rand(G, c.n_out) + 0.5, t_shift=rs.randn(G, c.n_out) * 0.1,
             u=rs.randn(n, T_STEPS, c.n_in), nz=rs.rand(n + 1, n_steps(c), c.n_res))
    if c.kind == "predict":
        d.update(W_out=rs.randn(G, c.n_out, c.n_res + c.n_in) * 0.004,
                 x0=rs.randn(G, c.n_res) * 0.1, y0=rs.randn(G, c.n_out) * 0.1)
    else:
        d.update(d=rs.randn(n, T_STEPS, c.n_out) * 0.3)
    return d


def oracle_run(c, data, i, draws):
    """Sequence i of the case through the float64 oracle with the uniforms `draws` [n_steps, n_res]: the outputs
    [T - transient, n_out] of a predict, the states [T, n_res] of a harvest."""
    from oracle import esn_oracle as eo
    grp = i // c.F
    o = eo.OracleESN(c.n_in, c.n_out, c.n_res, noise=c.noise, input_scaling=data["in_scale"][grp],
                     input_shift=data["in_shift"][grp], teacher_scaling=data["t_scale"][grp],
                     teacher_shift=data["t_shift"][grp], weights=(data["W"], data["W_in"], data["W_fb"]))
    o.rng = ReplayRng(draws)
    if c.kind == "predict":
        o.W_out = data["W_out"][grp]
        o.laststate, o.lastoutput = data["x0"][grp], data["y0"][grp]
        return o.predict(data["u"][i], TRANSIENT, continuation=True)
    o.fit(data["u"][i], data["d"][i], 0)
    return o._ext_states[:, :c.n_res]


def exchange_rows(draws, a, b, n):
    """draws [..., n_res] with rows a .. a+n-1 and b .. b+n-1 exchanged (clipped to n_res)"""
    n = min(n, draws.shape[-1] - b)
    out = draws.copy()
    out[..., a:a + n], out[..., b:b + n] = draws[..., b:b + n], draws[..., a:a + n]
    return out


def wrong_streams(nz, i):
    """The four wrong streams of sequence i of the uniforms nz [n + 1, n_steps, n_res]: the errors the suite must see."""
    right = nz[i]
    return {"step+1": np.roll(right, -1, axis=0),
            "frame+1": nz[i + 1],
            "rows 0..31 <-> 32..63": exchange_rows(right, 0, 32, 32),
            "no noise": np.full_like(right, 0.5)}


def rel_err(got, want):
    return float(np.max(np.abs(got - want)) / (np.max(np.abs(want)) + 1e-300))


# Counter mode against tensor mode fed counter_uniforms, same kernel and launch: bitwise on the float64 paths; on the
# others the two modes round the addition differently.  Largest relative difference measured on the MI355X per
# precision, times two (tests/test_gpu_noise_parity.py holds the table of measurements); 0 = bitwise.
# Measured: f32 4.4e-7 (h-f32-600), f16 9.5e-4 (p-f16-512-skew16: one fp16 ulp of a state above 1), bf16 0 on both cases.
COUNTER_VS_TENSOR = {"f64": 0.0, "f32": 8.9e-7, "f16": 1.91e-3, "bf16": 0.0}
