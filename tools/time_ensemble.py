#!/usr/bin/env python3
"""What the ensemble tail costs (csrc/esn_ensemble.hip) and what an ensemble costs beside the single ESN it replaces, at
the benchmark's 153 600 frames (N = 128, n_t = 4, 16-QAM, groups of 75) unless told otherwise:

  (a) esn_detect_count_ens[_f32] at K = 2 / 4 / 8, float32 and float64 Y (and with member_err at K = 4);
  (b) the unfused path it replaces: Y.mean(0) -- or torch.einsum with a [G, K] weight table -- then esn_detect_count[_f32];
  (c) a device copy of the K slabs;
  (d) K predict launches at N_res = 256 in fp16 beside one at N_res = 512 (equal recurrence FLOPs), and the K fits
      (harvest fp16 + ridge solve) beside one.

Device events around the calls on preallocated inputs, 3 warm-ups, median of 9, the candidates of a section interleaved
in one process.  The judged figure: fused / unfused at K = 4 with float32 Y must not exceed 1.  --out FILE also writes
the table there (profiles/ensemble_time.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from esn_ofdm_mimo_amd import _lib  # noqa: E402
from esn_ofdm_mimo_amd.batched import ReservoirBank  # noqa: E402
from esn_ofdm_mimo_amd.ensemble import EnsembleBank  # noqa: E402
from esn_ofdm_mimo_amd.sweep import draw_reservoir  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=153600)
ap.add_argument("--per-group", type=int, default=75)
ap.add_argument("--n-sub", type=int, default=128)
ap.add_argument("--n-t", type=int, default=4)
ap.add_argument("--n-r", type=int, default=8)
ap.add_argument("--m", type=int, default=4)
ap.add_argument("--members", type=int, nargs="+", default=[2, 4, 8])
ap.add_argument("--skip-recurrence", action="store_true", help="leave section (d) out")
ap.add_argument("--out")
a = ap.parse_args()

lib, ptr = _lib.load(), _lib.ptr
dev = torch.device("cuda:%d" % torch.cuda.current_device())
B, F, N, n_t, m = a.frames, a.per_group, a.n_sub, a.n_t, a.m
G = (B + F - 1) // F
KMAX = max(a.members)
WARM, REPS = 3, 9
stream = _lib.stream_handle()
gen = torch.Generator(device=dev).manual_seed(1)
tx = torch.randint(0, 2, (B, N * m, n_t), dtype=torch.uint8, device=dev, generator=gen)
p_i = torch.full((G,), 0.1, dtype=torch.float64, device=dev)
err = torch.zeros(G, dtype=torch.int64, device=dev)
nb = torch.zeros(G, dtype=torch.int64, device=dev)
merr = torch.zeros((G, KMAX), dtype=torch.int64, device=dev)
wts = torch.rand((G, KMAX), dtype=torch.float64, device=dev, generator=gen)


def timed(calls):
    """[(name, fn)] -> {name: sorted ms}: interleaved, every repetition runs the calls one after the other."""
    for _ in range(WARM):
        for _, fn in calls:
            fn()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in calls]
          for _ in range(REPS)]
    for r in range(REPS):
        for (s, e), (_, fn) in zip(ev[r], calls):
            s.record(); fn(); e.record()
    torch.cuda.synchronize()
    return {name: sorted(ev[r][i][0].elapsed_time(ev[r][i][1]) for r in range(REPS)) for i, (name, _) in enumerate(calls)}


def row(name, ms, extra=""):
    return f"{name:58s} {ms[REPS // 2]:8.3f} ms  ({ms[0]:.3f} .. {ms[-1]:.3f}){extra}"


info = _lib.device_info()
lines = [f"{info['arch']}, {info['cu_count']} CUs; {B} frames in groups of {F}, N = {N}, n_t = {n_t}, m = {m}; device "
         f"events, {WARM} warm-ups, median (min .. max) of {REPS}, interleaved per section"]
verdict = None
for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
    es = 4 if dtype == torch.float32 else 8
    Y = torch.randn((KMAX, B, N, 2 * n_t), dtype=dtype, device=dev, generator=gen) * (N * 0.1) ** 0.5
    Yc = torch.empty_like(Y)
    fused_fn = lib.esn_detect_count_ens_f32 if dtype == torch.float32 else lib.esn_detect_count_ens
    single_fn = lib.esn_detect_count_f32 if dtype == torch.float32 else lib.esn_detect_count

    def fused(K, w=None, me=None):
        def fn():
            _lib.check(fused_fn(ptr(Y), K, B, F, N, n_t, m, ptr(p_i), ptr(w), ptr(tx), ptr(err), ptr(nb), ptr(me), None,
                                stream), "esn_detect_count_ens")
        return fn

    def unfused(K, w=None):
        w = None if w is None else w.to(dtype)

        def fn():
            if w is None:
                y = Y[:K].mean(0)
            else:
                y = torch.einsum("gk,kgfns->gfns", w, Y[:K].view(K, G, F, N, 2 * n_t)).reshape(B, N, 2 * n_t)
            _lib.check(single_fn(ptr(y), B, F, N, n_t, m, ptr(p_i), ptr(tx), ptr(err), ptr(nb), None, stream),
                       "esn_detect_count")
        return fn

    def copy(K):
        return lambda: Yc[:K].copy_(Y[:K])

    calls = []
    for K in a.members:
        calls += [(f"{tag} K={K} fused tail", fused(K)), (f"{tag} K={K} mean(0) + detect_count", unfused(K)),
                  (f"{tag} K={K} copy of the K slabs", copy(K))]
    ragged = B % F != 0                     # (the einsum view needs whole groups)
    if 4 in a.members:
        w4 = wts[:, :4].contiguous()
        me4 = merr[:, :4].contiguous()
        calls += [(f"{tag} K=4 fused tail, weights", fused(4, w=w4)),
                  (f"{tag} K=4 fused tail, member_err", fused(4, me=me4))]
        if not ragged:
            calls += [(f"{tag} K=4 einsum(weights) + detect_count", unfused(4, w=w4))]
    calls += [(f"{tag} detect_count on one slab", lambda: _lib.check(
        single_fn(ptr(Y), B, F, N, n_t, m, ptr(p_i), ptr(tx), ptr(err), ptr(nb), None, stream), "esn_detect_count"))]
    t = timed(calls)
    slab_gb = B * N * 2 * n_t * es / 1e9
    for K in a.members:
        f_, u_, c_ = (t[f"{tag} K={K} {s}"] for s in ("fused tail", "mean(0) + detect_count", "copy of the K slabs"))
        mid = REPS // 2
        lines.append(row(f"{tag} K={K} fused tail", f_, f"  {(K * slab_gb + tx.numel() / 1e9) / f_[mid]:.2f} TB/s read"))
        lines.append(row(f"{tag} K={K} mean(0) + detect_count", u_))
        lines.append(row(f"{tag} K={K} copy of the K slabs", c_))
        lines.append(f"    fused / unfused = {f_[mid] / u_[mid]:.3f}   fused / copy = {f_[mid] / c_[mid]:.3f}")
        if tag == "f32" and K == 4:
            verdict = f_[mid] / u_[mid]
    for name in t:
        if "weights" in name or "member_err" in name or "one slab" in name:
            lines.append(row(name, t[name]))
    del Y, Yc
    torch.cuda.empty_cache()
if verdict is not None:
    lines.append(f"judged: fused / unfused at K = 4, float32 Y = {verdict:.3f} (must not exceed 1): "
                 + ("ok" if verdict <= 1.0 else "MISSED"))

if not a.skip_recurrence:
    # (d) equal recurrence FLOPs: K members of 256 units against one of 512, fp16 operands, float32 I/O
    n_in, n_out, cp, d = 2 * a.n_r, 2 * n_t, 7, 3
    T_in, T, forget = N + cp, N + cp + d, d + cp
    K = 4

    def bank(n, seed):
        b = ReservoirBank(n_in, n_out, n, *draw_reservoir(n_in, n_out, n, 0.9, 0.1, seed), noise=0.001, device=dev)
        b.set_scaling(np.full((G, n_in), 0.05), None, np.full((G, n_out), 0.05), None)
        b.set_readout(torch.randn((G, n_out, n + n_in), dtype=torch.float64, device=dev, generator=gen) * 0.01)
        return b

    small = EnsembleBank([bank(256, 10 + k) for k in range(K)])
    big = bank(512, 99)
    U = torch.randn((B, T_in, n_in), dtype=torch.float32, device=dev, generator=gen)
    Ys = torch.empty((K, B, T - forget, n_out), dtype=torch.float32, device=dev)
    Yb = torch.empty((B, T - forget, n_out), dtype=torch.float32, device=dev)
    Up = torch.zeros((G, T, n_in), dtype=torch.float64, device=dev)
    Dp = torch.zeros((G, T, n_out), dtype=torch.float64, device=dev)
    Up[:, :T_in] = torch.randn((G, T_in, n_in), dtype=torch.float64, device=dev, generator=gen)
    Dp[:, d:] = torch.randn((G, T_in, n_out), dtype=torch.float64, device=dev, generator=gen)
    fit_kw = dict(transient=forget, precision="f16", method="auto", e_dtype="f32", ridge=1e-3)
    mid = REPS // 2
    # two sections: a fit drops its bank's packed read-out, which the next predict would pack again inside its timing
    calls = [(f"{K} x predict, N_res = 256, fp16 (one U, K slabs)",
              lambda: small.predict(U, F, T=T, transient=forget, precision="f16", io="f32", out=Ys)),
             ("1 x predict, N_res = 512, fp16",
              lambda: big.predict(U, F, T=T, transient=forget, precision="f16", io="f32", out=Yb))]
    t = timed(calls)
    for name, _ in calls:
        lines.append(row(name, t[name]))
    lines.append(f"    K predicts / one = {t[calls[0][0]][mid] / t[calls[1][0]][mid]:.3f}")
    calls = [(f"{K} x fit, N_res = 256 (harvest fp16 + ridge solve), {G} pilots", lambda: small.fit(Up, Dp, **fit_kw)),
             (f"1 x fit, N_res = 512 (harvest fp16 + ridge solve), {G} pilots", lambda: big.fit(Up, Dp, **fit_kw))]
    t = timed(calls)
    for name, _ in calls:
        lines.append(row(name, t[name]))
    lines.append(f"    K fits / one = {t[calls[0][0]][mid] / t[calls[1][0]][mid]:.3f}")
print("\n".join(lines))
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
