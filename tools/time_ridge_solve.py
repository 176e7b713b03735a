#!/usr/bin/env python3
"""Time of the read-out solve with and without ridge at the benchmark's fit: 2048 systems of 128 x 528 with float32
extended states (the LDS Cholesky kernel, csrc/esn_solve_chol.hip).  Device events around each launch, warm-up first,
median (and minimum) of the repeats; the candidates alternate inside every repeat, all in one process:

    parent pinv    esn_readout_solve_chol_batch_f32 of another build of the library (--parent-lib, e.g. the parent commit's)
    pinv           esn_readout_solve_chol_batch_f32 of this tree
    ridge L = 1    esn_readout_solve_chol_ridge_batch_f32, one lambda per system
    ridge L = 8    ... eight lambdas per system in one launch (one workgroup per (system, lambda))
    parent ridge   ... L = 1 of the --parent-lib build
    loo L = 1      esn_readout_ridge_loo_batch_f32 (csrc/esn_loo.hip): one candidate, its score, W_out
    loo L = 8      ... eight candidates per system: one Gram pass, eight factorisations and scores, one W_out

    python tools/time_ridge_solve.py [--parent-lib path/to/libesn_hip.so] [--groups 2048] [--repeats 15] [--e64]

--e64: float64 extended states, the entry points without _f32 (other instances of the same kernels).
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from esn_ofdm_mimo_amd import _lib  # noqa: E402
from esn_ofdm_mimo_amd._lib import check, ptr  # noqa: E402
from tools.time_chan_metrics import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--groups", type=int, default=2048)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--cols", type=int, default=528)
    ap.add_argument("--n-out", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--lam", type=float, default=1e-3)
    ap.add_argument("--e64", action="store_true", help="float64 E: the entry points without _f32")
    a = ap.parse_args()
    lib = _lib.load()
    G, rows, cols, n_out, tr = a.groups, a.rows, a.cols, a.n_out, 10
    T = rows + tr
    gen = torch.Generator(device="cuda").manual_seed(5)
    E = torch.randn((G, T, cols), generator=gen, device="cuda", dtype=torch.float64 if a.e64 else torch.float32)
    sfx = "" if a.e64 else "_f32"
    D = torch.randn((G, T, n_out), generator=gen, device="cuda", dtype=torch.float64)
    st = _lib.stream_handle()
    fns, outs = {}, {}

    def pinv_call(l, name):
        fn = getattr(l, "esn_readout_solve_chol_batch" + sfx)
        fn.restype, fn.argtypes = _lib.SIGNATURES["esn_readout_solve_chol_batch" + sfx]
        W = torch.empty((G, n_out, cols), dtype=torch.float64, device="cuda")
        s = torch.empty(G, dtype=torch.int32, device="cuda")
        outs[name] = (W, s)
        return lambda: check(fn(ptr(E), ptr(D), G, T, tr, cols, n_out, None, None, ptr(W), ptr(s), None, 0, st), name)

    def ridge_call(nl, name, lam, l=None):
        fn = getattr(l or lib, "esn_readout_solve_chol_ridge_batch" + sfx)
        fn.restype, fn.argtypes = _lib.SIGNATURES["esn_readout_solve_chol_ridge_batch" + sfx]
        W = torch.empty((G, nl, n_out, cols), dtype=torch.float64, device="cuda")
        s = torch.empty((G, nl), dtype=torch.int32, device="cuda")
        r = torch.full((G, nl), lam, dtype=torch.float64, device="cuda")
        outs[name] = (W, s)
        return lambda: check(fn(
            ptr(E), ptr(D), G, T, tr, cols, n_out, None, None, ptr(r), nl, ptr(W), ptr(s), None, 0, st), name)

    def loo_call(nl, name, lam):
        W = torch.empty((G, n_out, cols), dtype=torch.float64, device="cuda")
        sc = torch.empty((G, nl), dtype=torch.float64, device="cuda")
        ch = torch.empty(G, dtype=torch.int32, device="cuda")
        s = torch.empty((G, nl), dtype=torch.int32, device="cuda")
        # distinct candidates around lam, half a decade apart
        r = (lam * 10.0 ** (0.5 * torch.arange(nl, dtype=torch.float64, device="cuda"))).expand(G, nl).contiguous()
        wb = lib.esn_readout_ridge_loo_workspace_bytes(G, nl, rows, cols)
        ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
        outs[name] = (W, s)
        keep[name] = (r, sc, ch, ws)
        return lambda: check(getattr(lib, "esn_readout_ridge_loo_batch" + sfx)(
            ptr(E), ptr(D), G, T, tr, cols, n_out, None, None, ptr(r), nl, ptr(W), ptr(sc), ptr(ch), ptr(s), ptr(ws), wb,
            st), name)

    keep = {}
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        fns["parent pinv"] = pinv_call(parent, "parent pinv")
        fns["parent ridge"] = ridge_call(1, "parent ridge", a.lam, parent)
    fns["pinv"] = pinv_call(lib, "pinv")
    fns["ridge L = 1"] = ridge_call(1, "ridge L = 1", a.lam)
    fns["ridge L = 8"] = ridge_call(8, "ridge L = 8", a.lam)
    fns["loo L = 1"] = loo_call(1, "loo L = 1", a.lam)
    fns["loo L = 8"] = loo_call(8, "loo L = 8", a.lam)
    print(f"device {_lib.device_info()['arch']}  {G} systems of {rows} x {cols}, {'float64' if a.e64 else 'float32'} E, n_out {n_out}, "
          f"lambda {a.lam:g}  repeats {a.repeats} (median [min .. max])")
    ms = timed(fns, warmup=3, repeats=a.repeats)
    base = ms["pinv"][len(ms["pinv"]) // 2]
    for k, v in ms.items():
        med = v[len(v) // 2]
        print(f"  {k:12s} {med:8.3f} ms [{v[0]:8.3f} .. {v[-1]:8.3f}]   {med / base:6.3f} x pinv   "
              f"{G * (outs[k][1].numel() // G) / med:8.1f} solves/ms")
    for k, (W, s) in outs.items():
        assert int(s.ne(0).sum().item()) == 0, k
    if a.parent_lib:
        print("  parent pinv == pinv bitwise:", bool(torch.equal(outs["parent pinv"][0], outs["pinv"][0])))
        print("  parent ridge == ridge L = 1 bitwise:", bool(torch.equal(outs["parent ridge"][0], outs["ridge L = 1"][0])))
    W0 = ridge_call(1, "ridge 0", 0.0)
    W0()
    torch.cuda.synchronize()
    print("  ridge(lambda = 0) == pinv bitwise:", bool(torch.equal(outs["ridge 0"][0][:, 0], outs["pinv"][0])))
    w_r, w_l = outs["ridge L = 1"][0][:, 0], outs["loo L = 1"][0]
    print(f"  loo L = 1 against ridge L = 1: max |dW| / max |W| = {float((w_l - w_r).abs().max() / w_r.abs().max()):.2e}")
    print("  loo L = 8 choices:", torch.bincount(keep["loo L = 8"][2].clamp(min=0).long(), minlength=8).tolist())


if __name__ == "__main__":
    main()
