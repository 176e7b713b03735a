"""Reservoirs drawn, measured and rescaled on the device: what ``ESN.initweights`` does on the host
(pyESN.py:93-109 -- uniform draw, sparsify, spectral radius, rescale), for a batch of weight sets and without an
eigensolver.  The spectral radius is the ratio form of repeated squaring (esn_spectral_radius_batch in
include/esn_hip.h): 24 squarings are within 1e-7 relative of ``max|eigvals|`` on the reference's matrices.

    radius = spectral_radius(W)                          # [n, n] or [S, n, n], NumPy or torch -> device tensor
    radius = spectral_radius(W, 16, precision="f16x2")   # the squarings on the fp16 matrix pipe, operands split in two
    W, W_in, W_fb, radius, status = generate(n_in, n_out, n_res, 0.9, 0.1, seed, first_set=b0, n_sets=n)

torch is used for device memory and streams only; a missing library or GPU is an error."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import EsnHipError, check, ptr

N_SQUARINGS = 24
# precision -> (workspace query, entry point): "f64" squares on the float64 matrix pipe; "f16x2" splits every operand
# into two fp16 pieces and squares with three float32-accumulated fp16 products (esn_spectral_radius_split_batch:
# within 1e-6 relative of "f64" at the same n_squarings on the reference's matrices)
RADIUS_PRECISIONS = {"f64": ("esn_spectral_radius_workspace_bytes", "esn_spectral_radius_batch"),
                     "f16x2": ("esn_spectral_radius_split_workspace_bytes", "esn_spectral_radius_split_batch")}


def _radius_entry(precision):
    if precision not in RADIUS_PRECISIONS:
        raise ValueError(f"the radius precision must be one of {sorted(RADIUS_PRECISIONS)}, not {precision!r}")
    return RADIUS_PRECISIONS[precision]


def _dev_f64(x, torch, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.float64).contiguous()
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=device)


def _radius_status(W, n_squarings, torch, precision="f64"):
    """(radius [S] float64, status [S] int32) of W [S, n, n] (contiguous float64 on the current device)."""
    query, entry = _radius_entry(precision)
    lib = _lib.load()
    s, n = W.shape[0], W.shape[1]
    radius = torch.empty(s, dtype=torch.float64, device=W.device)
    status = torch.empty(s, dtype=torch.int32, device=W.device)
    wbytes = getattr(lib, query)(s, n)
    if wbytes == 0:
        raise EsnHipError(f"{entry} does not serve n_reservoir = {n}")
    ws = torch.empty(wbytes, dtype=torch.uint8, device=W.device)
    check(getattr(lib, entry)(ptr(W), s, n, int(n_squarings), ptr(radius), ptr(status), ptr(ws), wbytes,
                              _lib.stream_handle()), entry)
    return radius, status


def spectral_radius(W, n_squarings=N_SQUARINGS, device=None, return_status=False, precision="f64"):
    """Spectral radius of W ([n, n] -> 0-d tensor, [S, n, n] -> [S]) on the device, float64.  A matrix whose powers
    vanish or overflow (zero, nilpotent) gets radius 0 and status 1; `return_status` hands the int32 status back too.
    precision: "f64" or "f16x2" (RADIUS_PRECISIONS); with "f16x2" a matrix whose powers fall below the fp16 range may
    be flagged as well."""
    _radius_entry(precision)
    torch = _lib.require_gpu()
    dev = torch.device(device if device is not None else
                       (W.device if isinstance(W, torch.Tensor) and W.is_cuda else "cuda:%d" % torch.cuda.current_device()))
    with torch.cuda.device(dev):
        w = _dev_f64(W, torch, dev)
        single = w.ndim == 2
        if single:
            w = w[None]
        if w.ndim != 3 or w.shape[1] != w.shape[2] or w.shape[0] < 1 or w.shape[1] < 1:
            raise ValueError(f"W must be [n, n] or [S, n, n], not {tuple(w.shape)}")
        radius, status = _radius_status(w, n_squarings, torch, precision)
    if single:
        radius, status = radius[0], status[0]
    return (radius, status) if return_status else radius


def generate(n_in, n_out, n_res, spectral_radius, sparsity, seed, first_set=0, n_sets=1, uniforms=None,
             n_squarings=N_SQUARINGS, device=None, check_status=True, radius_precision="f64", radius=None,
             radius_status=None):
    """The weight sets with global index first_set .. first_set + n_sets - 1, drawn and scaled to `spectral_radius`
    on the device: (W [n_sets, n, n], W_in [n_sets, n, n_in], W_fb [n_sets, n, n_out], radius [n_sets] of the unscaled
    W, status [n_sets]).  Set s sits in slot s % n_sets and is the same bits in any batch (Philox keyed by
    (seed, s, purpose, element)).

    uniforms [n_sets, 2 n^2 + n n_in + n n_out] (NumPy or torch): the draws to consume instead, row i for set
    first_set + i, in the reference's order rand(n, n), mask rand(n, n), rand(n, n_in), rand(n, n_out).

    radius_precision: "f64" or "f16x2", the pipe the radius is measured on (RADIUS_PRECISIONS).

    radius [n_sets] (float64 on the device): known radii of the unscaled W, slot by slot -- the measurement is
    skipped, status is radius_status [n_sets] (int32, the status that came with those radii) or, without it, 1 where
    the radius is 0 (a flagged set's) and 0 elsewhere, and W is bitwise what the path that measured these radii returned.

    A flagged set (its radius cannot be measured: a zero or nilpotent W) raises EsnHipError naming it; that is one
    host read, which check_status=False leaves to the caller (such a set is returned unscaled)."""
    _radius_entry(radius_precision)
    torch = _lib.require_gpu()
    lib = _lib.load()
    dev = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
    n_in, n_out, n, s = int(n_in), int(n_out), int(n_res), int(n_sets)
    if s < 1:
        raise ValueError("n_sets must be at least 1")
    if int(first_set) < 0:
        raise ValueError("first_set must not be negative")
    with torch.cuda.device(dev):
        u = None
        if uniforms is not None:
            u = _dev_f64(uniforms, torch, dev)
            want = (s, 2 * n * n + n * n_in + n * n_out)
            if u.ndim == 1 and s == 1:
                u = u[None]
            if tuple(u.shape) != want:
                raise ValueError(f"uniforms must be {want}, not {tuple(u.shape)}")
        W = torch.empty((s, n, n), dtype=torch.float64, device=dev)
        W_in = torch.empty((s, n, n_in), dtype=torch.float64, device=dev)
        W_fb = torch.empty((s, n, n_out), dtype=torch.float64, device=dev)
        check(lib.esn_gen_reservoirs(n, n_in, n_out, float(sparsity), int(seed) & (2 ** 64 - 1), int(first_set), s,
                                     ptr(u), ptr(W), ptr(W_in), ptr(W_fb), _lib.stream_handle()), "esn_gen_reservoirs")
        if radius is None:
            radius, status = _radius_status(W, n_squarings, torch, radius_precision)
        else:
            if not isinstance(radius, torch.Tensor) or tuple(radius.shape) != (s,):
                raise ValueError(f"radius must be a device tensor of shape ({s},)")
            radius = radius.to(device=dev, dtype=torch.float64).contiguous()
            if radius_status is not None:
                if not isinstance(radius_status, torch.Tensor) or tuple(radius_status.shape) != (s,):
                    raise ValueError(f"radius_status must be a device tensor of shape ({s},)")
                status = radius_status.to(device=dev, dtype=torch.int32).contiguous()
            else:
                status = (~(torch.isfinite(radius) & (radius > 0))).to(torch.int32)  # a flagged set's radius is 0
        check(lib.esn_scale_reservoirs(ptr(W), s, n, float(spectral_radius), ptr(radius), ptr(status),
                                       _lib.stream_handle()), "esn_scale_reservoirs")
        if check_status:
            bad = torch.nonzero(status).flatten().tolist()
            if bad:
                first = int(first_set)
                sets = [next(g for g in range(first, first + s) if g % s == slot) for slot in bad]
                raise EsnHipError(f"generate: the spectral radius of weight set(s) {sets} (slot(s) {bad}) cannot be "
                                  f"measured -- a zero or nilpotent W (n_reservoir={n}, sparsity={sparsity}, seed={seed})")
    return W, W_in, W_fb, radius, status
