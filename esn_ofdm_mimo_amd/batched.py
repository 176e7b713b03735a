"""Batched, device-resident form of the ESN hot path.

``ReservoirBank`` holds G echo-state networks on one GPU -- either one shared
reservoir (W, W_in, W_feedb) with G readouts ("shared-reservoir" mode) or one
reservoir per group ("reference-faithful" mode, the reference draws a fresh
reservoir per coherence block) -- and runs the reference's three
operations for all of them at once through the C ABI of ``include/esn_hip.h``:

    harvest  -> state-collection loop of ESN.fit      (libs/pyESN.py:176-189)
    solve    -> pinv readout solve of ESN.fit         (libs/pyESN.py:191-192)
    predict  -> ESN.predict                           (libs/pyESN.py:218-255)
    detect   -> reconstruct/FFT/slicer/error count    (Demo_MIMO_4x8_..._v2.py:47-58,439-456)

torch is used for device memory and streams only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import PRECISIONS, Shape, check, ptr


def _as_dev(x, torch, device, dtype=None):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        t = x.to(device=device, dtype=dtype or torch.float64)
    else:
        a = np.ascontiguousarray(x)
        if not a.flags.writeable:                 # (arrays out of an .npz are read-only; torch wants ownership)
            a = a.copy()
        t = torch.as_tensor(a, device=device).to(dtype or torch.float64)
    return t.contiguous()


_HARVEST_TIMED_OUT = ("harvest cluster kernel: a workgroup timed out waiting for the others "
                      "(the device is oversubscribed); the extended states are invalid")


def _lambdas(torch, device, lam, g, grid=False):
    """The lambdas of G groups -- `ridge` (a scalar, [G] or [G, L]) or, with `grid`, `ridge_grid` (L candidates or
    [G, L]), as an array, a sequence or a tensor -> (device float64 [G, L], whether the caller gave no L axis)."""
    flat = not grid and (lam.ndim if isinstance(lam, torch.Tensor) else np.ndim(lam)) < 2
    if isinstance(lam, torch.Tensor):
        r = lam.to(device=device, dtype=torch.float64)
    elif flat and np.ndim(lam) == 0:
        r = torch.full((g, 1), float(lam), dtype=torch.float64, device=device)   # (no host copy)
    else:
        r = torch.as_tensor(np.array(lam, dtype=np.float64), device=device)
    if r.ndim == 1:
        r = r[None, :].expand(g, r.shape[0]) if grid else r[:, None]
    elif r.ndim == 0 and not grid:
        r = r.reshape(1, 1).expand(g, 1)
    if r.ndim != 2 or r.shape[0] != g or (r.shape[1] < 1 and not grid):
        raise ValueError(f"ridge_grid must hold L candidates or be [G, L] with G = {g}, not {tuple(r.shape)}" if grid else
                         f"ridge must be a scalar, [G] or [G, L] with G = {g}, not {tuple(r.shape)}")
    return r.contiguous(), flat


class GramState:
    """A read-out kept as running normal equations (ReservoirBank.gram_accumulate): G [groups, cols, cols] and
    C [groups, n_out, cols], float64 on the device, and the teacher scalings (t_scale, t_shift: [groups, n_out] or None)
    every segment was accumulated under.  Its size does not depend on the number of segments it has seen."""
    __slots__ = ("G", "C", "t_scale", "t_shift")

    def __init__(self, G, C, t_scale, t_shift):
        self.G, self.C, self.t_scale, self.t_shift = G, C, t_scale, t_shift


class ReservoirBank:
    def __init__(self, n_inputs, n_outputs, n_reservoir, W, W_in, W_feedb,
                 teacher_forcing=True, noise=0.001, device=None, leak_rate=1.0):
        torch = _lib.require_gpu()
        self.torch = torch
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.n_inputs, self.n_outputs, self.n_reservoir = int(n_inputs), int(n_outputs), int(n_reservoir)
        self.noise = float(noise)
        W = np.asarray(W, dtype=np.float64)
        W_in = np.asarray(W_in, dtype=np.float64)
        W_feedb = np.asarray(W_feedb, dtype=np.float64)
        if W.ndim == 2:
            W, W_in, W_feedb = W[None], W_in[None], W_feedb[None]
        self.n_wsets = W.shape[0]
        if W.shape[1:] != (n_reservoir, n_reservoir) or W_in.shape != (self.n_wsets, n_reservoir, n_inputs) \
                or W_feedb.shape != (self.n_wsets, n_reservoir, n_outputs):
            raise ValueError("weight shapes do not match (n_wsets, n_reservoir, ...)")
        if not 0.0 < float(leak_rate) <= 1.0:
            raise ValueError("leak_rate must be in (0, 1]")
        self.leak_rate = float(leak_rate)       # extension (the reference has none): float64 kernels only when != 1
        self.shape = Shape(n_reservoir, n_inputs, n_outputs, 1 if teacher_forcing else 0, self.n_wsets, self.leak_rate)
        with torch.cuda.device(self.device):
            self._W = _as_dev(W, torch, self.device)
            self._W_in = _as_dev(W_in, torch, self.device)
            self._W_fb = _as_dev(W_feedb, torch, self.device)
        self._packed = {}
        self._packed_wout = {}
        self.in_scale = self.in_shift = self.t_scale = self.t_shift = None
        self.W_out = None
        # what the last harvest / solve / fit left (device tensors; None until then, see those methods)
        self.harvest_timeout = self._cluster_err = self.last_solve_status = None
        self.last_ridge_choice = self.last_ridge_scores = self.last_ridge_status = None
        self.last_ridge_grid = self.last_ridge_lambda = self.fit_ridge = self.fit_status = self.fit_rows = None
        self.gram_state = None                  # fit_pilots(method="gram"): the GramState behind W_out

    def set_weights(self, W, W_in, W_feedb):
        """Swap the weight sets: [n_res, n_res] / [n_res, n_in] / [n_res, n_out], or each with a leading [n_wsets]
        axis.  Device tensors are taken as they are (float64, this device: no host round trip), anything else is
        copied.  The number of sets may change; the packed weights of every precision are dropped and packed again
        at the next call that needs them.  The read-out and the scalings stay."""
        torch = self.torch
        with torch.cuda.device(self.device):
            W, W_in, W_feedb = (_as_dev(x, torch, self.device) for x in (W, W_in, W_feedb))
        if W.ndim == 2:
            W, W_in, W_feedb = W[None], W_in[None], W_feedb[None]
        n_wsets, n = W.shape[0], self.n_reservoir
        if tuple(W.shape[1:]) != (n, n) or tuple(W_in.shape) != (n_wsets, n, self.n_inputs) \
                or tuple(W_feedb.shape) != (n_wsets, n, self.n_outputs):
            raise ValueError("weight shapes do not match (n_wsets, n_reservoir, ...)")
        self.n_wsets = n_wsets
        self.shape = Shape(n, self.n_inputs, self.n_outputs, self.shape.teacher_forcing, n_wsets, self.leak_rate)
        self._W, self._W_in, self._W_fb = W.contiguous(), W_in.contiguous(), W_feedb.contiguous()
        self._packed = {}

    @property
    def weights(self):
        """(W [n_wsets, n_res, n_res], W_in [n_wsets, n_res, n_in], W_fb [n_wsets, n_res, n_out]): float64, device."""
        return self._W, self._W_in, self._W_fb

    @classmethod
    def generate(cls, n_inputs, n_outputs, n_reservoir, spectral_radius=0.9, sparsity=0.1, seed=0, first_set=0,
                 n_sets=1, uniforms=None, teacher_forcing=True, noise=0.001, device=None, leak_rate=1.0,
                 radius_precision="f64", n_squarings=None):
        """A bank whose weight sets are drawn, measured and scaled on the device (reservoirs.generate): the sets with
        global index first_set .. first_set + n_sets - 1, set s in slot s % n_sets, which is the set the kernels pick
        for global group s.  radius_precision and n_squarings (None: reservoirs.N_SQUARINGS) go to
        reservoirs.generate."""
        from . import reservoirs
        torch = _lib.require_gpu()
        dev = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        W, W_in, W_fb, radius, _ = reservoirs.generate(n_inputs, n_outputs, n_reservoir, spectral_radius, sparsity, seed,
                                                       first_set=first_set, n_sets=n_sets, uniforms=uniforms, device=dev,
                                                       radius_precision=radius_precision,
                                                       n_squarings=reservoirs.N_SQUARINGS if n_squarings is None
                                                       else n_squarings)
        n = int(n_reservoir)
        # (placeholders of one set for __init__, which keeps its signature; the device tensors replace them at once)
        bank = cls(n_inputs, n_outputs, n, np.zeros((n, n)), np.zeros((n, int(n_inputs))), np.zeros((n, int(n_outputs))),
                   teacher_forcing=teacher_forcing, noise=noise, device=dev, leak_rate=leak_rate)
        bank.set_weights(W, W_in, W_fb)
        bank.generated_radius = radius          # of the unscaled W, float64 [n_sets] on the device
        return bank

    # ------------------------------------------------------------------ packing
    def tile_frames(self, precision):
        rc = self.lib.esn_tile_frames(PRECISIONS[precision], C.byref(self.shape))
        if rc <= 0:
            check(rc if rc else -2, "esn_tile_frames")
        return rc

    def packed_weights(self, precision):
        if precision not in self._packed:
            torch, p = self.torch, PRECISIONS[precision]
            nbytes = self.lib.esn_packed_weights_bytes(p, C.byref(self.shape))
            if nbytes == 0:
                raise _lib.EsnHipError(f"precision {precision} does not support n_reservoir={self.n_reservoir}")
            with torch.cuda.device(self.device):
                buf = torch.empty(nbytes * self.n_wsets, dtype=torch.uint8, device=self.device)
                check(self.lib.esn_pack_weights(p, C.byref(self.shape), ptr(self._W), ptr(self._W_in),
                                                ptr(self._W_fb), ptr(buf), _lib.stream_handle()),
                      "esn_pack_weights")
            self._packed[precision] = buf
        return self._packed[precision]

    def set_scaling(self, in_scale=None, in_shift=None, t_scale=None, t_shift=None):
        """Per-group scalings, each [G, n] (or None = identity): pyESN.py:127-152."""
        torch = self.torch
        self.in_scale = _as_dev(in_scale, torch, self.device)
        self.in_shift = _as_dev(in_shift, torch, self.device)
        self.t_scale = _as_dev(t_scale, torch, self.device)
        self.t_shift = _as_dev(t_shift, torch, self.device)

    def set_readout(self, W_out):
        """W_out [G, n_out, n_res + n_in] (float64)."""
        self.W_out = _as_dev(W_out, self.torch, self.device)
        if self.W_out.ndim == 2:
            self.W_out = self.W_out[None].contiguous()
        self._packed_wout = {}

    def packed_readout(self, precision):
        if self.W_out is None:
            raise AttributeError("W_out: fit (or set_readout) before predict")
        if precision not in self._packed_wout:
            torch, p = self.torch, PRECISIONS[precision]
            g = self.W_out.shape[0]
            nbytes = self.lib.esn_packed_readout_bytes(p, C.byref(self.shape))
            with torch.cuda.device(self.device):
                buf = torch.empty(nbytes * g, dtype=torch.uint8, device=self.device)
                check(self.lib.esn_pack_readout(p, C.byref(self.shape), g, ptr(self.W_out), ptr(buf),
                                                _lib.stream_handle()), "esn_pack_readout")
            self._packed_wout[precision] = buf
        return self._packed_wout[precision]

    # ------------------------------------------------------------------ fit
    def harvest(self, U, D, precision="f64", noise_mode="counter", noise_u=None, seed=0, e_dtype="f64",
                group_offset=0):
        """U [G,T,n_in], D [G,T,n_out] -> extended states E [G,T,n_res+n_in] (device).

        group_offset: global index of group 0 in the caller's sweep -- the counter noise and (with several
        weight sets) the weight set follow the GLOBAL group, so a sweep cut into chunks or ranks gives the
        same states (include/esn_hip.h).

        e_dtype "f32" (MFMA precisions only) stores E as float32 -- exact for the state columns, 6e-8
        relative on the scaled inputs -- which halves the store tail here and the reads of `solve`."""
        torch = self.torch
        U = _as_dev(U, torch, self.device)
        D = _as_dev(D, torch, self.device)
        g, t = U.shape[0], U.shape[1]
        if D.shape[0] != g or D.shape[1] != t:
            raise ValueError("inputs and teacher disagree on [G, T]")
        self._check_groups(g)
        nm, nz = self._noise_args(noise_mode, noise_u, (g, t - 1, self.n_reservoir))
        with torch.cuda.device(self.device):
            if e_dtype not in ("f64", "f32"):
                raise ValueError("e_dtype must be 'f64' or 'f32'")
            f32 = e_dtype == "f32"
            fn = self.lib.esn_harvest_batch_f32 if f32 else self.lib.esn_harvest_batch
            E = torch.empty((g, t, self.n_reservoir + self.n_inputs),
                            dtype=torch.float32 if f32 else torch.float64, device=self.device)
            # some kernels run out of a caller-owned workspace (include/esn_hip.h: enum esn_path)
            wbytes = self.lib.esn_harvest_workspace_bytes(PRECISIONS[precision], C.byref(self.shape), g)
            ws = self._scratch("_harvest_ws", wbytes)
            check(fn(PRECISIONS[precision], C.byref(self.shape), ptr(self.packed_weights(precision)),
                     ptr(self.in_scale), ptr(self.in_shift), ptr(self.t_scale), ptr(self.t_shift),
                     ptr(U), ptr(D), g, t, self.noise, nm, ptr(nz), int(seed) & (2**64 - 1), int(group_offset),
                     ptr(E), ptr(ws), wbytes, _lib.stream_handle()), "esn_harvest_batch")
            # the two cluster kernels wait for their peers with bounded spins and raise an error word instead of hanging
            path = _lib.recur_path(True, precision, self.shape, g, have_workspace=wbytes > 0)
            if path == "cluster_f64":
                self._cluster_err = self._error_word(ws, wbytes)
            self.harvest_timeout = self._error_word(ws, wbytes) if path == "harvest_cluster" else None
        return E

    def raise_if_harvest_timed_out(self):
        """Host-synchronising check of the last fp16/bf16 harvest on the cluster kernel (see harvest)."""
        if self.harvest_timeout is not None and int(self.harvest_timeout.item()) != 0:
            raise _lib.EsnHipError(_HARVEST_TIMED_OUT)

    def chol_fits(self, rows, cols):
        """Shapes the Cholesky solve covers (esn_readout_solve_chol_batch): Gram dimension up to 128 in LDS,
        up to 512 out of a workspace."""
        return min(rows, cols) <= 512 and self.n_outputs <= 8

    LOO_MAX_GRAM, LOO_MAX_GRID = 128, 16      # esn_readout_ridge_loo_batch: Gram dimension, candidates per group

    # (kind, lambdas given, float32 E) -> (entry point, workspace query, the bank's scratch buffer; None: one per call)
    _READOUT = {
        ("qr", False, False): ("esn_readout_solve_batch", "esn_readout_solve_workspace_bytes", None),
        ("qr", True, False): ("esn_readout_solve_ridge_batch", "esn_readout_solve_ridge_workspace_bytes", None),
        ("chol", False, False): ("esn_readout_solve_chol_batch", "esn_readout_chol_workspace_bytes", "_chol_ws"),
        ("chol", False, True): ("esn_readout_solve_chol_batch_f32", "esn_readout_chol_workspace_bytes", "_chol_ws"),
        ("chol", True, False): ("esn_readout_solve_chol_ridge_batch", "esn_readout_chol_ridge_workspace_bytes", "_chol_ws"),
        ("chol", True, True): ("esn_readout_solve_chol_ridge_batch_f32", "esn_readout_chol_ridge_workspace_bytes", "_chol_ws"),
        ("loo", True, False): ("esn_readout_ridge_loo_batch", "esn_readout_ridge_loo_workspace_bytes", "_loo_ws"),
        ("loo", True, True): ("esn_readout_ridge_loo_batch_f32", "esn_readout_ridge_loo_workspace_bytes", "_loo_ws"),
    }

    def _readout(self, E, D, transient, kind, lam, t_scale, t_shift):
        """The one way into the read-out kernels.  kind "qr", "chol" or "loo" (leave-one-out among the lambdas); lam
        None (pinv) or device float64 [G, L]; t_scale / t_shift the teacher scalings of these G groups.  Returns
        (W_out, status) with an L axis after G where lam is given, for "loo" (W_out [G, n_out, cols], status [G, L],
        scores [G, L], choice [G])."""
        torch, lib, n_out = self.torch, self.lib, self.n_outputs
        e32 = isinstance(E, torch.Tensor) and E.dtype == torch.float32       # as written by harvest(e_dtype="f32")
        E = _as_dev(E, torch, self.device, torch.float32 if e32 else None)
        if e32 and kind == "qr":
            E, e32 = E.double(), False                                      # the QR kernel works in place on float64
        D = _as_dev(D, torch, self.device)
        g, t, cols = E.shape
        nl = () if lam is None else (lam.shape[1],)
        entry, query, scratch = self._READOUT[kind, lam is not None, e32]
        with torch.cuda.device(self.device):
            def new(dtype, *shape):
                return torch.empty(shape, dtype=dtype, device=self.device)
            W_out = new(torch.float64, g, *(nl if kind != "loo" else ()), n_out, cols)
            status = new(torch.int32, g, *nl)
            loo = (new(torch.float64, g, *nl), new(torch.int32, g)) if kind == "loo" else ()      # scores, choice
            wbytes = getattr(lib, query)(g, *nl, t - transient, cols, *((n_out,) if kind == "qr" else ()))
            ws = self._scratch(scratch, wbytes) if scratch else new(torch.uint8, wbytes)
            check(getattr(lib, entry)(ptr(E), ptr(D), g, t, int(transient), cols, n_out, ptr(t_scale), ptr(t_shift),
                                      *((ptr(lam), *nl) if nl else ()), ptr(W_out), *map(ptr, loo), ptr(status), ptr(ws),
                                      *((wbytes,) if kind != "qr" else ()), _lib.stream_handle()),
                  "esn_readout_solve_chol_batch" if (kind, nl) == ("chol", ()) else entry)
        return (W_out, status, *loo)

    def _solve_ridge_grid(self, E, D, transient, ridge_grid):
        """solve(ridge_grid=...): leave-one-out choice among the candidates, one Gram pass per group."""
        torch = self.torch
        g, t, cols = np.shape(E)
        rows = t - transient
        lam, _ = _lambdas(torch, self.device, ridge_grid, g, grid=True)
        nl = lam.shape[1]
        if not 1 <= nl <= self.LOO_MAX_GRID:
            raise ValueError(f"ridge_grid holds {nl} candidates per group, the kernel takes 1 to {self.LOO_MAX_GRID}")
        if min(rows, cols) > self.LOO_MAX_GRAM:
            raise ValueError(f"ridge_grid needs min(rows, cols) <= {self.LOO_MAX_GRAM}, not {min(rows, cols)}")
        if self.n_outputs > 8:
            raise ValueError(f"ridge_grid needs n_outputs <= 8, not {self.n_outputs}")
        W_out, status_l, scores, choice = self._readout(E, D, transient, "loo", lam, self.t_scale, self.t_shift)
        with torch.cuda.device(self.device):
            self.last_ridge_choice = choice
            self.last_ridge_scores = scores
            self.last_ridge_status = status_l
            self.last_ridge_grid = lam
            # (device-side gather; NaN where no candidate survived)
            picked = lam.gather(1, choice.clamp(min=0).long()[:, None])[:, 0]
            self.last_ridge_lambda = torch.where(choice >= 0, picked, torch.full_like(picked, float("nan")))
            status = (choice < 0).to(torch.int32)
        self.last_solve_status = status
        return W_out, status

    def solve(self, E, D, transient, method="qr", ridge=None, ridge_grid=None):
        """W_out[g] = (pinv(E[g][transient:]) @ scale(D[g][transient:])).T ; returns (W_out, status).

        ridge (extension, the reference has none; None = the pinv solve above, untouched): lambda >= 0 of
        W_out = argmin |E W^T - D_s|^2 + lambda |W|^2, absolute, in the units of the Gram matrix of the scaled states.
        A float or a [G] array / tensor gives W_out [G, n_out, cols] and status [G]; a [G, L] one solves L lambdas
        per group in one launch and gives W_out [G, L, n_out, cols] and status [G, L].  lambda = 0 is the pinv solve
        bit for bit; a negative or non-finite lambda gives status 2 and a zero W_out for that entry.

        method "qr": float64 Householder QR (accurate to cond(E) eps; the drop-in's choice).
        method "chol": float64 normal equations on the float64 matrix pipe (min(rows, cols) <= 512, n_out <= 8;
        Gram + factor in LDS up to 128, in a workspace beyond), an order of magnitude faster; groups whose pivot test fails are re-solved
        with QR on the GPU.  "auto" = "chol" when the shape fits.

        ridge_grid (extension): a sequence of L candidates, or a [G, L] array / tensor of them.  Each group takes the
        candidate with the smallest leave-one-out score of its own pilot (esn_readout_ridge_loo_batch: one Gram pass,
        min(rows, cols) <= 128, n_out <= 8, L <= 16; `method` does not apply) and the result is (W_out [G, n_out, cols],
        status [G]) with status 0 where a choice was made and 1 where no candidate survived (W_out zero; see
        resolve_failed).  last_ridge_choice (int32 [G], -1 = none), last_ridge_lambda (float64 [G]) and
        last_ridge_scores ([G, L]) stay on the device."""
        if ridge_grid is not None:
            if ridge is not None:
                raise ValueError("give ridge or ridge_grid, not both")
            return self._solve_ridge_grid(E, D, transient, ridge_grid)
        g, t, cols = np.shape(E)
        fits = self.chol_fits(t - transient, cols)
        if method == "auto":
            method = "chol" if fits else "qr"
        if method == "chol" and not fits:
            raise ValueError("method='chol' needs min(rows, cols) <= 512 and n_outputs <= 8")
        lam, flat = (None, False) if ridge is None else _lambdas(self.torch, self.device, ridge, g)
        W_out, status = self._readout(E, D, transient, "chol" if method == "chol" else "qr", lam,
                                      self.t_scale, self.t_shift)
        if flat:
            W_out, status = W_out[:, 0], status[:, 0]       # (L = 1: contiguous views)
        if method == "chol":
            self.last_solve_status = status        # checked lazily: no host sync on the fast path
        return W_out, status

    def resolve_failed(self, E, D, transient, W_out, status, ridge=None, ridge_grid=None):
        """Re-solve with QR (on the GPU) the groups a "chol" solve flagged; returns their count.  `ridge` as given to
        that solve: each flagged entry is re-solved with its own lambda, so a repaired group is a ridge solution too.
        `ridge_grid` as given to a solve(ridge_grid=...): a group left without a choice (choice == -1, status 1) is
        re-solved by QR at its largest finite candidate -- the most regularised fit the caller was willing to accept --
        and last_ridge_lambda takes that value; the choice stays -1.  A status of -9 (fit: the harvest cluster kernel
        timed out, the states were never written) is not repaired: EsnHipError, W_out and status untouched."""
        torch = self.torch
        if ridge is not None and ridge_grid is not None:
            raise ValueError("give ridge or ridge_grid, not both")
        at = torch.nonzero(status).unbind(1)        # (groups,) of a status [G], (groups, lambdas) of a [G, L] one
        bad, nbad = at[0], int(at[0].numel())
        if not nbad:
            return 0
        if bool(status.eq(-9).any()):
            raise _lib.EsnHipError(_HARVEST_TIMED_OUT)
        lam = None
        if ridge_grid is not None:
            lam = _lambdas(torch, self.device, ridge_grid, status.shape[0], grid=True)[0][bad]
            # (no finite candidate at all: lambda stays negative, the QR solve answers status 2 and a zero W_out)
            lam = torch.where(torch.isfinite(lam), lam, torch.full_like(lam, -1.0)).max(dim=1).values
        elif ridge is not None:
            lam = _lambdas(torch, self.device, ridge, status.shape[0])[0][bad, at[1] if len(at) > 1 else 0]
        W_out[at], status[at] = self.resolve_failed_at(E, D, transient, bad, lam)
        if ridge_grid is not None and self.last_ridge_lambda is not None \
                and self.last_ridge_lambda.shape[0] == status.shape[0]:
            self.last_ridge_lambda[bad] = lam
        return nbad

    def resolve_failed_at(self, E, D, transient, bad, lam):
        """QR solve of the groups `bad` (device index tensor) at lam [len(bad)], or pinv for lam None, under those
        groups' own teacher scalings; returns (W_out, status) of len(bad) groups."""
        def sub(x):
            return None if x is None else x[bad].contiguous()
        out = self._readout(sub(E), sub(_as_dev(D, self.torch, self.device)), transient, "qr",
                            None if lam is None else lam.reshape(-1, 1).contiguous(), sub(self.t_scale), sub(self.t_shift))
        return out if lam is None else (out[0][:, 0], out[1][:, 0])

    def fit(self, U, D, transient=0, precision="f64", noise_mode="counter", noise_u=None, seed=0,
            method="qr", e_dtype="f64", group_offset=0, ridge=None, ridge_grid=None):
        """harvest + solve + set_readout.  ridge: None (pinv), a float or one lambda per group [G] -- see solve.
        ridge_grid: candidates (L or [G, L]); each group's lambda is chosen by leave-one-out on its own pilot and
        fit_ridge becomes the chosen per-group lambda tensor (float64 [G], device)."""
        if ridge is not None and ridge_grid is not None:
            raise ValueError("give ridge or ridge_grid, not both")
        if ridge is not None and np.ndim(ridge) > 1:
            raise ValueError("fit takes one lambda per group (a scalar or [G]); solve() takes [G, L]")
        E = self.harvest(U, D, precision, noise_mode, noise_u, seed, e_dtype=e_dtype, group_offset=group_offset)
        W_out, status = self.solve(E, D, transient, method=method, ridge=ridge, ridge_grid=ridge_grid)
        self.fit_ridge = ridge if ridge_grid is None else self.last_ridge_lambda
        self.set_readout(W_out)
        ht = self.harvest_timeout
        if ht is not None:
            # a harvest cluster that timed out waiting for its peer left invalid states: every group's status says so
            # (-9; device-side, no host sync here -- whoever reads fit_status sees it)
            status = self.torch.where(ht.ne(0).expand_as(status), self.torch.full_like(status, -9), status)
        self.fit_status = status
        return E

    # ------------------------------------------------------------------ running normal equations
    GRAM_MAX_COLS, GRAM_MAX_GRID, GRAM_MAX_OUT = 544, 16, 16      # esn_gram_accumulate / esn_gram_solve

    def gram_accumulate(self, E, D, transient, state=None, decay=1.0):
        """One training segment into a read-out kept as running normal equations (esn_gram_accumulate): over rows
        [transient, T) of E [G, T, cols] (float64, or float32 as harvest(e_dtype="f32") writes it) and the unscaled
        teacher D [G, T, n_out],  G <- decay G + E^T E,  C <- decay C + D_s^T E.  state None: a new GramState under
        this bank's teacher scalings, started with decay 0 (`decay` is not read).  Otherwise `state` is updated in
        place, under the scalings it was started with, and returned; decay in [0, 1] is the forgetting factor, and
        decay 0 starts the sum again without reading what the state held.  Nothing is read back."""
        torch, n_out = self.torch, self.n_outputs
        e32 = isinstance(E, torch.Tensor) and E.dtype == torch.float32
        E = _as_dev(E, torch, self.device, torch.float32 if e32 else None)
        D = _as_dev(D, torch, self.device)
        if E.ndim != 3 or tuple(D.shape) != (E.shape[0], E.shape[1], n_out):
            raise ValueError(f"gram_accumulate takes E [G, T, cols] and D [G, T, {n_out}], not {tuple(E.shape)} and "
                             f"{tuple(D.shape)}")
        g, t, cols = E.shape
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"decay must lie in [0, 1], not {decay}")
        with torch.cuda.device(self.device):
            if state is None:
                self._check_groups(g)
                state = GramState(torch.empty((g, cols, cols), dtype=torch.float64, device=self.device),
                                  torch.empty((g, n_out, cols), dtype=torch.float64, device=self.device),
                                  None if self.t_scale is None else self.t_scale[:g],
                                  None if self.t_shift is None else self.t_shift[:g])
                decay = 0.0
            elif tuple(state.G.shape) != (g, cols, cols) or tuple(state.C.shape) != (g, n_out, cols):
                raise ValueError(f"the state holds G {tuple(state.G.shape)} and C {tuple(state.C.shape)}, the segment "
                                 f"needs [{g}, {cols}, {cols}] and [{g}, {n_out}, {cols}]")
            if E.data_ptr() % 16:               # (a view into a larger buffer: the kernel loads 16-byte units)
                E = E.clone()
            name = "esn_gram_accumulate_f32" if e32 else "esn_gram_accumulate"
            check(getattr(self.lib, name)(ptr(E), ptr(D), g, t, int(transient), cols, n_out, ptr(state.t_scale),
                                          ptr(state.t_shift), float(decay), ptr(state.G), ptr(state.C),
                                          _lib.stream_handle()), name)
        return state

    def gram_solve(self, state, ridge):
        """(G + lambda I) W^T = C^T for the groups of a GramState (esn_gram_solve): the ridge read-out of every row the
        state has seen, weighted by its forgetting.  ridge as in solve: a scalar or [G] gives (W_out [G, n_out, cols],
        status [G]); [G, L] (L <= 16) solves L lambdas per group from the one G and gives W_out [G, L, n_out, cols] and
        status [G, L].  status 1: a pivot was rejected, that entry's W_out is zero (nothing is repaired: the state
        keeps no rows); 2: a negative or non-finite lambda.  The state is only read."""
        torch = self.torch
        g, n_out, cols = state.C.shape
        lam, flat = _lambdas(torch, self.device, ridge, g)
        nl = lam.shape[1]
        if not 1 <= nl <= self.GRAM_MAX_GRID:
            raise ValueError(f"ridge holds {nl} candidates per group, the kernel takes 1 to {self.GRAM_MAX_GRID}")
        with torch.cuda.device(self.device):
            W_out = torch.empty((g, nl, n_out, cols), dtype=torch.float64, device=self.device)
            status = torch.empty((g, nl), dtype=torch.int32, device=self.device)
            wbytes = self.lib.esn_gram_solve_workspace_bytes(g, nl, cols)
            ws = self._scratch("_gram_ws", max(wbytes, 16))
            check(self.lib.esn_gram_solve(ptr(state.G), ptr(state.C), g, cols, n_out, ptr(lam), nl, ptr(W_out),
                                          ptr(status), ptr(ws), wbytes, _lib.stream_handle()), "esn_gram_solve")
        if flat:
            W_out, status = W_out[:, 0], status[:, 0]
        self.last_solve_status = status
        return W_out, status

    def _fit_pilots_gram(self, U, D, transient, precision, noise_mode, noise_u, seed, e_dtype, group_offset, ridge,
                         ridge_grid):
        """fit_pilots(method="gram"): one harvest and one gram_accumulate per pilot, no stacked rows."""
        self._pilot_fit_method(np.shape(U), np.shape(D), transient, "qr", ridge, ridge_grid)      # (the shape checks)
        if ridge is None and ridge_grid is None:
            raise ValueError("method='gram' needs ridge or ridge_grid: with fewer rows than columns the normal "
                             "equations have no pinv solution")
        torch = self.torch
        U = _as_dev(U, torch, self.device)
        D = _as_dev(D, torch, self.device)
        g, P = U.shape[0], U.shape[1]
        if ridge_grid is not None and P < 2:
            raise ValueError("method='gram' chooses among ridge_grid on a held-out pilot: it needs at least two pilots")
        seeds = [int(s) for s in seed] if np.ndim(seed) else [int(seed)] * P
        if len(seeds) != P:
            raise ValueError(f"seed must be one value or one per pilot ({P}), not {len(seeds)}")
        state, timed_out, E = None, None, None
        for p in range(P):
            D_p = D[:, p].contiguous()
            E = self.harvest(U[:, p].contiguous(), D_p, precision, noise_mode,
                             None if noise_u is None else noise_u[:, p], seeds[p], e_dtype=e_dtype,
                             group_offset=group_offset)
            ht = self.harvest_timeout
            if ht is not None:
                timed_out = ht.ne(0) if timed_out is None else timed_out | ht.ne(0)
            if ridge_grid is not None and p == P - 1:
                # the candidates from pilots 0 .. P - 2, all out of the one G, scored on pilot P - 1 before it goes in
                lam, _ = _lambdas(torch, self.device, ridge_grid, g, grid=True)
                W_cand, status_l = self.gram_solve(state, lam)
                scores, choice = self.holdout_choose(E, D_p, transient, W_cand, status_l)
                del W_cand
            state = self.gram_accumulate(E, D_p, transient, state, 1.0)
        with torch.cuda.device(self.device):
            if ridge_grid is None:
                W_out, status = self.gram_solve(state, ridge)
                self.fit_ridge = ridge
            else:
                none = choice < 0
                picked = lam.gather(1, choice.clamp(min=0).long()[:, None])[:, 0]
                # (a group without a choice: solved at lambda 0 for the launch's sake, then zeroed and flagged)
                W_out, status = self.gram_solve(state, torch.where(none, torch.zeros_like(picked), picked))
                W_out = torch.where(none[:, None, None], torch.zeros_like(W_out), W_out)
                status = torch.where(none, torch.ones_like(status), status)
                self.last_ridge_choice, self.last_ridge_scores, self.last_ridge_status = choice, scores, status_l
                self.last_ridge_grid = lam
                self.last_ridge_lambda = torch.where(none, torch.full_like(picked, float("nan")), picked)
                self.last_solve_status = status
                self.fit_ridge = self.last_ridge_lambda
        self.set_readout(W_out)
        self.harvest_timeout = None if timed_out is None else timed_out.to(torch.int32)
        if timed_out is not None:
            status = torch.where(timed_out.expand_as(status), torch.full_like(status, -9), status)
        self.fit_status = status
        self.fit_rows = None
        self.gram_state = state
        return state

    # ------------------------------------------------------------------ several pilots per group
    HOLDOUT_MAX_GRID = 16                     # esn_readout_holdout_score: candidates per group

    def holdout_choose(self, E_val, D_val, transient, W_cand, status=None):
        """Score the candidate read-outs W_cand [G, L, n_out, cols] (a multi-lambda solve's W_out) on rows
        [transient, T) of a segment the fit has not seen -- E_val [G, T, cols] (float64, or float32 as
        harvest(e_dtype="f32") writes it) and its unscaled teacher D_val [G, T, n_out] -- under this bank's teacher
        scalings (esn_readout_holdout_score).  status: that solve's int32 [G, L], or None for all 0.  Returns
        (scores float64 [G, L], +inf where the status is not 0 or the sum is not finite; choice int32 [G], the lowest
        candidate with the smallest finite score, -1 if none).  Device tensors; nothing is read back."""
        torch, n_out = self.torch, self.n_outputs
        e32 = isinstance(E_val, torch.Tensor) and E_val.dtype == torch.float32
        E = _as_dev(E_val, torch, self.device, torch.float32 if e32 else None)
        D = _as_dev(D_val, torch, self.device)
        W = _as_dev(W_cand, torch, self.device)
        if E.ndim != 3 or W.ndim != 4:
            raise ValueError("holdout_choose takes E_val [G, T, cols] and W_cand [G, L, n_out, cols]")
        g, t, cols = E.shape
        nl = W.shape[1]
        if tuple(W.shape) != (g, nl, n_out, cols) or tuple(D.shape) != (g, t, n_out):
            raise ValueError(f"W_cand must be [{g}, L, {n_out}, {cols}] and D_val [{g}, {t}, {n_out}], not "
                             f"{tuple(W.shape)} and {tuple(D.shape)}")
        if not 1 <= nl <= self.HOLDOUT_MAX_GRID:
            raise ValueError(f"W_cand holds {nl} candidates per group, the kernel takes 1 to {self.HOLDOUT_MAX_GRID}")
        status = _as_dev(status, torch, self.device, torch.int32)
        if status is not None and tuple(status.shape) != (g, nl):
            raise ValueError(f"status must be [{g}, {nl}], not {tuple(status.shape)}")
        self._check_groups(g)
        with torch.cuda.device(self.device):
            if E.data_ptr() % 16:               # (a view into a larger buffer: the kernel loads 16-byte units)
                E = E.clone()
            if W.data_ptr() % 16:
                W = W.clone()
            scores = torch.empty((g, nl), dtype=torch.float64, device=self.device)
            choice = torch.empty((g,), dtype=torch.int32, device=self.device)
            name = "esn_readout_holdout_score_f32" if e32 else "esn_readout_holdout_score"
            check(getattr(self.lib, name)(ptr(E), ptr(D), ptr(W), g, t, int(transient), cols, n_out, ptr(self.t_scale),
                                          ptr(self.t_shift), nl, ptr(status), ptr(scores), ptr(choice),
                                          _lib.stream_handle()), name)
        return scores, choice

    def _pilot_fit_method(self, u_shape, d_shape, transient, method, ridge, ridge_grid):
        """The checks of fit_pilots that need no device, on the shapes alone; returns the solve kernel ("chol" or
        "qr") of the stacked system."""
        if len(u_shape) != 4 or len(d_shape) != 4 or tuple(u_shape[:3]) != tuple(d_shape[:3]):
            raise ValueError(f"fit_pilots takes U [G, P, T, n_in] and D [G, P, T, n_out], not {tuple(u_shape)} and "
                             f"{tuple(d_shape)}")
        p, t = int(u_shape[1]), int(u_shape[2])
        if p < 1 or not 0 <= int(transient) < t:
            raise ValueError(f"need at least one pilot and 0 <= transient < T (P = {p}, transient = {transient}, T = {t})")
        if ridge is not None and ridge_grid is not None:
            raise ValueError("give ridge or ridge_grid, not both")
        if ridge is not None and np.ndim(ridge) > 1:
            raise ValueError("fit_pilots takes one lambda per group (a scalar or [G]); solve() takes [G, L]")
        if ridge_grid is not None:
            nl = np.shape(ridge_grid)[-1] if np.ndim(ridge_grid) else 0
            if not 1 <= nl <= self.HOLDOUT_MAX_GRID:
                raise ValueError(f"ridge_grid holds {nl} candidates per group, 1 to {self.HOLDOUT_MAX_GRID} are taken")
        if method not in ("qr", "chol", "auto"):
            raise ValueError(f"method must be 'qr', 'chol' or 'auto', not {method!r}")
        rows, cols = p * (t - int(transient)), self.n_reservoir + self.n_inputs
        fits = min(rows, cols) <= 512 and self.n_outputs <= 8
        if method == "chol" and not fits:
            raise ValueError(f"method='chol' needs min(rows, cols) <= 512 and n_outputs <= 8: {p} pilots stack to "
                             f"{rows} rows against {cols} columns")
        return "chol" if fits and method != "qr" else "qr"

    def fit_pilots(self, U, D, transient=0, precision="f64", noise_mode="counter", noise_u=None, seed=0,
                   method="qr", e_dtype="f64", group_offset=0, ridge=None, ridge_grid=None):
        """fit on P pilots per group: U [G, P, T, n_in], D [G, P, T, n_out].  One harvest per pilot index p over all G
        groups, every pilot from a zero state and under the same group_offset, so weight set, scalings and noise key
        follow the global group as in fit; rows [transient, T) of the P results are stacked along the row axis
        ([G, P (T - transient), cols]) and solved once.  seed: one value, or P of them (pilot p's state-noise stream;
        with one value every pilot of a group sees the same noise).  noise_u (noise_mode="tensor"):
        [G, P, T - 1, n_res].  Returns the stacked extended states; fit_rows keeps (them, the stacked teacher), which
        is what resolve_failed takes with transient 0.

        P = 1 is fit(), bit for bit (ridge_grid: leave-one-out).  With P >= 2, ridge_grid (at most 16 candidates, or
        [G, L]) is chosen on a held-out pilot: the multi-lambda solve runs on pilots 0 .. P - 2, holdout_choose scores
        every candidate on pilot P - 1 (candidates that solve flagged never win), and one solve on all P pilots at each
        group's own winner gives W_out.  last_ridge_choice / _lambda / _scores / _grid, fit_ridge and fit_status mean
        what they mean after the leave-one-out choice; a group without a choice gets status 1 and a zero W_out, which
        resolve_failed(ridge_grid=...) repairs at the largest finite candidate (as it does a group whose last solve
        was flagged).  A harvest that timed out marks every group -9, as in fit.

        method: "chol" refuses a stacked shape outside min(rows, cols) <= 512; "auto" falls back to QR there.  At
        T - transient = 128 and n_reservoir + n_inputs = 528 the Cholesky path therefore ends at P = 4 (512 rows);
        five pilots and more are QR solves.

        method "gram" (needs ridge or ridge_grid; any P >= 1, ridge_grid from P = 2): the primal form.  Every pilot is
        harvested and accumulated into one GramState (gram_accumulate), so no rows are stacked and P is not bounded by
        a kernel's shape.  With ridge_grid the L candidates are solved out of the one G of pilots 0 .. P - 2, scored by
        holdout_choose on pilot P - 1, that pilot is accumulated into the same state and one solve at each group's
        winner gives W_out.  Returns the GramState, which gram_state keeps; fit_rows is None (no rows exist, and a
        flagged group cannot be repaired by resolve_failed)."""
        if method == "gram":
            return self._fit_pilots_gram(U, D, transient, precision, noise_mode, noise_u, seed, e_dtype, group_offset,
                                         ridge, ridge_grid)
        kind = self._pilot_fit_method(np.shape(U), np.shape(D), transient, method, ridge, ridge_grid)
        torch = self.torch
        U = _as_dev(U, torch, self.device)
        D = _as_dev(D, torch, self.device)
        g, P = U.shape[0], U.shape[1]
        seeds = [int(s) for s in seed] if np.ndim(seed) else [int(seed)] * P
        if len(seeds) != P:
            raise ValueError(f"seed must be one value or one per pilot ({P}), not {len(seeds)}")
        if P == 1:
            E = self.fit(U[:, 0], D[:, 0], transient, precision, noise_mode, None if noise_u is None else noise_u[:, 0],
                         seeds[0], method=method, e_dtype=e_dtype, group_offset=group_offset, ridge=ridge,
                         ridge_grid=ridge_grid)
            self.fit_rows = (E[:, transient:], D[:, 0, transient:])
            return self.fit_rows[0]
        Es, timed_out = [], None
        for p in range(P):
            Es.append(self.harvest(U[:, p].contiguous(), D[:, p].contiguous(), precision, noise_mode,
                                   None if noise_u is None else noise_u[:, p], seeds[p], e_dtype=e_dtype,
                                   group_offset=group_offset))
            ht = self.harvest_timeout
            if ht is not None:
                timed_out = ht.ne(0) if timed_out is None else timed_out | ht.ne(0)
        with torch.cuda.device(self.device):
            E_all = torch.cat([e[:, transient:] for e in Es], dim=1)
            D_all = D[:, :, transient:].reshape(g, -1, D.shape[-1]).contiguous()
            rows = E_all.shape[1] // P
        if ridge_grid is None:
            W_out, status = self.solve(E_all, D_all, 0, method=kind, ridge=ridge)
            self.fit_ridge = ridge
        else:
            lam, _ = _lambdas(torch, self.device, ridge_grid, g, grid=True)
            n_fit = (P - 1) * rows
            W_cand, status_l = self._readout(E_all[:, :n_fit].contiguous(), D_all[:, :n_fit].contiguous(), 0, kind, lam,
                                             self.t_scale, self.t_shift)
            scores, choice = self.holdout_choose(Es[P - 1], D[:, P - 1].contiguous(), transient, W_cand, status_l)
            del W_cand
            with torch.cuda.device(self.device):
                none = choice < 0
                picked = lam.gather(1, choice.clamp(min=0).long()[:, None])[:, 0]
                # (a group without a choice: solved at lambda 0 for the launch's sake, then zeroed and flagged)
                W_out, status = self.solve(E_all, D_all, 0, method=kind, ridge=torch.where(none, torch.zeros_like(picked), picked))
                W_out = torch.where(none[:, None, None], torch.zeros_like(W_out), W_out)
                status = torch.where(none, torch.ones_like(status), status)
                self.last_ridge_choice, self.last_ridge_scores, self.last_ridge_status = choice, scores, status_l
                self.last_ridge_grid = lam
                self.last_ridge_lambda = torch.where(none, torch.full_like(picked, float("nan")), picked)
            self.last_solve_status = status
            self.fit_ridge = self.last_ridge_lambda
        self.set_readout(W_out)
        self.harvest_timeout = None if timed_out is None else timed_out.to(torch.int32)
        if timed_out is not None:
            status = torch.where(timed_out.expand_as(status), torch.full_like(status, -9), status)
        self.fit_status = status
        self.fit_rows = (E_all, D_all)
        return E_all

    # ------------------------------------------------------------------ predict
    def predict(self, U, frames_per_group, T=None, transient=0, precision="f32", x0=None, y0=None,
                noise_mode="counter", noise_u=None, seed=0, out=None, group_offset=0, io="f64"):
        """U [B,T_in,n_in] (frames ordered by group) -> Y [B,T-transient,n_out] (device, unscaled).
        group_offset: global index of group 0 (noise key and weight set follow the global group).
        io="f32": U and Y are float32 (esn_predict_batch_f32; a float32 U is used as it is, any other dtype is
        converted once): Y is bitwise the float64 result rounded to float32.  Precisions f32 / f16 / bf16 only."""
        torch = self.torch
        if io not in ("f64", "f32"):
            raise ValueError(f"io must be 'f64' or 'f32', not {io!r}")
        io32 = io == "f32"
        if io32 and precision == "f64":
            raise ValueError("io='f32' needs precision f32, f16 or bf16 (the float64 kernels read and write float64)")
        U = _as_dev(U, torch, self.device, torch.float32 if io32 else None)
        if io32 and U.data_ptr() % 16:          # (a view into a larger buffer: the kernels stage 16-byte chunks)
            U = U.clone()
        b, t_in = U.shape[0], U.shape[1]
        T = t_in if T is None else int(T)
        if not (0 <= int(transient) < T and t_in <= T):
            raise ValueError(f"need 0 <= transient < T and T_in <= T (transient={transient}, T_in={t_in}, T={T})")
        g = (b + frames_per_group - 1) // frames_per_group
        self._check_groups(g)
        if self.W_out is None:
            raise AttributeError("W_out: fit (or set_readout) before predict")
        if self.W_out.shape[0] < g:
            raise ValueError(f"readout holds {None if self.W_out is None else self.W_out.shape[0]} groups, batch needs {g}")
        x0 = _as_dev(x0, torch, self.device)
        y0 = _as_dev(y0, torch, self.device)
        nm, nz = self._noise_args(noise_mode, noise_u, (b, T, self.n_reservoir))
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty((b, T - transient, self.n_outputs), dtype=torch.float32 if io32 else torch.float64,
                                  device=self.device)
            elif out.dtype != (torch.float32 if io32 else torch.float64):
                raise ValueError(f"out is {out.dtype}, io={io!r} writes {'float32' if io32 else 'float64'}")
            # some kernels run out of a caller-owned workspace (include/esn_hip.h: enum esn_path)
            wbytes = self.lib.esn_predict_workspace_bytes(PRECISIONS[precision], C.byref(self.shape), b,
                                                          int(frames_per_group))
            ws = self._scratch("_workspace", wbytes)
            fn = self.lib.esn_predict_batch_f32 if io32 else self.lib.esn_predict_batch
            check(fn(
                PRECISIONS[precision], C.byref(self.shape), ptr(self.packed_weights(precision)),
                ptr(self.packed_readout(precision)), ptr(self.in_scale), ptr(self.in_shift),
                ptr(self.t_scale), ptr(self.t_shift), ptr(U), b, int(frames_per_group), t_in, T,
                int(transient), ptr(x0), ptr(y0), self.noise, nm, ptr(nz), int(seed) & (2**64 - 1),
                int(group_offset), ptr(out), ptr(ws), wbytes, _lib.stream_handle()),
                "esn_predict_batch_f32" if io32 else "esn_predict_batch")
            if _lib.recur_path(False, precision, self.shape, b, frames_per_group, wbytes > 0) == "cluster_f64":
                self._cluster_err = self._error_word(ws, wbytes)     # of the single-sequence cluster kernel
        return out

    def raise_if_cluster_timed_out(self):
        """Host-synchronising check after a single-sequence float64 call (the 2-D drop-in makes it when it copies the
        result to the host): the cluster kernel's workgroups wait for each other with bounded spins and raise an
        error word instead of hanging (include/esn_hip.h, esn_predict_batch: workspace)."""
        w, self._cluster_err = self._cluster_err, None
        if w is not None:
            if int(w.item()) != 0:
                raise _lib.EsnHipError("single-sequence cluster kernel: a workgroup timed out waiting for the others "
                                       "(the device is oversubscribed); outputs are invalid")

    # ------------------------------------------------------------------ detector tail
    def detect_count(self, Y, tx_bits, p_i, frames_per_group, n_sub, n_t, bits_per_sym,
                     err=None, bits=None, want_xhat=False):
        """Y [B,N,2 n_t] -> per-group int64 (errors, bits) accumulated into err/bits.  A float32 Y (predict with
        io="f32") is read as it is by esn_detect_count_f32: the counts and X_hat are those of the widened Y."""
        torch = self.torch
        y32 = getattr(Y, "dtype", None) in (torch.float32, np.float32)
        Y = _as_dev(Y, torch, self.device, torch.float32 if y32 else None)
        b = Y.shape[0]
        g = (b + frames_per_group - 1) // frames_per_group
        p_i = _as_dev(p_i, torch, self.device)
        tx_bits = _as_dev(tx_bits, torch, self.device, dtype=torch.uint8)
        with torch.cuda.device(self.device):
            if err is None:
                err = torch.zeros(g, dtype=torch.int64, device=self.device)
            if bits is None:
                bits = torch.zeros(g, dtype=torch.int64, device=self.device)
            xh = torch.empty((b, n_sub, 2 * n_t), dtype=torch.float64, device=self.device) if want_xhat else None
            fn = self.lib.esn_detect_count_f32 if y32 else self.lib.esn_detect_count
            check(fn(ptr(Y), b, int(frames_per_group), int(n_sub), int(n_t),
                     int(bits_per_sym), ptr(p_i), ptr(tx_bits), ptr(err), ptr(bits),
                     ptr(xh), _lib.stream_handle()), "esn_detect_count_f32" if y32 else "esn_detect_count")
        return (err, bits, xh) if want_xhat else (err, bits)

    def detect_remod(self, Y, tx_bits, p_i, frames_per_group, n_sub, cp, delay, n_t, bits_per_sym,
                     err=None, bits=None, want_xhat=False, want_bits=False):
        """detect_count and, in the same launch, the decisions re-modulated (esn_detect_remod): Y [B, N, 2 n_t] float64
        -> D_hat [B, delay + cp + N, 2 n_t], the time-domain teacher rows of the decided symbols in the layout harvest
        takes (delay zero rows, cyclic prefix, body).  tx_bits None: nothing is counted.  Returns
        (D_hat, err, bits[, X_hat][, dec_bits]) -- err / bits are None without tx_bits, dec_bits uint8 [B, N m, n_t]."""
        torch = self.torch
        if getattr(Y, "dtype", None) in (torch.float32, np.float32):
            raise ValueError("detect_remod reads float64 Y (predict with io='f64'): the tracked path has no float32 I/O")
        Y = _as_dev(Y, torch, self.device)
        b = Y.shape[0]
        g = (b + frames_per_group - 1) // frames_per_group
        p_i = _as_dev(p_i, torch, self.device)
        tx_bits = _as_dev(tx_bits, torch, self.device, dtype=torch.uint8)
        with torch.cuda.device(self.device):
            if tx_bits is not None:
                if err is None:
                    err = torch.zeros(g, dtype=torch.int64, device=self.device)
                if bits is None:
                    bits = torch.zeros(g, dtype=torch.int64, device=self.device)
            else:
                err = bits = None
            xh = torch.empty((b, n_sub, 2 * n_t), dtype=torch.float64, device=self.device) if want_xhat else None
            db = torch.empty((b, n_sub * bits_per_sym, n_t), dtype=torch.uint8, device=self.device) if want_bits else None
            D_hat = torch.empty((b, int(delay) + int(cp) + int(n_sub), 2 * n_t), dtype=torch.float64, device=self.device)
            check(self.lib.esn_detect_remod(ptr(Y), b, int(frames_per_group), int(n_sub), int(cp), int(delay), int(n_t),
                                            int(bits_per_sym), ptr(p_i), ptr(tx_bits), ptr(err), ptr(bits), ptr(xh),
                                            ptr(db), ptr(D_hat), _lib.stream_handle()), "esn_detect_remod")
        return (D_hat, err, bits) + ((xh,) if want_xhat else ()) + ((db,) if want_bits else ())

    # ------------------------------------------------------------------ helpers
    def _scratch(self, name, nbytes):
        """The bank's device scratch `name`, grown on demand to nbytes (None for 0).  Called under the device guard."""
        if not nbytes:
            return None
        ws = getattr(self, name, None)
        if ws is None or ws.numel() < nbytes:
            ws = self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.device)
            setattr(self, name, ws)
        return ws

    def _error_word(self, ws, wbytes):
        """int32 view [1] of the error word that the two cluster kernels (paths "cluster_f64", "harvest_cluster")
        keep 64 bytes before the end of their workspace: non-zero after a workgroup gave up waiting for its peers."""
        return ws[wbytes - 64:wbytes - 60].view(self.torch.int32)

    def _check_groups(self, g):
        for name in ("in_scale", "in_shift", "t_scale", "t_shift"):
            t = getattr(self, name)
            if t is not None and t.shape[0] < g:
                raise ValueError(f"{name} holds {t.shape[0]} groups, batch has {g}")

    def _noise_args(self, noise_mode, noise_u, shape):
        if self.noise == 0.0 or noise_mode in (None, "none"):
            return _lib.NOISE_NONE, None
        if noise_mode == "tensor":
            nz = _as_dev(noise_u, self.torch, self.device)
            if nz is None or tuple(nz.shape) != tuple(shape):
                raise ValueError(f"noise_u must have shape {shape}")
            return _lib.NOISE_TENSOR, nz
        if noise_mode == "counter":
            return _lib.NOISE_COUNTER, None
        raise ValueError("noise_mode must be 'none', 'tensor' or 'counter'")
