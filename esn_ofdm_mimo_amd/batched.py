"""Batched, device-resident form of the ESN hot path.

``ReservoirBank`` holds G echo-state networks on one GPU -- either one shared
reservoir (W, W_in, W_feedb) with G readouts ("shared-reservoir" mode) or one
reservoir per group ("reference-faithful" mode, the reference draws a fresh
reservoir per coherence block) -- and runs the reference's three
operations for all of them at once through the C ABI of ``include/esn_hip.h``:

    harvest  -> state-collection loop of ESN.fit      (libs/pyESN.py:176-189)
    solve    -> pinv readout solve of ESN.fit         (libs/pyESN.py:191-192)         readout.ReadoutFit
    predict  -> ESN.predict                           (libs/pyESN.py:218-255)
    detect   -> reconstruct/FFT/slicer/error count    (Demo_MIMO_4x8_..._v2.py:47-58,439-456)   bankbase.DetectorTail

This module holds the recurrence: weights and their packing, harvest, predict, and fit / fit_pilots, which put a
harvest in front of the read-out fit.  The read-out fit itself (readout.py) and the detector tail (bankbase.py) read
no reservoir; the bank inherits them, and so do the windowed comparators (elm.py, fnn.py).

torch is used for device memory and streams only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import PRECISIONS, Shape, check, ptr
from .bankbase import DetectorTail, DeviceBank, _as_dev
from .readout import _HARVEST_TIMED_OUT, GramState, ReadoutFit, _lambdas  # noqa: F401  (GramState: importable from here)


class ReservoirBank(DeviceBank, ReadoutFit, DetectorTail):
    W_out = None
    # what the last harvest / fit left (device tensors; None until then, see those methods; ReadoutFit: the solve's)
    harvest_timeout = _cluster_err = fit_ridge = fit_status = fit_rows = None
    gram_state = None                           # fit_pilots(method="gram"): the GramState behind W_out

    def __init__(self, n_inputs, n_outputs, n_reservoir, W, W_in, W_feedb,
                 teacher_forcing=True, noise=0.001, device=None, leak_rate=1.0):
        DeviceBank.__init__(self, device)
        self.n_inputs, self.n_outputs, self.n_reservoir = int(n_inputs), int(n_outputs), int(n_reservoir)
        self.noise = float(noise)
        if not 0.0 < float(leak_rate) <= 1.0:
            raise ValueError("leak_rate must be in (0, 1]")
        self.leak_rate = float(leak_rate)       # extension (the reference has none): float64 kernels only when != 1
        self.shape = Shape(n_reservoir, n_inputs, n_outputs, 1 if teacher_forcing else 0, 0, self.leak_rate)
        self.set_weights(W, W_in, W_feedb)
        self._packed_wout = {}

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
        bank = cls(n_inputs, n_outputs, n_reservoir, W, W_in, W_fb, teacher_forcing=teacher_forcing, noise=noise,
                   device=dev, leak_rate=leak_rate)
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
        if ridge_grid is None:
            W_out, status = self.gram_solve(state, ridge)
            self.fit_ridge = ridge
        else:
            W_out, status = self._solve_at_winner(lam, status_l, scores, choice, lambda at: self.gram_solve(state, at))
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
        fits = self.chol_fits(rows, cols)
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
            W_out, status = self._solve_at_winner(lam, status_l, scores, choice,
                                                  lambda at: self.solve(E_all, D_all, 0, method=kind, ridge=at))
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

    # ------------------------------------------------------------------ helpers
    def _error_word(self, ws, wbytes):
        """int32 view [1] of the error word that the two cluster kernels (paths "cluster_f64", "harvest_cluster")
        keep 64 bytes before the end of their workspace: non-zero after a workgroup gave up waiting for its peers."""
        return ws[wbytes - 64:wbytes - 60].view(self.torch.int32)

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
