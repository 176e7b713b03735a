"""The read-out fit of every bank (ReservoirBank, elm.ElmBank): rows E and a teacher D in, W_out and a status out.

    ReadoutFit     solve (pinv of ESN.fit, libs/pyESN.py:191-192, or ridge; QR, Cholesky, leave-one-out choice),
                   resolve_failed, the running normal equations (gram_accumulate, gram_solve on a GramState) and
                   the hold-out choice among candidates (holdout_choose)

None of it reads a reservoir: ReadoutFit is mixed into a bankbase.DeviceBank and needs of it n_outputs, the teacher
scalings, _scratch and _check_groups."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check, ptr
from .bankbase import _as_dev

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
    """A read-out kept as running normal equations (ReadoutFit.gram_accumulate): G [groups, cols, cols] and
    C [groups, n_out, cols], float64 on the device, and the teacher scalings (t_scale, t_shift: [groups, n_out] or None)
    every segment was accumulated under.  Its size does not depend on the number of segments it has seen."""
    __slots__ = ("G", "C", "t_scale", "t_shift")

    def __init__(self, G, C, t_scale, t_shift):
        self.G, self.C, self.t_scale, self.t_shift = G, C, t_scale, t_shift


class ReadoutFit:
    # what the last solve left (device tensors; None until then, see solve, gram_solve and _solve_at_winner)
    last_solve_status = None
    last_ridge_choice = last_ridge_scores = last_ridge_status = last_ridge_grid = last_ridge_lambda = None

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
        and last_ridge_lambda takes that value; the choice stays -1.  A status of -9 (ReservoirBank.fit: the harvest
        cluster kernel timed out, the states were never written) is not repaired: EsnHipError, W_out and status
        untouched."""
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

    # ------------------------------------------------------------------ choice on a held-out segment
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

    def _solve_at_winner(self, lam, status_l, scores, choice, solve_at):
        """The last step of a hold-out choice: `choice` [G] among the candidates lam [G, L] (holdout_choose on the
        multi-lambda solve that gave status_l) -> solve_at(lambdas [G]) = (W_out, status) at every group's winner.  A
        group without a choice is solved at lambda 0 for the launch's sake, then zeroed and flagged 1.  Leaves the
        last_ridge_* record as the leave-one-out choice does; returns (W_out, status)."""
        torch = self.torch
        with torch.cuda.device(self.device):
            none = choice < 0
            picked = lam.gather(1, choice.clamp(min=0).long()[:, None])[:, 0]
            W_out, status = solve_at(torch.where(none, torch.zeros_like(picked), picked))
            W_out = torch.where(none[:, None, None], torch.zeros_like(W_out), W_out)
            status = torch.where(none, torch.ones_like(status), status)
            self.last_ridge_choice, self.last_ridge_scores, self.last_ridge_status = choice, scores, status_l
            self.last_ridge_grid = lam
            self.last_ridge_lambda = torch.where(none, torch.full_like(picked, float("nan")), picked)
        self.last_solve_status = status
        return W_out, status
