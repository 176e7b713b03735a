"""Reservoir ensembles: K independently drawn ReservoirBank members per coherence block, each with its own read-out
fitted on the block's pilot; their time-domain outputs are combined and the detector tail runs once.

    fit      every member on the same pilots (K harvests + K solves, member k under its own state-noise seed)
    predict  K launches on the one U, member k into slab k of Y [K, B, T - transient, n_out]
    detect   esn_detect_count_ens: the ordered weighted sum of the slabs -> FFT / slicer / error count, one launch

The members read no common state: member k built alone gives slab k bit for bit.  A one-member ensemble is its
ReservoirBank bit for bit (weight 1.0, 1.0 y = y).  torch is used for device memory and streams only."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check, ptr
from .bankbase import _as_dev

MAX_MEMBERS = 16            # esn_detect_count_ens


class EnsembleBank:
    def __init__(self, members):
        """members: 1..16 ReservoirBank of one shape (n_inputs, n_outputs, n_reservoir) on one device; their weights
        should differ -- equal members only repeat each other."""
        members = list(members)
        if not 1 <= len(members) <= MAX_MEMBERS:
            raise ValueError(f"an ensemble holds 1 to {MAX_MEMBERS} members, not {len(members)}")
        m0 = members[0]
        for m in members[1:]:
            if (m.n_inputs, m.n_outputs, m.n_reservoir) != (m0.n_inputs, m0.n_outputs, m0.n_reservoir) \
                    or m.device != m0.device:
                raise ValueError("the members of an ensemble share one shape and one device")
        self.members = members
        self.torch, self.lib, self.device = m0.torch, m0.lib, m0.device
        self.n_inputs, self.n_outputs, self.n_reservoir = m0.n_inputs, m0.n_outputs, m0.n_reservoir

    @property
    def n_members(self):
        return len(self.members)

    def _per_member(self, name, value):
        """One value for all members, or a sequence of K."""
        if np.ndim(value) == 0:
            return [value] * self.n_members
        if len(value) != self.n_members:
            raise ValueError(f"{name} must be one value or one per member ({self.n_members}), not {len(value)}")
        return list(value)

    def set_scaling(self, in_scale=None, in_shift=None, t_scale=None, t_shift=None):
        for m in self.members:
            m.set_scaling(in_scale, in_shift, t_scale, t_shift)

    def fit(self, U, D, transient=0, precision="f64", noise_mode="counter", seed=0, method="qr", e_dtype="f64",
            group_offset=0, ridge=None, ridge_grid=None):
        """ReservoirBank.fit of every member on the same pilots U [G, T, n_in], D [G, T, n_out].  seed: one value or
        one per member (member k's state-noise stream).  Returns the K extended-state tensors; fit_status is
        [K, G] (device), nothing is read back."""
        torch = self.torch
        U = _as_dev(U, torch, self.device)
        D = _as_dev(D, torch, self.device)
        seeds = self._per_member("seed", seed)
        Es = [m.fit(U, D, transient, precision, noise_mode, None, seeds[k], method=method, e_dtype=e_dtype,
                    group_offset=group_offset, ridge=ridge, ridge_grid=ridge_grid)
              for k, m in enumerate(self.members)]
        self._fit_io = (D, int(transient), ridge, ridge_grid)
        return Es

    @property
    def fit_status(self):
        """int32 [K, G] on the device: the members' fit_status."""
        return self.torch.stack([m.fit_status for m in self.members])

    @property
    def W_out(self):
        """[K, G, n_out, n_res + n_in] on the device: the members' read-outs."""
        return self.torch.stack([m.W_out for m in self.members])

    def resolve_failed(self, Es):
        """ReservoirBank.resolve_failed per member on the states fit returned (host-synchronising): the groups a
        Cholesky solve flagged are solved again by QR at their own lambda.  Returns how many were."""
        D, transient, ridge, ridge_grid = self._fit_io
        n = 0
        for m, E in zip(self.members, Es):
            k = m.resolve_failed(E, D, transient, m.W_out, m.fit_status, ridge_grid=ridge_grid,
                                 ridge=None if ridge_grid is not None else m.fit_ridge)
            if k:
                m.set_readout(m.W_out)
            n += k
        return n

    def predict(self, U, frames_per_group, T=None, transient=0, precision="f32", noise_mode="counter", seed=0,
                group_offset=0, io="f64", out=None):
        """U [B, T_in, n_in] -> Y [K, B, T - transient, n_out]: K launches on the one U (it is not replicated), member
        k into slab k.  seed: one value or one per member.  io="f32" where ReservoirBank.predict allows it."""
        torch = self.torch
        io32 = io == "f32"
        U = _as_dev(U, torch, self.device, torch.float32 if io32 else None)
        if io32 and U.data_ptr() % 16:
            U = U.clone()
        seeds = self._per_member("seed", seed)
        b, t_in = U.shape[0], U.shape[1]
        T = t_in if T is None else int(T)
        shape = (self.n_members, b, T - int(transient), self.n_outputs)
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty(shape, dtype=torch.float32 if io32 else torch.float64, device=self.device)
            elif tuple(out.shape) != shape or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous {shape} tensor, not {tuple(out.shape)}")
        for k, m in enumerate(self.members):
            m.predict(U, frames_per_group, T=T, transient=transient, precision=precision, noise_mode=noise_mode,
                      seed=seeds[k], out=out[k], group_offset=group_offset, io=io)
        return out

    def detect_count(self, Y, tx_bits, p_i, frames_per_group, n_sub, n_t, bits_per_sym, err=None, bits=None,
                     weights=None, want_member_counts=False, want_xhat=False, member_err=None):
        """Y [K, B, N, 2 n_t] (float64, or float32 as predict(io="f32") writes it) -> per-group int64 (errors, bits) of
        the combination acc = w[g, 0] y_0, acc = acc + w[g, k] y_k (k = 1 .. K-1), accumulated into err / bits.
        weights: [G, K] float64 or None (1 / K each).  want_member_counts: also int64 [G, K], member k's own error
        count (accumulated into member_err when given).  Returns (err, bits[, member_err][, X_hat])."""
        torch = self.torch
        y32 = getattr(Y, "dtype", None) in (torch.float32, np.float32)
        Y = _as_dev(Y, torch, self.device, torch.float32 if y32 else None)
        if Y.ndim != 4 or Y.shape[2] != n_sub or Y.shape[3] != 2 * n_t:
            raise ValueError(f"Y must be [K, B, {n_sub}, {2 * n_t}], not {tuple(Y.shape)}")
        k, b = Y.shape[0], Y.shape[1]
        g = (b + frames_per_group - 1) // frames_per_group
        p_i = _as_dev(p_i, torch, self.device)
        tx_bits = _as_dev(tx_bits, torch, self.device, dtype=torch.uint8)
        weights = _as_dev(weights, torch, self.device)
        if weights is not None and tuple(weights.shape) != (g, k):
            raise ValueError(f"weights must be [{g}, {k}] (groups, members), not {tuple(weights.shape)}")
        with torch.cuda.device(self.device):
            if err is None:
                err = torch.zeros(g, dtype=torch.int64, device=self.device)
            if bits is None:
                bits = torch.zeros(g, dtype=torch.int64, device=self.device)
            if want_member_counts and member_err is None:
                member_err = torch.zeros((g, k), dtype=torch.int64, device=self.device)
            if member_err is not None and (tuple(member_err.shape) != (g, k) or not member_err.is_contiguous()):
                raise ValueError(f"member_err must be a contiguous [{g}, {k}] tensor")
            xh = torch.empty((b, n_sub, 2 * n_t), dtype=torch.float64, device=self.device) if want_xhat else None
            name = "esn_detect_count_ens_f32" if y32 else "esn_detect_count_ens"
            check(getattr(self.lib, name)(ptr(Y), k, b, int(frames_per_group), int(n_sub), int(n_t), int(bits_per_sym),
                                          ptr(p_i), ptr(weights), ptr(tx_bits), ptr(err), ptr(bits), ptr(member_err),
                                          ptr(xh), _lib.stream_handle()), name)
        return (err, bits) + ((member_err,) if want_member_counts else ()) + ((xh,) if want_xhat else ())
