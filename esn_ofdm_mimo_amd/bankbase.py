"""What every device bank is built from, whatever it computes (ReservoirBank, elm.ElmBank, fnn.FnnBank):

    DeviceBank     the open device (torch, lib, device), the four per-group scalings and the scratch buffers
    DetectorTail   reconstruct / FFT / slicer / error count on a DeviceBank   (Demo_MIMO_4x8_..._v2.py:47-58,439-456)

torch is used for device memory and streams only."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check, ptr


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


class DeviceBank:
    """The one home of the scalings: every kernel call of a bank reads in_scale / in_shift / t_scale / t_shift here."""
    in_scale = in_shift = t_scale = t_shift = None

    def __init__(self, device=None):
        torch = _lib.require_gpu()
        self.torch = torch
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())

    def set_scaling(self, in_scale=None, in_shift=None, t_scale=None, t_shift=None):
        """Per-group scalings, each [G, n] (or None = identity): pyESN.py:127-152."""
        torch = self.torch
        self.in_scale = _as_dev(in_scale, torch, self.device)
        self.in_shift = _as_dev(in_shift, torch, self.device)
        self.t_scale = _as_dev(t_scale, torch, self.device)
        self.t_shift = _as_dev(t_shift, torch, self.device)

    def _check_groups(self, g):
        for name in ("in_scale", "in_shift", "t_scale", "t_shift"):
            t = getattr(self, name)
            if t is not None and t.shape[0] < g:
                raise ValueError(f"{name} holds {t.shape[0]} groups, batch has {g}")

    def _scratch(self, name, nbytes):
        """The bank's device scratch `name`, grown on demand to nbytes (None for 0).  Called under the device guard."""
        if not nbytes:
            return None
        ws = getattr(self, name, None)
        if ws is None or ws.numel() < nbytes:
            ws = self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.device)
            setattr(self, name, ws)
        return ws


class DetectorTail:
    """The detector tail of a DeviceBank: it reads torch, lib and device, nothing else."""

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

    def detect_llr(self, Y, tx_bits, p_i, frames_per_group, n_sub, n_t, bits_per_sym, weights=None, bias=None,
                   err=None, bits=None, want_xhat=False):
        """detect_count and, in the same launch, the soft outputs of its X_hat (esn_detect_llr; a float32 Y goes to
        esn_detect_llr_f32): the frame's decision-directed sigma2 [B] and llr [B, n_t, N m] = weights (d1 - d0)(X_hat /
        bias) / sigma2 in the decoder's layout, weights / bias float64 [G, N, n_t] (FrameSource.mmse_sinr) or None = 1:
        what LdpcCode.llrs gives on that X_hat, which never goes to memory unless want_xhat.  tx_bits None: nothing is
        counted.  Returns (err, bits, llr, sigma2[, X_hat]); err / bits are None without tx_bits."""
        torch = self.torch
        y32 = getattr(Y, "dtype", None) in (torch.float32, np.float32)
        Y = _as_dev(Y, torch, self.device, torch.float32 if y32 else None)
        b, fpg = Y.shape[0], int(frames_per_group)
        if fpg < 1:
            raise ValueError(f"frames_per_group = {frames_per_group} must be positive")
        g = (b + fpg - 1) // fpg
        p_i = _as_dev(p_i, torch, self.device)
        tx_bits = _as_dev(tx_bits, torch, self.device, dtype=torch.uint8)
        for name, t in (("weights", weights), ("bias", bias)):     # as LdpcCode.llrs: float64 as given, never cast
            if t is not None and (getattr(t, "dtype", None) not in (torch.float64, np.float64) or len(t.shape) != 3
                                  or tuple(t.shape[1:]) != (n_sub, n_t) or t.shape[0] < g):
                raise ValueError(f"{name} must be float64 [G >= {g}, {n_sub}, {n_t}], not "
                                 f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        weights, bias = _as_dev(weights, torch, self.device), _as_dev(bias, torch, self.device)
        with torch.cuda.device(self.device):
            if tx_bits is not None:
                if err is None:
                    err = torch.zeros(g, dtype=torch.int64, device=self.device)
                if bits is None:
                    bits = torch.zeros(g, dtype=torch.int64, device=self.device)
            else:
                err = bits = None
            xh = torch.empty((b, n_sub, 2 * n_t), dtype=torch.float64, device=self.device) if want_xhat else None
            llr = torch.empty((b, n_t, n_sub * int(bits_per_sym)), dtype=torch.float64, device=self.device)
            s2 = torch.empty(b, dtype=torch.float64, device=self.device)
            name = "esn_detect_llr_f32" if y32 else "esn_detect_llr"
            check(getattr(self.lib, name)(ptr(Y), b, fpg, int(n_sub), int(n_t), int(bits_per_sym), ptr(p_i), ptr(tx_bits),
                                          ptr(err), ptr(bits), ptr(weights), ptr(bias), ptr(llr), ptr(s2), ptr(xh),
                                          _lib.stream_handle()), name)
        return (err, bits, llr, s2) + ((xh,) if want_xhat else ())

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
