"""What the reference's Adam-trained comparators (fnn.py, cnn.py, lstm.py) share on the host: a bank of G models whose
parameters are a tuple of named arrays, trained per pilot by one esn_<model>_train launch and read by one
esn_<model>_predict launch, and the reference's model surface on NumPy sequences around such a bank.

    TrainedBank    the device bank: parameter sets and their checks, the workspace, train, predict
    TrainedModel   fit / predict of the reference's model classes, one sequence at a time

A comparator states its NAMES, the shapes of one set, the integers its entry points take, their names and its
train_shape_error; its init_weights stays beside it."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import PRECISIONS, check, ptr
from .bankbase import _as_dev
from .windowed import WindowedBank

_COUNT = {4: "four", 6: "six"}


class TrainedBank(WindowedBank):
    NAMES = ()                  # the arrays of one parameter set, in the order of the entry points' arguments
    ENTRY = None                # "cnn": esn_cnn_workspace_bytes, esn_cnn_train, esn_cnn_predict
    F16 = False                 # whether predict serves "f16"
    train_shape_error = None    # staticmethod(*_sizes(), T) -> None or the limit the shape misses
    loss = _work = None

    def __init__(self, n_inputs, n_outputs, n_hidden, window, n_groups=1, device=None):
        WindowedBank.__init__(self, n_inputs, n_outputs, n_hidden, window, device)
        self.n_groups = int(n_groups)
        self._hold([None] * len(self.NAMES))

    def _sizes(self):
        """The integers every entry point takes after `precision`."""
        raise NotImplementedError

    def _shapes(self, n):
        """The shapes of n parameter sets, in NAMES order."""
        raise NotImplementedError

    def _entry(self, what):
        return getattr(self.lib, f"esn_{self.ENTRY}_{what}")

    def _scalings(self):
        return [ptr(self.in_scale), ptr(self.in_shift), ptr(self.t_scale), ptr(self.t_shift)]

    def _sets(self, params):
        """The arrays of NAMES, one set or [n_sets, ...] -> contiguous device tensors [n_sets, ...]."""
        torch, names = self.torch, self.NAMES
        with torch.cuda.device(self.device):
            prm = [_as_dev(t, torch, self.device) for t in params]
        if len(prm) != len(names):
            raise ValueError(f"need the {_COUNT.get(len(names), len(names))} arrays {names}, got {len(prm)}")
        if prm[0].ndim == len(self._shapes(1)[0]) - 1:
            prm = [t[None] for t in prm]
        want = self._shapes(prm[0].shape[0])
        got = tuple(tuple(t.shape) for t in prm)
        if got != want:
            raise ValueError(f"{names} must have shapes {want}, not {got}")
        return [t.contiguous() for t in prm]

    def _hold(self, sets):
        for n, t in zip(self.NAMES, sets):
            setattr(self, n, t)

    def set_weights(self, *params):
        """Trained parameters in NAMES order, [G, ...] (or one set): what predict reads."""
        self._hold(self._sets(params))

    def _workspace_bytes(self, n_groups, n_frames, T):
        return self._entry("workspace_bytes")(*self._sizes(), n_groups, n_frames, T)

    def _workspace(self, n_groups, n_frames, T):
        """[pointer, bytes] of the device workspace of a training of n_groups or a prediction of n_frames (under the
        device guard)."""
        need = int(self._workspace_bytes(n_groups, n_frames, T))
        if self._work is None or self._work.numel() * 8 < need:
            self._work = None                                  # (release before growing)
            self._work = self.torch.empty(max(1, (need + 7) // 8), dtype=self.torch.float64, device=self.device)
        return [ptr(self._work), self._work.numel() * 8]

    def _shape_check(self, T, who):
        why = self.train_shape_error(*self._sizes(), T)
        if why:
            raise ValueError(f"{who} does not serve this shape: " + why)

    def train(self, U, D, init, transient=0, epochs=50, lr=0.01, betas=(0.9, 0.999), eps=1e-8, group_offset=0,
              want_loss=False):
        """U [G, T_in, n_in], D [G, T, n_out] (T_in <= T: zero rows are appended before scaling); init = the arrays of
        init_weights, one set or [n_isets, ...]: group g starts from set (group_offset + g) % n_isets.  The loss runs
        over rows [transient, T).  Sets the arrays of NAMES [G, ...] (and loss [G, epochs], the loss before each step, if
        want_loss); returns self."""
        torch = self.torch
        U, D = _as_dev(U, torch, self.device), _as_dev(D, torch, self.device)
        g, t_in, T = U.shape[0], U.shape[1], D.shape[1]
        if D.shape[0] != g or U.shape[2] != self.n_inputs or D.shape[2] != self.n_outputs or t_in > T:
            raise ValueError(f"U {tuple(U.shape)} and D {tuple(D.shape)} must be [G, T_in, {self.n_inputs}] and "
                             f"[G, T, {self.n_outputs}] with T_in <= T")
        who = f"esn_{self.ENTRY}_train"
        self._shape_check(T, who)
        init = self._sets(init)
        self._check_groups(g)
        with torch.cuda.device(self.device):
            kw = dict(dtype=torch.float64, device=self.device)
            out = [torch.empty(s, **kw) for s in self._shapes(g)]
            loss = torch.empty((g, int(epochs)), **kw) if want_loss else None
            work = self._workspace(g, 0, T)
            check(self._entry("train")(_lib.F64, *self._sizes(), init[0].shape[0], *[ptr(t) for t in init],
                                       *self._scalings(), ptr(U), ptr(D), g, t_in, T, int(transient), int(group_offset),
                                       int(epochs), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                       *[ptr(t) for t in out], ptr(loss), *work, _lib.stream_handle()), who)
        self._hold(out)
        self.loss = loss
        return self

    def predict(self, U, frames_per_group, T=None, transient=0, precision="f64", out=None):
        """U [B, T_in, n_in] (frames ordered by group) -> Y [B, T - transient, n_out] (device, unscaled); group g reads
        its own trained set.  precision "f64", and "f16" where the comparator has such an instance (F16)."""
        if precision != "f64" and not self.F16:
            raise ValueError(f"precision must be 'f64' ({type(self).__name__} has no fp16 prediction), not {precision!r}")
        first = self.NAMES[0]
        U, b, t_in, T, out = self._predict_args(U, frames_per_group, T, transient, precision, out, getattr(self, first),
                                                first + ": train (or set_weights) before predict",
                                                "the bank holds {} trained sets, batch needs {}")
        who = f"esn_{self.ENTRY}_predict"
        self._shape_check(T, who)
        with self.torch.cuda.device(self.device):
            work = self._workspace(0, b, T)
            check(self._entry("predict")(PRECISIONS[precision], *self._sizes(), *[ptr(getattr(self, n)) for n in self.NAMES],
                                         *self._scalings(), ptr(U), b, int(frames_per_group), t_in, T, int(transient),
                                         ptr(out), *work, _lib.stream_handle()), who)
        return out


class TrainedModel:
    """The reference's model classes with their training loop (system_model_2_all_comparision.py:102-113, :133-145) on
    the GPU: inputs [T, n_in] and targets [T, n_out] are NumPy sequences, float64.  A subclass sets its sizes, then calls
    this constructor with its initial parameters, and builds its bank in _make_bank."""
    NAMES = ()

    def __init__(self, init, epochs, lr):
        self.epochs, self.lr = int(epochs), float(lr)
        for n, t in zip(self.NAMES, init):
            setattr(self, n, np.asarray(t, dtype=np.float64))
        self.loss = None
        self._bank = None

    def _get_bank(self):
        if self._bank is None:
            self._bank = self._make_bank()
        return self._bank

    def _params(self):
        return tuple(getattr(self, n) for n in self.NAMES)

    def fit(self, inputs, targets):
        bank = self._get_bank()
        bank.train(np.asarray(inputs, dtype=np.float64)[None], np.asarray(targets, dtype=np.float64)[None],
                   self._params(), transient=0, epochs=self.epochs, lr=self.lr, want_loss=True)
        for n in self.NAMES:
            setattr(self, n, getattr(bank, n)[0].cpu().numpy())
        self.loss = bank.loss[0].cpu().numpy()

    def predict(self, inputs):
        bank = self._get_bank()
        bank.set_weights(*self._params())
        return bank.predict(np.asarray(inputs, dtype=np.float64)[None], 1).cpu().numpy()[0]
