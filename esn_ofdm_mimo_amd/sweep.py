"""The sweep of the Monte-Carlo harness (montecarlo.py tells the whole chain): draw_reservoir, the reference's host-side
draw, with reservoir_seed, host_reservoirs and host_reservoir_bank (the pool of a sweep or a point as a bank) and
fit_e_dtype, which the points of points.py share; blocks_for_rank and reduce_counters, the rank split and the path's one
collective; check_io and check_sweep_options, every refusal of DetectorSweep(...), made before the device is opened;
RadiusCache and ChunkLayout, two named parts of DetectorSweep, the SNR sweep over Monte-Carlo blocks.  torch comes from
_lib.require_gpu() or a local import: no GPU is needed to import."""
from __future__ import annotations

import numpy as np

from . import _lib
from . import reservoirs as _reservoirs
from .batched import ReservoirBank
from .frames import FrameSource, _view_real, pilot_rows
from .link import LinkParams
from .readout import _lambdas


def blocks_for_rank(rank, world_size, n_blocks):
    """Contiguous deal of coherence blocks to ranks: rank r owns blocks
    [r n / W, (r+1) n / W); the union over ranks is range(n_blocks).  A block's random streams, state
    noise and (per-block reservoirs) weight set depend on its GLOBAL index only -- never on the rank,
    the chunk or the launch it lands in -- so the summed counters are identical for any world size.
    (Contiguous ranges, so that a chunk of a rank's blocks is one run of global indices and one
    `group_offset` describes it to the kernels.)"""
    lo = (rank * n_blocks) // world_size
    hi = ((rank + 1) * n_blocks) // world_size
    return list(range(lo, hi))


def reduce_counters(counters, dist=None, world_size=1):
    """The path's only collective: one all_reduce(SUM) of the int64 [n_snr, 2] (errors, bits)
    tensor (RCCL over xGMI on GPUs, gloo on CPU).  Integer sums are order independent, so the
    result is bit-identical for any world size.  Runs whenever a process group is handed in (a
    one-rank group included); `dist=None` is the single-process path."""
    if dist is not None and (world_size > 1 or dist.is_initialized()):
        dist.all_reduce(counters, op=dist.ReduceOp.SUM)
    return counters


def draw_reservoir(n_in, n_out, n_res, spectral_radius, sparsity, seed):
    """(W, W_in, W_feedb) in the reference's draw order (pyESN.py:93-109), host-side init."""
    rs = np.random.RandomState(seed)
    w = rs.rand(n_res, n_res) - 0.5
    w[rs.rand(n_res, n_res) < sparsity] = 0
    w *= spectral_radius / np.max(np.abs(np.linalg.eigvals(w)))
    return w, rs.rand(n_res, n_in) * 2 - 1, rs.rand(n_res, n_out) * 2 - 1


def reservoir_seed(seed):
    """Seed of the first reservoir set of the sweep with seed `seed`: set i of a pool is drawn from reservoir_seed + i."""
    return seed * 7919 + 17


def host_reservoirs(n_in, n_out, n_res, spectral_radius, sparsity, seeds):
    """draw_reservoir of every seed, stacked: (W [S, n, n], W_in [S, n, n_in], W_feedb [S, n, n_out])."""
    ws = [draw_reservoir(n_in, n_out, n_res, spectral_radius, sparsity, s) for s in seeds]
    return tuple(np.stack([w[k] for w in ws]) for k in range(3))


def host_reservoir_bank(n_in, n_out, n_res, spectral_radius, sparsity, seeds, **bank_kw):
    """The teacher-forced ReservoirBank of the host draws of `seeds`, one weight set per seed."""
    return ReservoirBank(n_in, n_out, n_res, *host_reservoirs(n_in, n_out, n_res, spectral_radius, sparsity, seeds),
                         teacher_forcing=True, **bank_kw)


def fit_e_dtype(bank, method, fit_precision, rows, cols):
    """Element type of the extended states of a fit of [rows, cols] systems: float32 on the all-GPU fast path (fp16 / bf16
    harvest + Cholesky, asked for or what "auto" picks at this shape) -- the state columns are exactly representable, the
    fit is unchanged to ~1e-7 -- else float64."""
    chol = method == "chol" or (method == "auto" and bank.chol_fits(rows, cols))
    return "f32" if (chol and fit_precision in ("f16", "bf16")) else "f64"


def check_io(io, precision):
    if io not in ("f64", "f32"):
        raise ValueError(f"io must be 'f64' or 'f32', not {io!r}")
    if io == "f32" and precision == "f64":
        raise ValueError("io='f32' needs precision f32, f16 or bf16 (the float64 kernels read and write float64)")


def check_sweep_options(params, precision, solve_method, train_ebno, io, ridge, ridge_grid, radius, radius_precision,
                        track, track_window, n_pilots, track_forget):
    """What DetectorSweep refuses, from its options and the link alone: no device is touched."""
    check_io(io, precision)
    gram = solve_method == "gram"
    if not 0.0 <= float(track_forget) <= 1.0:
        raise ValueError(f"track_forget must lie in [0, 1], not {track_forget}")
    if track not in (None, "decisions", "genie"):
        raise ValueError(f"track must be None, 'decisions' or 'genie', not {track!r}")
    if track is not None:
        if int(track_window) < 1:
            raise ValueError(f"track_window must be at least 1 (the training sets a re-fit sees), not {track_window}")
        grid_refused = ridge_grid is not None and not (gram and int(n_pilots) >= 2)
        for name, given in (("ridge_grid", grid_refused), ("train_ebno", train_ebno is not None),
                            ("params.continuation", params.continuation), ("io='f32'", io == "f32")):
            if given:
                raise ValueError(f"track={track!r} does not go with {name}: the re-fits are plain pinv / ridge solves "
                                 "on float64 frames of the actual Eb/No, every frame from a fresh state")
    if int(n_pilots) != n_pilots or int(n_pilots) < 1:
        raise ValueError(f"n_pilots must be a whole number of at least 1, not {n_pilots!r}")
    if gram and ridge is None and ridge_grid is None:
        raise ValueError("solve_method='gram' needs ridge or ridge_grid: the normal equations of fewer rows than "
                         "columns have no pinv solution")
    if gram and ridge_grid is not None and int(n_pilots) == 1:
        raise ValueError("solve_method='gram' chooses among ridge_grid on a held-out pilot: it needs n_pilots >= 2")
    if gram and params.continuation:
        raise ValueError("solve_method='gram' does not go with params.continuation: every pilot is fitted from a zero "
                         "state and no training-final state is kept")
    if int(n_pilots) > 1:
        for name, given in (("track", track is not None and not gram), ("train_ebno", train_ebno is not None),
                            ("params.continuation", params.continuation)):
            if given:
                raise ValueError(f"n_pilots={n_pilots} does not go with {name}: several pilots are fitted once, at "
                                 "the actual Eb/No, each from a zero state")
    if ridge is not None and ridge_grid is not None:
        raise ValueError("give ridge or ridge_grid, not both")
    if int(n_pilots) > 1 and ridge_grid is not None and not 1 <= np.size(ridge_grid) <= ReservoirBank.HOLDOUT_MAX_GRID:
        raise ValueError(f"ridge_grid holds {np.size(ridge_grid)} candidates, the hold-out choice takes 1 to "
                         f"{ReservoirBank.HOLDOUT_MAX_GRID}")
    if radius not in ("host", "device"):
        raise ValueError(f"radius must be 'host' or 'device', not {radius!r}")
    if radius_precision not in _reservoirs.RADIUS_PRECISIONS:
        raise ValueError(f"radius_precision must be one of {sorted(_reservoirs.RADIUS_PRECISIONS)}, "
                         f"not {radius_precision!r}")


def stream_seed(seed, snr_idx, leg):
    """64-bit seed of the state-noise stream of one Eb/No point of the sweep with seed `seed`; leg 0 = training
    (harvest), 1 = detection.  With the kernels' global frame index this makes the noise a function of (seed, snr, leg,
    global frame, step, row) -- independent of chunking and world size.  Member k of an ensemble
    (points.ensemble_point) takes leg + (k << 24)."""
    h = (int(seed) * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) % (2 ** 64)
    for k in (snr_idx, leg):
        h = ((h ^ (h >> 31)) * 0xBF58476D1CE4E5B9 + int(k) + 1) % (2 ** 64)
    return h


class RadiusCache:
    """The spectral radii of one run() with reservoirs="fresh": radius float64 [n] and status int32 [n] on `device` for
    the n contiguous blocks from `base` on (a rank's own), and on the host which of them are filled, so that no
    decision here reads the device.  A chunk's values are kept slot by slot: block b of a chunk of n_blocks sits in
    slot b % n_blocks, the set the kernels pick for it."""

    def __init__(self, base, n, device):
        import torch
        self.torch, self.base = torch, base
        self.radius = torch.zeros(n, dtype=torch.float64, device=device)
        self.status = torch.ones(n, dtype=torch.int32, device=device)
        self.filled = np.zeros(n, dtype=bool)

    def _slots(self, first_block, n_blocks):
        """Cache index of the block in slot 0 .. n_blocks - 1, on the host and on the device; None for a chunk that
        starts before the base or runs past the end."""
        if first_block < self.base or first_block + n_blocks - self.base > len(self.filled):
            return None
        idx = first_block + (np.arange(n_blocks) - first_block) % n_blocks - self.base
        return idx, self.torch.as_tensor(idx, dtype=self.torch.int64, device=self.radius.device)

    def lookup(self, first_block, n_blocks):
        """(radius, status) of a chunk, slot by slot, when every one of its blocks has been stored; else None."""
        slots = self._slots(first_block, n_blocks)
        if slots is None or not self.filled[slots[0]].all():
            return None
        return self.radius[slots[1]], self.status[slots[1]]

    def store(self, first_block, n_blocks, radius, status):
        slots = self._slots(first_block, n_blocks)
        if slots is not None:
            self.radius[slots[1]] = radius
            self.status[slots[1]] = status
            self.filled[slots[0]] = True


class ChunkLayout:
    """What one chunk hands to run(): ONE int64 device vector -- errors, bits, flagged fits, then how many blocks took
    each of the n_choices ridge candidates, then (errors, bits) of each of the n_symbols data symbols of a block.
    `pack` writes that order and the slices read it."""

    def __init__(self, n_choices, n_symbols):
        self.totals, self.flagged = slice(0, 2), 2
        self.choices = slice(3, 3 + n_choices)
        self.symbols = slice(3 + n_choices, 3 + n_choices + 2 * n_symbols)
        self.size = self.symbols.stop

    @staticmethod
    def pack(torch, errors, bits, flagged, choices=None, symbols=None):
        """choices [n_choices] or None; symbols [n_symbols, 2] or None."""
        parts = [torch.stack([errors, bits, flagged])]
        if choices is not None:
            parts.append(choices)
        if symbols is not None:
            parts.append(symbols.reshape(-1))
        return torch.cat(parts)


class DetectorSweep:
    """SNR sweep x Monte-Carlo blocks, sharded over ranks by block."""

    def __init__(self, params: LinkParams, n_reservoir=512, spectral_radius=0.9, sparsity=0.1, noise=0.001,
                 seed=0, precision="f32", fit_precision="f64", reservoirs="shared", pool=8, device=None,
                 rank=0, world_size=1, solve_method="auto", train_ebno=None, io="f64", ridge=None, ridge_grid=None,
                 radius="host", radius_precision="f64", radius_squarings=24, fresh_radius_cache=True,
                 symbol_counts=False, track=None, track_window=2, n_pilots=1, track_forget=1.0):
        """reservoirs: "shared" (one reservoir for every block), "per_block" (block b uses set b % pool of a pool
        drawn here) or "fresh" (the reference's own rule, SURVEY F5: every coherence block gets a reservoir of its
        own, drawn on the device by reservoirs.generate and keyed by (seed, global block index) -- the same at every
        Eb/No point, as the pool is, and the same for any chunking and world size; each chunk draws its blocks'
        reservoirs and swaps them into the bank before it trains).  With "fresh" the default chunk of run() is also
        bounded by memory: 2 GiB for the float64 W, the two squaring images and the packed weights of a chunk, counted
        as 40 n_reservoir^2 bytes per block (about 200 blocks at n_reservoir = 512); see default_chunk_blocks.

        radius: "host" (default: draw_reservoir, np.linalg.eigvals per set, bit for bit what it always was) or
        "device" for the "shared" and "per_block" modes: the same RandomState uniforms, drawn on the host in the same
        order, are scaled by the device's spectral radius (reservoirs.generate(uniforms=...)) -- W within 1e-6 of the
        host's, without pool x eigvals in this constructor (8.8 s per set at n_reservoir = 2048).

        radius_precision, radius_squarings: how the device measures a radius, for reservoirs="fresh" and for
        radius="device" -- "f64" (default) or "f16x2" (reservoirs.RADIUS_PRECISIONS: split fp16 operands, within 1e-6
        of "f64"), and the number of squarings.

        fresh_radius_cache ("fresh" only): a block's reservoir is keyed by (seed, global block), so its radius is the
        same at every Eb/No point of a run(); the first point's radius and status stay on the device (12 bytes per
        block of this rank) and the later points scale with them instead of measuring again -- the same bits, so the
        same counters.  fresh_radius_hits counts the blocks of the last run() that were served this way.

        ridge (extension; None = the reference's pinv fit): lambda of the ridge read-out (ReservoirBank.solve), a
        float or a callable ebno_db -> float (the best lambda moves with Eb/No and n_reservoir).

        ridge_grid (extension): a sequence of L candidates; every block takes the one with the smallest
        leave-one-out score of its own pilot (ReservoirBank.solve(ridge_grid=)), no data frame touched.  After run(),
        ridge_choice_counts is {ebno: int64 [L]}: how many of this rank's blocks took each candidate (summed on the
        device, read once per Eb/No point).

        symbol_counts (extension): the detector tail counts every data frame on its own (one frame per group, Pi
        expanded) and the counts are summed on the device by position in the block; after run(),
        symbol_error_counts is {ebno: int64 [F, 2]} = (errors, bits) of data symbol 0 .. F - 1 over this rank's blocks,
        read once per Eb/No point.  The block totals, so the returned BER and counters, are the same integers either
        way.  With params.fading == "jakes" (FrameSource.blocks_fast) this is BER against the age of the pilot.

        track (extension; None = every read-out is fitted once, on the pilot): "decisions" or "genie" re-fits the
        read-out after every data symbol of a block (_chunk_tracked).  Data symbol k of all blocks of a chunk is predicted
        with the current read-outs and detected; "decisions" turns the detector's own decisions back into the teacher
        signal on the device (ReservoirBank.detect_remod), "genie" takes the generator's transmit signal of that frame
        (the bound: what a receiver that decided without error would have); the frame is harvested against that teacher
        and the read-out solved again over the most recent track_window training sets (the pilot is one, and drops out
        once track_window data symbols have been seen), with the sweep's solve_method and ridge.  Symbol k detects under
        stream_seed(si, 2 + 2 k) and re-trains under stream_seed(si, 3 + 2 k), keyed by the global block, so the
        counters do not depend on chunking or world size.  Read it with symbol_counts=True.  Not with ridge_grid,
        train_ebno, params.continuation or io="f32".  keep_track_xhat = True (an attribute, for tests and tools) makes
        every chunk leave its X_hat [F, G, N, 2 n_t] in track_xhat.

        io="f32": data frames complex64 and predict / detect with float32 I/O (same counters as "f64": the
        predict kernels see the same float inputs and write the same float outputs).  Pilots and training stay
        float64.  Needs precision f32 / f16 / bf16.

        n_pilots (extension; 1 = the reference's one pilot per block, today's path bit for bit): every block sends P
        pilot symbols (FrameSource.blocks_fast(n_pilots=P)) and its read-out is fitted on all of them, each harvested
        from a zero state, rows stacked into one solve (ReservoirBank.fit_pilots).  Pilot 0 trains under
        stream_seed(si, 0) as ever, pilot p >= 1 under stream_seed(si, PILOT_LEG0 + p).  ridge, ridge_grid,
        solve_method, fit_precision, reservoirs and io work as with one pilot; with P >= 2 ridge_grid is chosen on the
        held-out last pilot instead of by leave-one-out, for any stacked shape (pinv degrades as the stacked rows
        approach the number of columns -- 4 pilots of 128 rows against 528 columns -- so give ridge or ridge_grid).
        Not with track, train_ebno or params.continuation (ValueError): tracking and fixed-Eb/No training see one
        pilot, and no pilot's final state is "the" training-final state.

        solve_method="gram" (extension; needs ridge or ridge_grid): the read-out is kept as running normal equations
        (ReservoirBank.fit_pilots(method="gram"), gram_accumulate, gram_solve), whose size does not depend on the number
        of pilots or symbols seen.  Without track: any n_pilots on the device path, ridge_grid (chosen on the held-out
        last pilot) from n_pilots = 2.  With track: allowed together with n_pilots >= 1 and, from n_pilots = 2, with
        ridge_grid -- the hold-out choice is made once, at the pilot fit, and each block keeps its lambda for every
        re-fit.  After data symbol k the frame is harvested, accumulated into the block's state with decay
        track_forget (in [0, 1], default 1.0: nothing is forgotten; 0: every re-fit sees the newest symbol alone) and the
        read-out solved again at the block's lambda; track_window is not read in this mode.  A flagged re-fit keeps the
        block's previous read-out (a device-side select, no host read) and adds to the chunk's flagged count; no rows
        are kept, so nothing is repaired by QR and fits_repaired then counts fits that stayed flagged.  Stream seeds,
        state-noise legs and keys are those of the other solve methods.  train_ebno, params.continuation and io="f32"
        stay refused with track, and so does ridge_grid with one pilot; params.continuation is refused in this mode at
        any n_pilots (every pilot is fitted from a zero state: no training-final state exists)."""
        check_sweep_options(params, precision, solve_method, train_ebno, io, ridge, ridge_grid, radius, radius_precision,
                            track, track_window, n_pilots, track_forget)
        self.io, self.track_forget = io, float(track_forget)
        self.track, self.track_window, self.n_pilots = track, int(track_window), int(n_pilots)
        self.keep_track_xhat, self.track_xhat = False, None
        torch = _lib.require_gpu()
        self.torch, self.p = torch, params
        self.rank, self.world = rank, world_size
        self.precision, self.fit_precision = precision, fit_precision
        self.solve_method, self.ridge = solve_method, ridge
        self.ridge_grid = None if ridge_grid is None else np.array(ridge_grid, dtype=np.float64).reshape(-1)
        self.ridge_choice_counts = {}
        self.symbol_counts, self.symbol_error_counts = bool(symbol_counts), {}
        self.train_ebno = train_ebno      # not None: every ESN is trained at this fixed Eb/No
        self.n_in, self.n_out, self.n_res = 2 * params.n_r, 2 * params.n_t, n_reservoir
        self.seed, self.reservoir_seed = seed, reservoir_seed(seed)
        self.src = FrameSource(params, device, seed)
        self.device = self.src.device
        # the candidates on the device, copied once: [L]
        self._grid_t = None if ridge_grid is None else _lambdas(torch, self.device, self.ridge_grid, 1, grid=True)[0][0]
        self._ebno = self._train_bufs = self._fit_io = self._cont = None     # set_snr / train leave these
        self.radius_precision, self.radius_squarings = radius_precision, int(radius_squarings)
        self.fresh_radius_cache, self.fresh_radius_hits, self._radius_cache = bool(fresh_radius_cache), 0, None
        self.reservoirs = reservoirs
        self._res_args = (self.n_in, self.n_out, int(n_reservoir), float(spectral_radius), float(sparsity))
        self.bank = self._make_bank(pool, radius, noise)

    @property
    def n_sets(self):
        """Weight sets in the bank: 1, the pool, or under "fresh" the blocks of the last chunk."""
        return self.bank.n_wsets

    @property
    def fit_io(self):
        """(U, D, transient) of the last train(): what ReservoirBank.solve needs to fit the same pilots again."""
        return self._fit_io

    def _make_bank(self, pool, radius, noise):
        """The bank of the constructor: "fresh" holds block 0's reservoir until the first chunk swaps its own in;
        "shared" / "per_block" hold 1 / `pool` sets, set i drawn from reservoir_seed + i on the host or, with
        radius="device", from the same uniforms scaled on the device."""
        n_in, n_out, n = self._res_args[:3]
        kw = dict(teacher_forcing=True, noise=noise, device=self.device)
        if self.reservoirs == "fresh":
            return ReservoirBank.generate(*self._res_args, seed=self.reservoir_seed, first_set=0, n_sets=1,
                                          radius_precision=self.radius_precision, n_squarings=self.radius_squarings, **kw)
        seeds = [self.reservoir_seed + i for i in range(1 if self.reservoirs == "shared" else int(pool))]
        if radius == "host":
            return host_reservoir_bank(*self._res_args, seeds, noise=noise, device=self.device)
        sets = [self._device_scaled(s) for s in seeds]
        bank = ReservoirBank(n_in, n_out, n, np.zeros((n, n)), np.zeros((n, n_in)), np.zeros((n, n_out)), **kw)
        bank.set_weights(*(self.torch.cat([w[k] for w in sets]) for k in range(3)))
        return bank

    def _device_scaled(self, seed):
        """radius="device": the uniforms draw_reservoir(seed) consumes, in its order, scaled on the device."""
        n_in, n_out, n, rho, sparsity = self._res_args
        rs = np.random.RandomState(seed)
        u = np.concatenate([rs.rand(n, n).ravel(), rs.rand(n, n).ravel(), rs.rand(n, n_in).ravel(),
                            rs.rand(n, n_out).ravel()])
        return _reservoirs.generate(n_in, n_out, n, rho, sparsity, 0, uniforms=u[None], device=self.device,
                                    radius_precision=self.radius_precision, n_squarings=self.radius_squarings)[:3]

    # "fresh": bytes per block of a chunk -- float64 W (8 n^2), two squaring images (16 n^2, padded to 64) and the packed
    # weights of the fit and the detect precision (at most 8 n^2 each) -- and the budget they are held to
    FRESH_BYTES_PER_BLOCK_N2, FRESH_BUDGET_BYTES = 40, 2 << 30

    def _swap_in_fresh(self, first_block, n_blocks, check):
        """The reservoirs of global blocks [first_block, first_block + n_blocks) into the bank: block b in slot
        b % n_blocks, which is the set the kernels pick for it under group_offset = first_block.  Returns the int32
        status [n_blocks] on the device; `check` reads it on the host and raises for a set that could not be scaled."""
        cache = self._radius_cache
        known = None if cache is None else cache.lookup(first_block, n_blocks)
        W, W_in, W_fb, radius, status = _reservoirs.generate(*self._res_args, seed=self.reservoir_seed,
                                                             first_set=first_block, n_sets=n_blocks, device=self.device,
                                                             check_status=check, n_squarings=self.radius_squarings,
                                                             radius_precision=self.radius_precision,
                                                             radius=None if known is None else known[0],
                                                             radius_status=None if known is None else known[1])
        if known is not None:
            self.fresh_radius_hits += n_blocks
        elif cache is not None:
            cache.store(first_block, n_blocks, radius, status)
        self.bank.set_weights(W, W_in, W_fb)
        return status

    def _require_block_fading(self, who):
        if self.p.fading != "block":
            raise ValueError(f"{who} generates block-fading frames only (one tap set per block): params.fading is "
                             f"{self.p.fading!r}; BER against the symbol index is DetectorSweep(symbol_counts=True).run")

    def _require_block_independent_bank(self, who):
        if self.reservoirs == "fresh":
            raise ValueError(f"{who} trains through the bank as it stands, which under reservoirs='fresh' holds one "
                             "block's reservoir only: build the sweep with reservoirs='shared' or 'per_block'")

    def set_snr(self, ebno_db, n_groups, scale_ebno=None):
        """Scalings and Pi of n_groups blocks at this Eb/No.  scale_ebno: the input scaling is that of another Eb/No --
        an ESN trained at a fixed Eb/No keeps that scaling at train AND detect time
        (OFDM_MIMO_2-2_NBF_LDPC.py:347-367,440-448)."""
        torch, p = self.torch, self.p
        ones_in = torch.ones((n_groups, self.n_in), dtype=torch.float64, device=self.device)
        ones_out = torch.ones((n_groups, self.n_out), dtype=torch.float64, device=self.device)
        self.bank.set_scaling(ones_in * p.input_scaling(ebno_db if scale_ebno is None else scale_ebno), None,
                              ones_out * p.teacher_scale, None)
        self.p_i = self.src.p_i(ebno_db, n_groups)
        self._ebno = ebno_db

    def ridge_at(self, ebno_db):
        """lambda of the fits at this Eb/No (None: pinv)."""
        if self.ridge is None:
            return None
        return float(self.ridge(ebno_db)) if callable(self.ridge) else float(self.ridge)

    def stream_seed(self, snr_idx, leg):
        """stream_seed (the module's function) of this sweep's seed."""
        return stream_seed(self.seed, snr_idx, leg)

    def train(self, pilot_y, pilot_x, seed=0, group_offset=0):
        """helper_mimo_esn_generic.py:58-86 for G blocks: delay d, nForget = d + CP, one harvest + solve.
        group_offset = global index of the first block (noise key and weight set follow the global block)."""
        p, d = self.p, self.p.delay
        g, t = pilot_y.shape[0], pilot_y.shape[1]
        # zero-padded pilot buffers are kept between calls of the same shape (the padding rows are never written)
        kept = self._train_bufs
        fits = kept is not None and kept[0].shape == (g, t + d, self.n_in)
        U, D = self._train_bufs = pilot_rows(pilot_y, pilot_x, d, out=kept if fits else None)
        self._fit_io = (U, D, p.forget)
        e_dtype = self._fit_e_dtype = fit_e_dtype(self.bank, self.solve_method, self.fit_precision, t + d - p.forget,
                                                  self.bank.n_reservoir + self.n_in)
        E = self.bank.fit(U, D, transient=p.forget, precision=self.fit_precision, noise_mode="counter",
                          seed=seed, method=self.solve_method, e_dtype=e_dtype, group_offset=group_offset,
                          ridge=self.ridge_at(self._ebno), ridge_grid=self._grid_t)
        self._cont = None
        if p.continuation:      # laststate / lastoutput of pyESN.py:195-197: training-final state, scaled teacher
            y_last = D[:, -1, :]
            if self.bank.t_scale is not None:
                y_last = y_last * self.bank.t_scale[:g]
            if self.bank.t_shift is not None:
                y_last = y_last + self.bank.t_shift[:g]
            self._cont = (E[:, -1, :self.bank.n_reservoir].double().contiguous(), y_last.contiguous())
        return E

    PILOT_LEG0 = 1 << 20        # stream_seed leg of pilot p >= 1 is PILOT_LEG0 + p: beyond every leg of a tracked block

    def train_pilots(self, pilots_y, pilots_x, snr_idx=0, group_offset=0):
        """train for P pilots per block: pilots_y [G, P, T, n_r], pilots_x [G, P, T, n_t] (blocks_fast(n_pilots=P)),
        through ReservoirBank.fit_pilots.  Returns the stacked extended states [G, P rows, cols]; fit_io becomes
        (None, the stacked teacher, 0), which is what repair_fit needs."""
        p, d = self.p, self.p.delay
        P, t = pilots_y.shape[1:3]
        U, D = pilot_rows(pilots_y, pilots_x, d)
        gram = self.solve_method == "gram"          # (the accumulate kernel reads float32 states as the Cholesky ones do)
        e_dtype = self._fit_e_dtype = fit_e_dtype(self.bank, "chol" if gram else self.solve_method, self.fit_precision,
                                                  P * (t + d - p.forget), self.bank.n_reservoir + self.n_in)
        seeds = [self.stream_seed(snr_idx, 0)] + [self.stream_seed(snr_idx, self.PILOT_LEG0 + q) for q in range(1, P)]
        E = self.bank.fit_pilots(U, D, transient=p.forget, precision=self.fit_precision, noise_mode="counter",
                                 seed=seeds, method=self.solve_method, e_dtype=e_dtype, group_offset=group_offset,
                                 ridge=self.ridge_at(self._ebno), ridge_grid=self._grid_t)
        self._fit_io = (None, None if gram else self.bank.fit_rows[1], 0)       # ("gram" keeps no rows)
        self._cont = None
        return E

    def repair_fit(self, E):
        """Host-synchronising check of the last fit: groups the Cholesky path flagged are re-solved
        with the QR kernel (GPU).  Returns how many were."""
        U, D, tr = self._fit_io
        n = self.bank.resolve_failed(E, D, tr, self.bank.W_out, self.bank.fit_status, ridge_grid=self._grid_t,
                                     ridge=None if self._grid_t is not None else self.bank.fit_ridge)
        if n:
            self.bank.set_readout(self.bank.W_out)
        return n

    def detect(self, data_y, data_bits, frames_per_block, err, bits, seed=0, out=None, group_offset=0,
               per_frame=False):
        """driver:433-456 for all data frames of G blocks: predict (d trailing zero rows synthesised
        in-kernel) -> fused FFT/slicer/count.  per_frame: err / bits are [G F], one counter per data frame (the tail
        runs with one frame per group and Pi expanded) instead of [G]."""
        p = self.p
        U = _view_real(data_y)
        x0, y0 = self._cont if (p.continuation and self._cont) else (None, None)
        y = self.bank.predict(U, frames_per_block, T=p.t_frame + p.delay, transient=p.forget, x0=x0, y0=y0,
                              precision=self.precision, noise_mode="counter", seed=seed, out=out,
                              group_offset=group_offset, io=self.io)
        if per_frame:
            self.bank.detect_count(y, data_bits, self.p_i.repeat_interleave(frames_per_block), 1, p.n_sub, p.n_t, p.m,
                                   err=err, bits=bits)
        else:
            self.bank.detect_count(y, data_bits, self.p_i, frames_per_block, p.n_sub, p.n_t, p.m, err=err, bits=bits)
        return y

    def default_chunk_blocks(self, frames_per_block):
        """Blocks per launch that fill the chip with whole rounds of workgroup tiles: about five tiles per CU
        (the benchmark's choice), i.e. 5 * CUs * tile_frames slots at ceil16(F) slots per block."""
        info = _lib.device_info()
        tile = self.bank.tile_frames(self.precision)
        fpad = ((frames_per_block + 15) // 16) * 16
        chunk = max(1, (5 * info["cu_count"] * tile) // fpad)
        if self.reservoirs == "fresh":      # one reservoir per block lives on the device for the length of a chunk
            chunk = min(chunk, max(1, self.FRESH_BUDGET_BYTES // (self.FRESH_BYTES_PER_BLOCK_N2 * self.n_res ** 2)))
        if self.solve_method == "gram":     # a block's G, C and the factor of its solve live for the length of a chunk
            cols = self.n_res + self.n_in
            per_block = 8 * (cols * cols + self.n_out * cols + ((cols + 15) // 16 * 16) ** 2)
            chunk = min(chunk, max(1, self.GRAM_BUDGET_BYTES // per_block))
        return chunk

    # solve_method="gram": state (8 cols^2 + 8 n_out cols bytes) plus solve workspace (8 ceil16(cols)^2) per block of a
    # chunk -- 4.5 MB at 528 columns -- are held to this budget (about 950 blocks there), whatever the candidates
    GRAM_BUDGET_BYTES = 4 << 30

    def _flagged_fits(self, unscaled, repair):
        """How many fits of the chunk just trained cannot be trusted, an int64 scalar on the device: the groups the
        Cholesky solve flagged, the harvest clusters that timed out and (`unscaled`: their int32 status, or None) the
        fresh reservoirs that could not be scaled.  Any of them has run() redo the chunk with `repair`, whose host
        reads deal with each -- repair_fit re-solves, reservoirs.generate raises, and here a timed-out harvest
        raises -- so that pass tallies zero."""
        torch = self.torch
        if repair:
            self.bank.raise_if_harvest_timed_out()
            return torch.zeros((), dtype=torch.int64, device=self.device)
        flagged = self.bank.fit_status.ne(0).sum().to(torch.int64)
        for more in (self.bank.harvest_timeout, unscaled):
            if more is not None:
                flagged = flagged + more.ne(0).sum().to(torch.int64)
        return flagged

    def _chunk(self, ebno, si, ids, F, repair=False):
        """One launch group: generate, train, detect the contiguous global blocks `ids`; returns the chunk's int64
        device vector (ChunkLayout) without synchronising the host unless `repair`."""
        torch = self.torch
        g = len(ids)
        data = self.src.blocks_fast(ebno, si, ids[0], g, F, io="c64" if self.io == "f32" else "c128",
                                    want_data_x=self.track == "genie", n_pilots=self.n_pilots)
        self.set_snr(ebno, g, scale_ebno=self.train_ebno)
        unscaled = None
        if self.reservoirs == "fresh":      # (no host read unless `repair`: an unscalable set counts as a flagged fit)
            unscaled = self._swap_in_fresh(ids[0], g, check=repair)
        if self.train_ebno is not None:
            # the "train@fixed Eb/No" ESN of the block-fading drivers (OFDM_MIMO_2-2_NBF_LDPC.py:181-183,347-367):
            # pilot generated at the training Eb/No over the SAME taps, evaluated on the data frames of the actual
            # Eb/No (:440-448)
            _, px, py = self.src.frames(data["taps"], 1, self.train_ebno, si, ids[0], 0, want_x=True)
            data["pilot_y"], data["pilot_x"] = py, px
        gram = self.solve_method == "gram"
        if gram and self.n_pilots == 1:     # (one pilot goes the same way: fit_pilots(method="gram") takes any P)
            E = self.train_pilots(data["pilot_y"][:, None], data["pilot_x"][:, None], snr_idx=si, group_offset=ids[0])
        elif self.n_pilots > 1:
            E = self.train_pilots(data["pilots_y"], data["pilots_x"], snr_idx=si, group_offset=ids[0])
        else:
            E = self.train(data["pilot_y"], data["pilot_x"], seed=self.stream_seed(si, 0), group_offset=ids[0])
        picks = None
        if self.ridge_grid is not None:     # (before a repair: a block without a choice is in no bin)
            ch = self.bank.last_ridge_choice
            picks = torch.bincount(ch.clamp(min=0).long(), weights=ch.ge(0).double(),
                                   minlength=len(self.ridge_grid)).to(torch.int64)
        if repair and not gram:             # ("gram" keeps no rows to solve again: a flagged fit stays flagged)
            self.repair_fit(E)
        if self.track is not None:
            tracked = self._chunk_tracked_gram if gram else self._chunk_tracked
            err, nb, flagged = tracked(ebno, si, ids, F, data, E, self._flagged_fits(unscaled, repair), repair)
            per_symbol = torch.stack([err.sum(dim=1), nb.sum(dim=1)], dim=1) if self.symbol_counts else None
            return ChunkLayout.pack(torch, err.sum(), nb.sum(), flagged, picks, per_symbol)
        n_cnt = g * F if self.symbol_counts else g
        err = torch.zeros(n_cnt, dtype=torch.int64, device=self.device)
        nb = torch.zeros(n_cnt, dtype=torch.int64, device=self.device)
        self.detect(data["data_y"], data["data_bits"], F, err, nb, seed=self.stream_seed(si, 1), group_offset=ids[0],
                    per_frame=self.symbol_counts)
        per_symbol = None
        if self.symbol_counts:
            per_symbol = torch.stack([err.view(g, F).sum(dim=0), nb.view(g, F).sum(dim=0)], dim=1)
        return ChunkLayout.pack(torch, err.sum(), nb.sum(), self._flagged_fits(unscaled, repair), picks, per_symbol)

    def _track_symbols(self, ebno, si, ids, F, data, flagged, repair, refit):
        """The per-symbol loop both tracked modes share: for k = 0 .. F - 1 predict and detect symbol k of every block
        with the current read-outs and, unless it is the last, harvest it against the teacher (the re-modulated
        decisions, or for "genie" the transmit signal) and hand the states to `refit(Ek, D_hat, flagged) -> flagged`,
        which solves the read-outs again and swaps them in.  Symbol k detects under stream_seed(si, 2 + 2 k) and
        re-trains under stream_seed(si, 3 + 2 k).  Returns (err [F, G], bits [F, G], flagged); `repair` raises for a
        harvest that timed out instead of counting it."""
        torch, p, bank = self.torch, self.p, self.bank
        g, d, T, forget = len(ids), p.delay, p.t_frame, p.forget
        y_sym = _view_real(data["data_y"]).view(g, F, T, self.n_in)
        bits_sym = data["data_bits"].view(g, F, p.n_sub * p.m, p.n_t)
        x_sym = _view_real(data["data_x"]).view(g, F, T, self.n_out) if self.track == "genie" else None
        err = torch.zeros((F, g), dtype=torch.int64, device=self.device)
        nb = torch.zeros((F, g), dtype=torch.int64, device=self.device)
        U = torch.zeros((g, T + d, self.n_in), dtype=torch.float64, device=self.device)       # d trailing zero rows
        D_true = torch.zeros((g, T + d, self.n_out), dtype=torch.float64, device=self.device) if x_sym is not None else None
        xhats = []
        for k in range(F):
            y = bank.predict(y_sym[:, k], 1, T=T + d, transient=forget, precision=self.precision, noise_mode="counter",
                             seed=self.stream_seed(si, 2 + 2 * k), group_offset=ids[0])
            out = bank.detect_remod(y, bits_sym[:, k].contiguous(), self.p_i, 1, p.n_sub, p.cp, d, p.n_t, p.m,
                                    err=err[k], bits=nb[k], want_xhat=self.keep_track_xhat)
            D_hat = out[0]
            if self.keep_track_xhat:
                xhats.append(out[3])
            if k == F - 1:
                break
            U[:, :T] = y_sym[:, k]
            if x_sym is not None:
                D_true[:, d:d + T] = x_sym[:, k]
                D_hat = D_true.clone()              # (a window of training sets keeps it beyond this symbol)
            Ek = bank.harvest(U, D_hat, precision=self.fit_precision, noise_mode="counter",
                              seed=self.stream_seed(si, 3 + 2 * k), e_dtype=self._fit_e_dtype, group_offset=ids[0])
            if repair:
                bank.raise_if_harvest_timed_out()
            elif bank.harvest_timeout is not None:
                flagged = flagged + bank.harvest_timeout.ne(0).sum().to(torch.int64)
            flagged = refit(Ek, D_hat, flagged)
        if self.keep_track_xhat:
            self.track_xhat = torch.stack(xhats)
        return err, nb, flagged

    def _chunk_tracked(self, ebno, si, ids, F, data, E, flagged, repair):
        """The data symbols of a chunk under `track`, after the pilot fit (E: its extended states; `flagged`: its
        flagged-fit count), through _track_symbols: every re-fit solves over the window of the most recent training
        sets.  Returns (err [F, G], bits [F, G], flagged + the flagged re-fits); `repair` re-solves flagged re-fits by QR
        on the spot (host reads)."""
        torch, bank = self.torch, self.bank
        U0, D0, forget = self._fit_io
        window = [(E[:, forget:], D0[:, forget:].clone())]        # (the pilot buffers are reused by the next chunk)
        ridge = self.ridge_at(ebno)

        def refit(Ek, D_hat, flagged):
            window[:] = (window + [(Ek[:, forget:], D_hat[:, forget:])])[-self.track_window:]
            E_w, D_w = (torch.cat([w[i] for w in window], dim=1) for i in (0, 1))
            W_out, status = bank.solve(E_w, D_w, 0, method=self.solve_method, ridge=ridge)
            if repair:
                bank.resolve_failed(E_w, D_w, 0, W_out, status, ridge=ridge)
            else:
                flagged = flagged + status.ne(0).sum().to(torch.int64)
            bank.set_readout(W_out)
            return flagged

        return self._track_symbols(ebno, si, ids, F, data, flagged, repair, refit)

    def _chunk_tracked_gram(self, ebno, si, ids, F, data, state, flagged, repair):
        """_chunk_tracked for solve_method="gram": `state` is the GramState the pilot fit left.  Every re-fit accumulates
        the symbol's states into it with decay track_forget and solves at the block's own lambda (the ridge of the
        sweep, or the hold-out choice of the pilot fit); a flagged re-fit keeps the block's previous read-out and is
        counted."""
        torch, bank, forget = self.torch, self.bank, self.p.forget
        # (a block without a hold-out choice carries NaN: its re-fits answer status 2 and its zero read-out stays)
        lam = bank.fit_ridge if self.ridge_grid is not None else self.ridge_at(ebno)

        def refit(Ek, D_hat, flagged):
            bank.gram_accumulate(Ek, D_hat, forget, state, self.track_forget)
            W_new, status = bank.gram_solve(state, lam)
            bad = status.ne(0)
            bank.set_readout(torch.where(bad[:, None, None], bank.W_out, W_new))
            return flagged + bad.sum().to(torch.int64)

        return self._track_symbols(ebno, si, ids, F, data, flagged, repair, refit)

    def run(self, ebno_list, blocks_per_snr, frames_per_block=None, chunk_blocks=None, dist=None):
        """Returns (BER[n_snr], counters [n_snr, 2]) -- identical on every rank and for every world size and
        chunking (contiguous block ranges per rank; every stream keyed by global indices).  No host
        synchronisation inside an Eb/No point: the Cholesky status flags (and, with reservoirs="fresh", the flags of
        reservoirs whose radius could not be measured) are summed on the device and read once per point; a chunk with
        a flagged fit (none on any run so far) is redone with the QR repair, and that pass raises EsnHipError for an
        unscalable fresh reservoir."""
        torch = self.torch
        F = frames_per_block or self.p.coherence_symbols
        chunk = int(chunk_blocks or self.default_chunk_blocks(F))
        lay = ChunkLayout(0 if self.ridge_grid is None else len(self.ridge_grid), F if self.symbol_counts else 0)
        n_snr = len(ebno_list)
        counters = torch.zeros((n_snr, 2), dtype=torch.int64, device=self.device)
        mine = blocks_for_rank(self.rank, self.world, blocks_per_snr)
        self.fits_repaired = self.fresh_radius_hits = 0
        cached = self.reservoirs == "fresh" and self.fresh_radius_cache and len(mine)
        self._radius_cache = RadiusCache(mine[0], len(mine), self.device) if cached else None
        for si, ebno in enumerate(ebno_list):
            chunks = [mine[c0:c0 + chunk] for c0 in range(0, len(mine), chunk)]
            if not chunks:
                continue
            res = torch.stack([self._chunk(ebno, si, ids, F) for ids in chunks])   # [n_chunks, lay.size]
            if int(res[:, lay.flagged].sum().item()):                   # the point's one host read
                for ci in torch.nonzero(res[:, lay.flagged]).flatten().tolist():
                    self.fits_repaired += int(res[ci, lay.flagged].item())
                    res[ci] = self._chunk(ebno, si, chunks[ci], F, repair=True)
            counters[si] += res[:, lay.totals].sum(dim=0)
            if self.ridge_grid is not None:
                self.ridge_choice_counts[ebno] = res[:, lay.choices].sum(dim=0).cpu().numpy()
            if self.symbol_counts:
                self.symbol_error_counts[ebno] = res[:, lay.symbols].sum(dim=0).view(F, 2).cpu().numpy()
        self._radius_cache = None           # (a run()'s own: nothing outside it is served from the cache)
        reduce_counters(counters, dist, self.world)
        c = counters.cpu().numpy()
        return c[:, 0] / np.maximum(c[:, 1], 1), c
