"""LinkParams: the constants of a driver configuration (Demo_MIMO_4x8_Sionna_CDL_ESN_v2.py:182-238, :285-288) and what
follows from them -- delay, transient, frame length, coherence time, and the Eb/No-dependent power, clip level and
input scaling.  No GPU, no torch."""
from __future__ import annotations

import math
from dataclasses import dataclass


@dataclass
class LinkParams:
    n_t: int = 4
    n_r: int = 8
    n_sub: int = 128
    m: int = 4
    isi: int = 8
    fs: float = 2 * 1.024e6
    no: float = 1e-5
    clip_db: float = 3.0
    ds_ns: float = 300.0
    input_scaler: float = 0.005
    teacher_scale: float = 5e-7
    min_delay: int = 0
    f_d: float = 100.0
    channel: str = "tdlb"         # "tdlb" | "exp" | "awgn"
    # driver variants (defaults = the north-star 4x8 driver: d = (Min+Max)//2, nForget = d + CP, fresh state)
    delay_fixed: int = -1         # >= 0: output delay d of the trainer (the SISO driver trains without delay)
    forget_fixed: int = -1        # >= 0: rows dropped from the fit and from every prediction
    continuation: bool = False    # True: every predict starts from the training-final state / teacher output
    coherence_fixed: int = 0      # > 0: data symbols per pilot instead of the Doppler formula
    # "block": one tap set per coherence block (the reference).  "jakes" (extension): the taps move from OFDM symbol to
    # OFDM symbol with Doppler f_d (esn_gen_taps_doppler): the pilot sees symbol 0, data frame k symbol k + 1
    fading: str = "block"

    def __post_init__(self):
        if self.fading not in ("block", "jakes"):
            raise ValueError(f"fading must be 'block' or 'jakes', not {self.fading!r}")
        if self.fading == "jakes" and self.channel == "awgn":
            raise ValueError("fading='jakes' needs a multipath channel ('tdlb' or 'exp'): the flat 'awgn' channel of "
                             "the SISO driver has no Doppler mode")

    @classmethod
    def siso_awgn(cls, n_sub=512, symbols_per_pilot=400):
        """Demo_SISO_QPSK_AWGN_LDPC_ESN_with_ZF_LS.py: 1x1, QPSK, N=512, CP=0 (:107-111), flat unit-modulus
        channel drawn once per Eb/No point (:203-206), `esn.fit(Ein, Eout)` with transient 0 and no output
        delay (:224-226), `esn.predict(ESN_input)` = continuation=True (:253-254), 400 symbols per pilot."""
        return cls(n_t=1, n_r=1, n_sub=n_sub, m=2, isi=1, channel="awgn", delay_fixed=0, forget_fixed=0,
                   continuation=True, coherence_fixed=symbols_per_pilot)

    @classmethod
    def block_fading(cls, n_t=2, n_r=2, n_sub=512):
        """OFDM_{SISO,SIMO_1-2,MIMO_2-2}_NBF_LDPC.py / Demo_MIMO_4x8_ChannelRank_..._fast.py: exponential-PDP
        Rayleigh taps exp(-k/(CP/9)) redrawn every coherence block (:162-164,:272-279), 16-QAM, same trainer
        as the 4x8 driver (delay (0+6)//2 = 3, nForget = 10)."""
        return cls(n_t=n_t, n_r=n_r, n_sub=n_sub, m=4, isi=8, channel="exp")

    @property
    def cp(self):
        return self.isi - 1

    @property
    def max_delay(self):
        return int(math.ceil(self.isi / 2) + 2)

    @property
    def delay(self):
        return self.delay_fixed if self.delay_fixed >= 0 else (self.min_delay + self.max_delay) // 2

    @property
    def forget(self):
        return self.forget_fixed if self.forget_fixed >= 0 else self.delay + self.cp

    @property
    def t_frame(self):
        return self.n_sub + self.cp

    @property
    def coherence_symbols(self):
        if self.coherence_fixed > 0:
            return self.coherence_fixed
        t_sym = (self.n_sub + self.isi - 1) / self.fs
        return max(1, math.floor((0.5 / max(self.f_d, 1e-9)) / t_sym))

    @property
    def fd_tsym(self):
        """Doppler frequency x OFDM symbol time, in cycles per symbol."""
        return self.f_d * (self.n_sub + self.cp) / self.fs

    def p_i(self, ebno_db):
        return (10 ** (ebno_db / 10)) * self.no

    def var_x(self, ebno_db):
        return (10 ** (ebno_db / 10)) * self.no * self.n_sub

    def a_clip(self, ebno_db):
        return math.sqrt(self.var_x(ebno_db)) * 10 ** (self.clip_db / 20)

    def input_scaling(self, ebno_db):
        return self.input_scaler / math.sqrt(self.var_x(ebno_db))
