#!/usr/bin/env python3
"""Generate tests/golden/chan_metrics.npz by RUNNING THE REFERENCE'S OWN STATEMENTS.

Runs only where the reference checkout exists (the build container), on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_chan_metrics_golden.py

The channel record of the block-fading drivers (mean capacity per subcarrier, fraction of full-rank subcarriers, median and
90th percentile of the condition number) is computed by OFDM_MIMO_2-2_NBF_LDPC.py:369-385 per coherence block and
aggregated per Eb/No by :515-521.  The script runs a whole sweep at import, so -- as make_golden.py does for the driver
loops -- the file is `ast`-parsed and exactly those statement nodes are compiled, unchanged, and executed with `H_true`,
`Pi`, `No`, `N`, `N_t`, `N_r`, `jj` and the accumulators supplied through the namespace.  `np` in that namespace is numpy
behind a shim that records what `np.linalg.svd` returned (the statements drop S after use).  `H_true` is built as :279
builds it, `np.fft.fft` of the zero-padded taps; the fixture stores the TAPS, not H.

Stored per case `c` (names in `cases`): c_taps [G, n_r, n_t, isi], c_ebno [E], c_p_i [E] (the reference's Pi), c_S
[G, N, min(n_t, n_r)], c_conds [G, N], and per Eb/No index e: c_e{e}_ranks [G, N], c_e{e}_cap_k [G, N], c_e{e}_agg =
(capacity_bits_per_sc, frac_rank_ge_full, cond_p50, cond_p90), c_e{e}_margin = min |S^2 / thr - 1|.

Rank is a threshold decision that the tests compare exactly, so every stored margin must be >= 1e-6: a draw that fails is
redrawn from the next seed (the seed used is stored), never masked.  A singular value that is exactly or nearly zero (the
rank-deficient hand-made matrices) has S^2 / thr ~ 0, a margin of 1.
"""
import ast
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle.ofdm_frames import LinkConfig, exp_pdp_taps  # noqa: E402

DRIVER = "/root/reference/system_model_2/OFDM_MIMO_2-2_NBF_LDPC.py"
BLOCK_LINES = (369, 385)     # "# Metrics from true H" .. rank_list.extend(ranks)
AGG_LINE = 515               # if len(cap_acc) > 0: ... Cond_p90[jj] = ...
N_SUB = 128
NO = 1e-5
MIN_MARGIN = 1e-6


def reference_statements():
    """(per-block statements :369-385, per-Eb/No aggregation statement :515-521) as two compiled modules."""
    tree = ast.parse(open(DRIVER).read(), filename=DRIVER)
    block = agg = None
    for node in ast.walk(tree):
        body = getattr(node, "body", None)
        if not isinstance(body, list):
            continue
        inside = [s for s in body if isinstance(s, ast.stmt) and BLOCK_LINES[0] <= s.lineno and s.end_lineno <= BLOCK_LINES[1]]
        if inside and ast.unparse(inside[0]) == "ranks = []" and inside[-1].end_lineno == BLOCK_LINES[1]:
            block = inside
        for s in body:
            if isinstance(s, ast.If) and s.lineno == AGG_LINE and ast.unparse(s.test) == "len(cap_acc) > 0":
                agg = s
    assert block is not None and agg is not None, "the reference's metric statements moved"
    assert ast.unparse(block[-1]) == "rank_list.extend(ranks)" and agg.end_lineno == 521
    assert "np.linalg.svd(Hk, full_matrices=False)" in ast.unparse(block[4])
    mk = lambda stmts: compile(ast.fix_missing_locations(ast.Module(body=stmts, type_ignores=[])), DRIVER, "exec")
    return mk(block), mk([agg])


class _Linalg:
    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        return getattr(np.linalg, name)

    def svd(self, *a, **kw):
        out = np.linalg.svd(*a, **kw)
        self._log.append(np.array(out[1]))
        return out


class _Numpy:
    """numpy, with linalg.svd recording the singular values it returned."""

    def __init__(self, log):
        self.linalg = _Linalg(log)

    def __getattr__(self, name):
        return getattr(np, name)


def h_true(taps):
    """:273-279 for one block: taps [n_r, n_t, isi] -> H_true [N, n_r, n_t]."""
    n_r, n_t, _ = taps.shape
    H = np.zeros((N_SUB, n_r, n_t), dtype=complex)
    for nr in range(n_r):
        for nt in range(n_t):
            c0 = taps[nr, nt]
            H[:, nr, nt] = np.fft.fft(np.r_[c0, np.zeros(N_SUB - len(c0))])
    return H


def run_case(code, taps, ebno):
    """The reference's statements over the blocks of `taps` at every Eb/No of `ebno`."""
    block_code, agg_code = code
    G, n_r, n_t, _ = taps.shape
    EbNoDB = np.array(ebno)
    Ptotal = 10 ** (EbNoDB / 10) * NO * N_SUB          # :146
    Pi = Ptotal / N_SUB                                 # :154
    out = dict(taps=taps, ebno=EbNoDB, p_i=Pi)
    for jj in range(len(ebno)):
        svals = []
        ns = dict(np=_Numpy(svals), H_true=None, Pi=Pi, No=NO, N=N_SUB, N_t=n_t, N_r=n_r, jj=jj,
                  cap_acc=[], cond_list=[], rank_list=[], min=min, max=max, len=len, float=float, range=range,
                  Capacity_bits_per_sc=np.zeros(len(ebno)), Frac_rank_ge_full=np.zeros(len(ebno)),
                  Cond_p50=np.zeros(len(ebno)), Cond_p90=np.zeros(len(ebno)))
        ranks, cap_k, conds = [], [], []
        for g in range(G):
            ns["H_true"] = h_true(taps[g])
            exec(block_code, ns)
            ranks.append(np.array(ns["ranks"])); cap_k.append(np.array(ns["cap_k"])); conds.append(np.array(ns["conds"]))
        exec(agg_code, ns)
        S = np.array(svals).reshape(G, N_SUB, min(n_t, n_r))
        thr = np.maximum(1e-2 * S[..., :1] ** 2, 10 * (NO / Pi[jj]))
        margin = float(np.abs(S ** 2 / thr - 1).min())
        if jj == 0:
            out["S"], out["conds"] = S, np.array(conds)
        assert np.array_equal(out["S"], S) and np.array_equal(out["conds"], np.array(conds))
        assert len(ns["rank_list"]) == G * N_SUB and len(ns["cap_acc"]) == G
        out[f"e{jj}_ranks"] = np.array(ranks).astype(np.uint8)
        out[f"e{jj}_cap_k"] = np.array(cap_k)
        out[f"e{jj}_agg"] = np.array([ns["Capacity_bits_per_sc"][jj], ns["Frac_rank_ge_full"][jj],
                                     ns["Cond_p50"][jj], ns["Cond_p90"][jj]])
        out[f"e{jj}_margin"] = margin
    return out


def margins(case):
    return [case[k] for k in case if k.endswith("_margin")]


def draw(n_t, n_r, n_blocks, seed):
    cfg = LinkConfig(n_t=n_t, n_r=n_r, n_sub=N_SUB)
    rs = np.random.RandomState(seed)
    return np.stack([exp_pdp_taps(cfg, rs) for _ in range(n_blocks)])


def main():
    code = reference_statements()
    cases = {}

    def add(name, make_taps, ebno, seed=None):
        """make_taps(seed) -> taps; redraw from the next seed while a rank decision sits within 1e-6 of its threshold."""
        for s in range(seed or 0, (seed or 0) + 50):
            c = run_case(code, make_taps(s), ebno)
            if min(margins(c)) >= MIN_MARGIN:
                break
            assert seed is not None, f"{name}: margin {min(margins(c)):.2e} and nothing to redraw"
        else:
            raise AssertionError(name)
        c["seed"] = s
        cases[name] = c
        print(f"{name:14s} seed {s}  taps {c['taps'].shape}  smallest margin {min(margins(c)):.2e}")

    for name, n_t, n_r, g in (("siso", 1, 1, 3), ("simo12", 1, 2, 3), ("mimo22", 2, 2, 3), ("mimo48", 4, 8, 2),
                              ("nr2_nt4", 4, 2, 3)):
        add(name, lambda s, a=(n_t, n_r, g): draw(*a, 1000 + s), [0, 12, 24], seed=0)
    loop = np.load(os.path.join(HERE, "loop_nbf.npz"))
    add("loop_nbf", lambda s: np.stack([loop["p0_b0_taps"], loop["p1_b0_taps"], loop["p1_b1_taps"]]),
        [int(e) for e in loop["ebno_db"]])
    base = draw(4, 8, 1, 77)

    def dup(t):
        t = t.copy(); t[:, :, 2] = t[:, :, 0]; return t

    def zcol(t):
        t = t.copy(); t[:, :, 1] = 0; return t

    for name, t in (("zeros", np.zeros_like(base)), ("dup_columns", dup(base)), ("zero_column", zcol(base)),
                    ("scaled_1e-13", base * 1e-13), ("scaled_1e8", base * 1e8)):
        add(name, lambda s, t=t: t, [12])
    # the 1e-12 clamp of :381 is active in the scaled-down case, and only there among the full-rank ones
    assert (cases["scaled_1e-13"]["S"][..., -1] < 1e-12).all() and (cases["mimo48"]["S"][..., -1] > 1e-12).all()
    flat = dict(cases=np.array(sorted(cases)), n_sub=N_SUB, no=NO)
    for name, c in cases.items():
        for k, v in c.items():
            flat[f"{name}_{k}"] = v
    path = os.path.join(HERE, "chan_metrics.npz")
    np.savez_compressed(path, **flat)
    print(f"chan_metrics.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
