"""Records SHA-256 digests of what the OFDM kernels write -- decide and re-modulate, the generic detector tail, the LS/MMSE
baseline, the channel tracker, taps to frequency, the frame generator and the LLRs -- over the smallest cases at which
their radix-2 stage loops, the QAM grid and the counter tail can go wrong, into tests/golden/ofdm_parent_digests.json,
for tests/test_gpu_ofdm_digests.py to compare against: these kernels share the arithmetic of csrc/esn_ofdm_math.h and
keep every output byte of the commit the file names.  None of them adds floating-point numbers atomically, so every
tensor is a function of the inputs alone.  Needs a GPU.

Run it with the library of the commit whose results are to be pinned (ESN_HIP_LIB selects another build), twice, and
compare the two files before trusting them:

    ESN_HIP_LIB=<that tree>/esn_ofdm_mimo_amd/libesn_hip.so python tools/record_ofdm_digests.py --commit <hash>

The sample.  N = 2 has one stage (unpaired only), 4 one pair, 8 a pair and the unpaired stage, 64 and 128 are the
benchmark's sizes with an even and an odd stage count; n_t in {1, 2, 3, 4}, n_r in {1, 2, 8}, 4-, 16- and 64-QAM; 2 to
9 frames (blocks, estimates) in groups with a ragged last one.  Each entry point keeps its own limits (mmse: n_t <= 4,
channel_estimate: N / n_t >= 2, channel_track: n_t isi <= min(64, N), cp < N), so the parent serves every case:
  remod      esn_detect_remod: D_hat, dec_bits, X_hat, err, bits; one case without tx_bits (no counters); one with
             N = 2048, n_t = 8, where the launcher splits the antennas over workgroups
  detect     esn_detect_count and _f32 at shapes the fixed instance does not serve (the generic kernel): err, bits, X_hat
  chanest    esn_channel_estimate, ls_only 0 and 1: H
  mmse, zf   esn_mmse_detect_count, esn_zf_detect_count: err, bits, X_hat
  track      esn_channel_track from X_hat and from bits, window 1 and 3: taps, H, status (0 in every case: the
             regulariser is positive)
  t2f        esn_taps_to_freq: H
  gen        esn_gen_frames and _c64, with supplied bits and noise and with the Philox streams, ls_pattern 0 and 1:
             bits, x_cp, y_cp
  llr        esn_qam_llr: llr, sigma2
Inputs come from NumPy generators seeded by (SEED, case index), so this tool and the test build the same arrays."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "ofdm_parent_digests.json")
SEED = 20261020


def cases():
    """The sample, a list of dicts: fn (family), id, and the family's sizes."""
    out = []
    # (N, n_t, m, B frames, F frames per group, cp, delay)
    det = [(2, 1, 2, 3, 2, 1, 0), (4, 2, 4, 5, 2, 3, 1), (8, 3, 6, 4, 3, 0, 2), (8, 4, 2, 2, 1, 2, 0),
           (64, 4, 4, 7, 3, 16, 3), (64, 2, 6, 9, 4, 5, 0), (128, 3, 4, 5, 2, 32, 2), (128, 1, 2, 4, 3, 9, 1),
           (128, 4, 6, 3, 2, 32, 0), (2048, 8, 4, 2, 1, 144, 1)]
    for n, nt, m, b, f, cp, delay in det:
        out.append(dict(fn="remod", N=n, n_t=nt, m=m, B=b, F=f, cp=cp, delay=delay, tx=True))
    out.append(dict(fn="remod", N=128, n_t=4, m=4, B=5, F=2, cp=32, delay=2, tx=True))
    out.append(dict(fn="remod", N=8, n_t=2, m=4, B=3, F=2, cp=2, delay=1, tx=False))
    for y32 in (False, True):
        for n, nt, m, b, f, _, _ in det:
            out.append(dict(fn="detect", N=n, n_t=nt, m=m, B=b, F=f, y32=y32))
    # (N, n_t, n_r, m, isi, cp, blocks)
    est = [(2, 1, 1, 2, 1, 1, 3), (4, 2, 2, 4, 2, 2, 2), (8, 4, 8, 6, 2, 3, 2), (64, 2, 8, 6, 5, 16, 3),
           (128, 4, 8, 4, 8, 32, 2), (128, 1, 2, 2, 3, 9, 4)]
    for n, nt, nr, m, isi, cp, g in est:
        for ls_only in (0, 1):
            out.append(dict(fn="chanest", N=n, n_t=nt, n_r=nr, m=m, isi=isi, cp=cp, G=g, ls_only=ls_only))
    # (N, n_t, n_r, m, cp, B, F)
    lin = [(2, 1, 1, 2, 1, 3, 2), (4, 2, 2, 4, 2, 5, 2), (8, 4, 8, 6, 3, 4, 3), (64, 2, 8, 6, 16, 9, 4),
           (128, 4, 8, 4, 32, 5, 2), (128, 1, 2, 2, 9, 3, 2)]
    for n, nt, nr, m, cp, b, f in lin:
        for zf in (0, 1):
            out.append(dict(fn="zf" if zf else "mmse", N=n, n_t=nt, n_r=nr, m=m, cp=cp, B=b, F=f))
    # (N, n_t, n_r, m, isi, cp, estimates, estimates per group)
    trk = [(2, 1, 1, 2, 2, 1, 3, 2), (4, 2, 2, 4, 2, 2, 4, 3), (8, 4, 8, 6, 2, 3, 2, 1), (64, 2, 8, 6, 5, 16, 3, 2),
           (128, 4, 8, 4, 8, 32, 2, 2), (128, 1, 2, 2, 16, 31, 4, 3)]
    for n, nt, nr, m, isi, cp, e, epg in trk:
        for src in ("xhat", "bits"):
            for window in (1, 3):
                out.append(dict(fn="track", N=n, n_t=nt, n_r=nr, m=m, isi=isi, cp=cp, E=e, EPG=epg, src=src, window=window))
    for n, nt, nr, isi, g in [(2, 1, 1, 2, 3), (8, 4, 8, 3, 2), (64, 2, 2, 5, 4), (128, 4, 8, 8, 3), (96, 3, 2, 7, 2)]:
        out.append(dict(fn="t2f", N=n, n_t=nt, n_r=nr, isi=isi, G=g))
    # (N, n_t, n_r, m, isi, cp, B, frames per block)
    gen = [(2, 1, 1, 2, 1, 1, 3, 2), (4, 2, 2, 4, 2, 2, 5, 2), (8, 4, 8, 6, 3, 3, 4, 3), (8, 4, 2, 4, 2, 2, 3, 2),
           (64, 2, 8, 6, 5, 16, 4, 3), (128, 4, 8, 4, 8, 32, 3, 2), (128, 1, 2, 2, 3, 9, 2, 1)]
    for c64 in (False, True):
        for n, nt, nr, m, isi, cp, b, f in gen:
            for given in (True, False):
                for ls in (0, 1):
                    out.append(dict(fn="gen", N=n, n_t=nt, n_r=nr, m=m, isi=isi, cp=cp, B=b, F=f, c64=c64, given=given, ls=ls))
    for n, nt, m, b in [(2, 1, 2, 3), (8, 3, 6, 2), (64, 2, 4, 4), (128, 4, 4, 3), (128, 4, 6, 2), (96, 2, 2, 2)]:
        out.append(dict(fn="llr", N=n, n_t=nt, m=m, B=b))
    for c in out:
        c["id"] = c["fn"] + "-" + "-".join(f"{k}{int(v) if isinstance(v, bool) else v}" for k, v in c.items() if k != "fn")
    assert len({c["id"] for c in out}) == len(out)
    return out


def _cplx(rs, *shape, scale=0.7):
    """complex128 [*shape] as float64 [*shape, 2]"""
    return rs.randn(*shape, 2) * scale


def run(i, c):
    """{output name: device tensor} of case i from the library that esn_ofdm_mimo_amd._lib has loaded"""
    import torch
    from esn_ofdm_mimo_amd import _lib
    lib, ptr, st = _lib.load(), _lib.ptr, _lib.stream_handle()
    rs = np.random.RandomState(SEED % (2 ** 31) + i)
    dev = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device="cuda")
    fn, N, n_t = c["fn"], c["N"], c["n_t"]
    m, n_r, cp = c.get("m"), c.get("n_r"), c.get("cp")
    res = None
    if fn in ("remod", "detect"):
        B, F = c["B"], c["F"]
        G = (B + F - 1) // F
        Y = rs.randn(B, N, 2 * n_t) * 0.7
        tx = dev(rs.randint(0, 2, (B, N * m, n_t)).astype(np.uint8))
        p_i = dev(0.5 + rs.rand(G))
        err, bits, xh = i64(G), i64(G), f64(B, N, n_t, 2)
        if fn == "detect":
            Yd = dev(Y.astype(np.float32) if c["y32"] else Y)
            f = lib.esn_detect_count_f32 if c["y32"] else lib.esn_detect_count
            rc = f(ptr(Yd), B, F, N, n_t, m, ptr(p_i), ptr(tx), ptr(err), ptr(bits), ptr(xh), st)
            res = dict(err=err, bits=bits, X_hat=xh)
        else:
            Yd = dev(Y)
            dec = torch.zeros((B, N * m, n_t), dtype=torch.uint8, device="cuda")
            dh = f64(B, c["delay"] + cp + N, n_t, 2)
            has = c["tx"]
            rc = lib.esn_detect_remod(ptr(Yd), B, F, N, cp, c["delay"], n_t, m, ptr(p_i), ptr(tx) if has else None,
                                      ptr(err) if has else None, ptr(bits) if has else None, ptr(xh), ptr(dec), ptr(dh), st)
            res = dict(D_hat=dh, dec_bits=dec, X_hat=xh, err=err, bits=bits)
    elif fn == "chanest":
        G, T = c["G"], N + cp
        y = dev(_cplx(rs, G, T, n_r))
        pb = dev(rs.randint(0, 2, (G, N * m, n_t)).astype(np.uint8))
        p_i = dev(0.5 + rs.rand(G))
        H = f64(G, N, n_r, n_t, 2)
        rc = lib.esn_channel_estimate(G, N, cp, n_t, n_r, c["isi"], m, ptr(p_i), 0.05, ptr(pb), ptr(y), c["ls_only"], ptr(H), st)
        res = dict(H=H)
    elif fn in ("mmse", "zf"):
        B, F, T = c["B"], c["F"], N + cp
        G = (B + F - 1) // F
        y = dev(_cplx(rs, B, T, n_r))
        H = dev(_cplx(rs, G, N, n_r, n_t))
        tx = dev(rs.randint(0, 2, (B, N * m, n_t)).astype(np.uint8))
        p_i = dev(0.5 + rs.rand(G))
        err, bits, xh = i64(G), i64(G), f64(B, N, n_t, 2)
        if fn == "zf":
            rc = lib.esn_zf_detect_count(B, F, N, cp, n_t, n_r, m, ptr(p_i), ptr(H), ptr(y), ptr(tx), ptr(err), ptr(bits), ptr(xh), st)
        else:
            rc = lib.esn_mmse_detect_count(B, F, N, cp, n_t, n_r, m, ptr(p_i), 0.05, ptr(H), ptr(y), ptr(tx), ptr(err), ptr(bits),
                                           ptr(xh), st)
        res = dict(err=err, bits=bits, X_hat=xh)
    elif fn == "track":
        E, EPG, W, L, T = c["E"], c["EPG"], c["window"], c["isi"], N + cp
        G = (E + EPG - 1) // EPG
        y = dev(_cplx(rs, E * W, T, n_r))
        xhat = dev(_cplx(rs, E * W, N, n_t))
        bt = dev(rs.randint(0, 2, (E * W, N * m, n_t)).astype(np.uint8))
        p_i, reg = dev(0.5 + rs.rand(G)), dev(0.5 + rs.rand(G, L))
        taps, H = f64(E, n_r, n_t, L, 2), f64(E, N, n_r, n_t, 2)
        status = torch.full((E,), -1, dtype=torch.int32, device="cuda")
        rc = lib.esn_channel_track(ptr(y), ptr(xhat) if c["src"] == "xhat" else None, ptr(bt) if c["src"] == "bits" else None,
                                   E, W, EPG, N, cp, n_t, n_r, L, m, ptr(p_i), ptr(reg), ptr(taps), ptr(H), ptr(status), st)
        res = dict(taps=taps, H=H, status=status)
    elif fn == "t2f":
        G = c["G"]
        taps = dev(_cplx(rs, G, n_r, n_t, c["isi"]))
        H = f64(G, N, n_r, n_t, 2)
        rc = lib.esn_taps_to_freq(G, N, n_t, n_r, c["isi"], ptr(taps), ptr(H), st)
        res = dict(H=H)
    elif fn == "gen":
        B, F, T, L = c["B"], c["F"], N + cp, c["isi"]
        G = (B + F - 1) // F
        taps = dev(_cplx(rs, G, n_r, n_t, L, scale=0.4))
        bits_in = dev(rs.randint(0, 2, (B, N * m, n_t)).astype(np.uint8))
        noise_in = dev(rs.randn(B, T, n_r, 2))
        p_i, a_clip = dev(0.5 + rs.rand(G)), dev(1.0 + rs.rand(G))
        if not c["given"]:
            bits_in = noise_in = None
        ft = torch.float32 if c["c64"] else torch.float64
        bits = torch.zeros((B, N * m, n_t), dtype=torch.uint8, device="cuda")
        x_cp = torch.zeros((B, T, n_t, 2), dtype=ft, device="cuda")
        y_cp = torch.zeros((B, T, n_r, 2), dtype=ft, device="cuda")
        f = lib.esn_gen_frames_c64 if c["c64"] else lib.esn_gen_frames
        rc = f(B, F, N, cp, n_t, n_r, L, m, c["ls"], ptr(p_i), ptr(a_clip), 0.05, ptr(taps), ptr(bits_in), ptr(noise_in),
               SEED + i, 1000 + i, ptr(bits), ptr(x_cp), ptr(y_cp), st)
        res = dict(bits=bits, x_cp=x_cp, y_cp=y_cp)
    elif fn == "llr":
        B = c["B"]
        xh = dev(_cplx(rs, B, N, n_t))
        llr, s2 = f64(B, n_t, N, m), f64(B)
        rc = lib.esn_qam_llr(B, N, n_t, m, ptr(xh), ptr(llr), ptr(s2), st)
        res = dict(llr=llr, sigma2=s2)
    _lib.check(rc, c["id"])
    torch.cuda.synchronize()
    if fn == "track":
        assert int(res["status"].abs().max()) == 0, f"{c['id']}: an estimate was flagged; the sample pins the served path"
    return res


def digests(i, c):
    """{output name: SHA-256 of its bytes} of case i"""
    return {k: hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest() for k, t in run(i, c).items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    from esn_ofdm_mimo_amd import _lib
    rows = [[c["id"], digests(i, c)] for i, c in enumerate(cases())]
    doc = {"commit": args.commit, "seed": SEED, "digests": rows}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(rows)} cases from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
