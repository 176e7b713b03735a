"""NumPy emulation of the split-operand spectral radius (include/esn_hip.h, esn_spectral_radius_split_batch): a helper
of the split-radius tests, not a test.  The recurrence is specrad_ref.specrad's; every squaring is three float16
products accumulated in float32:

    X = s B  (s a power of two fixed by n alone; |B| <= 1, so s |b_ij| <= s stays inside float16)
    hi = fp16(X), lo = fp16((X - hi) 2^11)
    X X ~ hi hi + 2^-11 (hi lo + lo hi)

As the kernel does it, an image holds s B_k un-normalised by its own norm f_k (B_k = A_{k-1} A_{k-1}); 1 / f_k^2
multiplies the NEXT product, and the norms are taken in float64 from the float32 values before they are split.  The
float32 sums here run in BLAS's order, the kernel's in the matrix pipe's: the two agree to rounding, not bitwise."""
import numpy as np

TILE = 64
LO_SCALE = 2048.0                               # 2^11: the bits one float16 piece holds


def scale(n):
    """s = 2^(ceil(log2 padded n) - 2), the padded n a multiple of 64."""
    npad = (int(n) + TILE - 1) // TILE * TILE
    return 2.0 ** (int(np.ceil(np.log2(npad))) - 2)


def split(x32, with_lo=True):
    hi = x32.astype(np.float16)
    if not with_lo:
        return hi, None
    lo = ((x32 - hi.astype(np.float32)) * np.float32(LO_SCALE)).astype(np.float16)
    return hi, lo


def square(hi, lo):
    """float32 hi hi + 2^-11 (hi lo + lo hi); the cross terms share one accumulator."""
    h = hi.astype(np.float32)
    p = h @ h
    if lo is not None:
        l = lo.astype(np.float32)
        p = p + np.float32(1.0 / LO_SCALE) * (h @ l + l @ h)
    return p


def _usable(f):
    return bool(f > 0.0 and np.isfinite(f))


def specrad_split(W, n_squarings=24, with_lo=True):
    """(radius, status): status 1 and radius 0.0 when some f_k is zero or not finite.  with_lo=False drops the second
    piece (what a single float16 operand would give)."""
    w = np.array(W, dtype=np.float64)
    s = scale(w.shape[0])
    with np.errstate(all="ignore"):
        f = float(np.sqrt(np.sum(w * w)))
        if not _usable(f):
            return 0.0, 1
        l_prev = np.log(f)                                          # l_0
        hi, lo = split((w * (s / f)).astype(np.float32), with_lo)   # s A_0
        n2 = 1.0                                                    # |A_0|^2 by construction
        for k in range(1, n_squarings + 1):
            c = 1.0 / (s * n2)
            if not _usable(c):
                return 0.0, 1
            x = (square(hi, lo).astype(np.float64) * c).astype(np.float32)      # s B_k
            b = x.astype(np.float64) / s
            n2 = float(np.sum(b * b))
            f = float(np.sqrt(n2))
            if not _usable(f):
                return 0.0, 1
            if k == n_squarings:
                r = float(np.exp((l_prev + np.log(f)) / 2.0 ** (n_squarings - 1)))
                return (r, 0) if _usable(r) else (0.0, 1)
            l_prev = 2.0 * l_prev + np.log(f)                       # l_k
            hi, lo = split(x, with_lo)
    raise ValueError("n_squarings must be at least 1")
