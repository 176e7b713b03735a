"""esn_mmse_equalize_rows on the device against its NumPy restatement (tests/equalize_ref.py) on device-generated frames:
the rows, X_hat bit for bit that of esn_mmse_detect_count, every output element written, the float32 rows, and a frame's
independence of the rest of the launch."""
import numpy as np
import pytest

import equalize_ref as qr

pytestmark = pytest.mark.gpu

EBNO = 15.0
# (N, cp, n_t, n_r, pad, groups, frames per group); the last: the largest n_r the LDS formula serves at N = 2048
SHAPES = [(8, 2, 2, 2, 0, 2, 2), (16, 7, 4, 8, 3, 2, 3), (128, 7, 4, 8, 0, 2, 3), (4, 0, 1, 1, 1, 1, 1),
          (2048, 7, 2, 4, 0, 1, 2)]
_cases = {}


def _case(shape):
    """Frames of the HIP generator under the true channel of their taps, the kernel's outputs and the restatement's,
    made once per shape."""
    if shape in _cases:
        return _cases[shape]
    from esn_ofdm_mimo_amd.montecarlo import FrameSource, LinkParams
    n, cp, n_t, n_r, pad, G, F = shape
    src = FrameSource(LinkParams(n_t=n_t, n_r=n_r, n_sub=n, isi=cp + 1), seed=n + n_r)
    taps = src.taps(G, 0, 0)
    bits, _, y = src.frames(taps, F, EBNO, 0, 0, 1)
    H = src.true_channel(taps)
    rows, xh = src.equalize_rows(H, y, F, EBNO, pad=pad, want_xhat=True)
    p_i = np.full(G, src.p.p_i(EBNO))
    X_ref, rows_ref = qr.equalize(y.cpu().numpy(), H.cpu().numpy(), p_i, src.p.no, cp, pad, F)
    c = dict(src=src, bits=bits, y=y, H=H, rows=rows, xh=xh, X_ref=X_ref, rows_ref=rows_ref, p_i=p_i)
    _cases[shape] = c
    return c


def _launch(src, H, y, frames_per_group, pad, out, xh=None):
    """The entry point on caller-owned outputs (FrameSource.equalize_rows allocates its own)."""
    import torch
    from esn_ofdm_mimo_amd import _lib
    p = src.p
    g = H.shape[0]
    p_i = torch.full((g,), p.p_i(EBNO), dtype=torch.float64, device=src.device)
    name = "esn_mmse_equalize_rows_f32" if out.dtype == torch.float32 else "esn_mmse_equalize_rows"
    _lib.check(getattr(src.lib, name)(y.shape[0], frames_per_group, p.n_sub, p.cp, pad, p.n_t, p.n_r, _lib.ptr(p_i), p.no,
                                      _lib.ptr(H), _lib.ptr(y), _lib.ptr(out), _lib.ptr(xh), _lib.stream_handle()), name)
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", SHAPES)
def test_rows_match_the_restatement_and_xhat_is_the_detectors(shape):
    """Rows within 1e-9 of the frame's largest |z|, the bound tests/test_gpu_baseline.py holds X_hat to (measured on an
    MI355X: 3.5e-16 at N = 4 to 1.6e-15 at N = 8, 1.4e-15 at N = 2048 -- the inverse transform needs no more); X_hat bitwise
    that of esn_mmse_detect_count."""
    import torch
    n, cp, n_t, n_r, pad, G, F = shape
    c = _case(shape)
    rows = c["rows"].cpu().numpy()
    assert rows.shape == (G * F, cp + n + pad, 2 * n_t) == c["rows_ref"].shape
    worst = 0.0
    for f in range(G * F):
        scale = np.max(np.hypot(c["rows_ref"][f, :, 0::2], c["rows_ref"][f, :, 1::2]))
        err = np.max(np.abs(rows[f] - c["rows_ref"][f])) / scale
        worst = max(worst, err)
        assert err < 1e-9, (f, err)
    xh = c["xh"].cpu().numpy()
    xerr = np.max(np.abs(xh - c["X_ref"])) / np.max(np.abs(c["X_ref"]))
    print(shape, "rows", worst, "X_hat against the restatement", xerr)
    assert xerr < 1e-9
    _, _, x_det = c["src"].mmse_detect_count(c["H"], c["y"], c["bits"], F, EBNO, want_xhat=True)
    assert torch.equal(torch.view_as_real(x_det), torch.view_as_real(c["xh"]))
    assert np.array_equal(rows[:, :cp], rows[:, n:n + cp])


@pytest.mark.parametrize("shape", SHAPES)
def test_every_element_is_written_pad_rows_are_zero_and_f32_rows_are_the_f64_rows_rounded(shape):
    import torch
    n, cp, n_t, n_r, pad, G, F = shape
    c = _case(shape)
    src = c["src"]
    pad = pad + 2                                             # (a pad where the shape has none, two rows more elsewhere)
    out = torch.full((G * F, cp + n + pad, 2 * n_t), float("nan"), dtype=torch.float64, device=src.device)
    xh = torch.full((G * F, n, n_t), float("nan"), dtype=torch.complex128, device=src.device)
    _launch(src, c["H"], c["y"], F, pad, out, xh)
    assert not torch.isnan(out).any() and not torch.isnan(torch.view_as_real(xh)).any()
    assert torch.equal(out[:, cp + n:], torch.zeros_like(out[:, cp + n:]))
    assert not torch.signbit(out[:, cp + n:]).any()
    assert torch.equal(out[:, :cp + n], c["rows"][:, :cp + n])         # the pad changes nothing above it
    assert torch.equal(torch.view_as_real(xh), torch.view_as_real(c["xh"]))
    out32 = torch.full(out.shape, float("nan"), dtype=torch.float32, device=src.device)
    _launch(src, c["H"], c["y"], F, pad, out32)
    assert not torch.isnan(out32).any()
    assert torch.equal(out32, out.to(torch.float32))
    rows32 = src.equalize_rows(c["H"], c["y"], F, EBNO, pad=shape[4], io="f32")
    assert rows32.dtype == torch.float32 and torch.equal(rows32, c["rows"].to(torch.float32))


@pytest.mark.parametrize("shape", SHAPES)
def test_a_frame_alone_is_the_frame_inside_the_batch_under_any_group_cut(shape):
    import torch
    n, cp, n_t, n_r, pad, G, F = shape
    c = _case(shape)
    src = c["src"]
    j = G * F - 1                                             # the last frame, alone with its group's H
    alone, x_alone = src.equalize_rows(c["H"][j // F:j // F + 1].contiguous(), c["y"][j:j + 1].contiguous(), 1, EBNO,
                                       pad=pad, want_xhat=True)
    assert torch.equal(alone[0], c["rows"][j])
    assert torch.equal(torch.view_as_real(x_alone[0]), torch.view_as_real(c["xh"][j]))
    # one frame per group, every frame with a copy of its H
    cut, x_cut = src.equalize_rows(c["H"].repeat_interleave(F, dim=0), c["y"], 1, EBNO, pad=pad, want_xhat=True)
    assert torch.equal(cut, c["rows"])
    assert torch.equal(torch.view_as_real(x_cut), torch.view_as_real(c["xh"]))


def test_method_refuses_mismatched_arguments():
    import torch
    c = _case(SHAPES[0])
    src = c["src"]
    with pytest.raises(ValueError, match="io"):
        src.equalize_rows(c["H"], c["y"], 2, EBNO, io="f16")
    with pytest.raises(ValueError, match="pad"):
        src.equalize_rows(c["H"], c["y"], 2, EBNO, pad=-1)
    with pytest.raises(ValueError, match="blocks of H"):
        src.equalize_rows(c["H"][:1], c["y"], 2, EBNO)
    with pytest.raises(ValueError, match="complex128"):
        src.equalize_rows(c["H"].to(torch.complex64), c["y"], 2, EBNO)
