"""esn_mmse_dcc_detect_count, FrameSource.mmse_dcc_detect_count and montecarlo.dcc_point on the device: n_iter = 0 bitwise
the LS-MMSE detector, X_hat and every counter against the NumPy model (tests/dcc_ref.py) on its supplied inputs, a frame's
independence of the rest of the launch, and the point's counters.  The model's slicer margin on these very inputs is held
on the CPU (tests/test_dcc_reference_cpu.py), so the counts are compared exactly and nothing is excluded."""
import numpy as np
import pytest

import dcc_ref as dr

pytestmark = pytest.mark.gpu

_dev = {}


def _on_device(shape, frames=dr.FRAMES):
    """The supplied inputs of a shape as device tensors, uploaded once."""
    import torch
    key = (shape, frames)
    if key not in _dev:
        d = dr.inputs(shape, frames)
        _dev[key] = {k: torch.from_numpy(np.array(d[k])).cuda() for k in ("p_i", "a_clip", "H", "y", "bits")}
    return _dev[key]


def _dcc(shape, t, n_iter, per_group=dr.PER_GROUP, count=True, want_xhat=True, want_iter=True, fill=0):
    """The C entry point on the tensors t: (rc, err [G], bits [G], err_iter [G, n_iter + 1] or None, X_hat or None)."""
    import torch
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    n, n_t, n_r, m, cp, _ = shape
    b, g = t["y"].shape[0], t["H"].shape[0]
    err, nb = (torch.full((g,), fill, dtype=torch.int64, device="cuda") for _ in range(2))
    it = torch.full((g, n_iter + 1), fill, dtype=torch.int64, device="cuda") if want_iter else None
    xh = torch.full((b, n, n_t), float("nan"), dtype=torch.complex128, device="cuda") if want_xhat else None
    rc = lib.esn_mmse_dcc_detect_count(b, per_group, n, cp, n_t, n_r, m, n_iter, _lib.ptr(t["p_i"]), _lib.ptr(t["a_clip"]),
                                       dr.NO, _lib.ptr(t["H"]), _lib.ptr(t["y"]), _lib.ptr(t["bits"]) if count else None,
                                       _lib.ptr(err), _lib.ptr(nb), _lib.ptr(it), _lib.ptr(xh), _lib.stream_handle())
    torch.cuda.synchronize()
    return rc, err, nb, it, xh


def _per_frame(t, order):
    """The frames `order` of t, one per group, each with its own copy of its group's H, Pi and clip level."""
    import torch
    idx = torch.as_tensor(order, device="cuda")
    grp = idx // dr.PER_GROUP
    return dict(p_i=t["p_i"][grp].contiguous(), a_clip=t["a_clip"][grp].contiguous(), H=t["H"][grp].contiguous(),
                y=t["y"][idx].contiguous(), bits=t["bits"][idx].contiguous())


@pytest.mark.parametrize("shape", [dr.SHAPES[3], dr.SHAPES[1]], ids=str)
def test_no_pass_is_the_mmse_detector_bit_for_bit(shape):
    import torch
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    n, n_t, n_r, m, cp, _ = shape
    t = _on_device(shape)
    rc, err, nb, it, xh = _dcc(shape, t, 0)
    assert rc == 0, lib.esn_last_error()
    g = t["H"].shape[0]
    e2, n2 = (torch.zeros(g, dtype=torch.int64, device="cuda") for _ in range(2))
    x2 = torch.full_like(xh, float("nan"))
    rc = lib.esn_mmse_detect_count(dr.FRAMES, dr.PER_GROUP, n, cp, n_t, n_r, m, _lib.ptr(t["p_i"]), dr.NO, _lib.ptr(t["H"]),
                                   _lib.ptr(t["y"]), _lib.ptr(t["bits"]), _lib.ptr(e2), _lib.ptr(n2), _lib.ptr(x2),
                                   _lib.stream_handle())
    assert rc == 0, lib.esn_last_error()
    torch.cuda.synchronize()
    assert torch.equal(err, e2) and torch.equal(nb, n2) and torch.equal(it[:, 0], e2)
    assert torch.equal(torch.view_as_real(xh), torch.view_as_real(x2))
    assert int(e2.sum()) > 0


def _against_model(shape, frames):
    from esn_ofdm_mimo_amd import _lib
    n_iter = shape[5]
    t, want = _on_device(shape, frames), dr.answers(shape, frames)
    rc, err, nb, it, xh = _dcc(shape, t, n_iter)
    assert rc == 0, _lib.load().esn_last_error()
    xh = xh.cpu().numpy()
    worst = 0.0
    for f in range(frames):
        ref = want["X"][f, n_iter]
        worst = max(worst, np.abs(xh[f] - ref).max() / np.abs(ref).max())
    print(shape, "X_hat against the model", worst, "err_iter", it.cpu().numpy().tolist())
    assert worst <= dr.XHAT_BOUND
    assert np.array_equal(it.cpu().numpy(), want["err_iter"])
    assert np.array_equal(err.cpu().numpy(), want["err"]) and np.array_equal(nb.cpu().numpy(), want["bits"])


@pytest.mark.parametrize("shape", dr.SHAPES, ids=str)
def test_xhat_and_every_count_match_the_model(shape):
    _against_model(shape, dr.FRAMES)


def test_the_largest_4x8_shape_is_served_and_the_next_is_refused():
    import torch
    from esn_ofdm_mimo_amd import _lib
    _against_model(dr.BIG_SHAPE, 1)
    n, n_t, n_r, m, cp, n_iter = dr.REFUSED_SHAPE
    t = dict(p_i=torch.ones(1, dtype=torch.float64, device="cuda"), a_clip=torch.ones(1, dtype=torch.float64, device="cuda"),
             H=torch.zeros((1, n, n_r, n_t), dtype=torch.complex128, device="cuda"),
             y=torch.zeros((1, n + cp, n_r), dtype=torch.complex128, device="cuda"),
             bits=torch.zeros((1, n * m, n_t), dtype=torch.uint8, device="cuda"))
    rc, err, nb, it, xh = _dcc(dr.REFUSED_SHAPE, t, n_iter, per_group=1, fill=7)
    msg = _lib.load().esn_last_error().decode()
    assert rc == -1 and "LDS" in msg and str(dr.lds_bytes(n, n_t, n_r)) in msg, (rc, msg)
    assert int(err[0]) == 7 and int(nb[0]) == 7 and bool(torch.isnan(xh.real).all())


@pytest.mark.parametrize("shape", [dr.SHAPES[3], dr.SHAPES[4]], ids=str)
def test_a_frame_is_the_same_alone_first_and_last_in_a_batch(shape):
    import torch
    n_iter = shape[5]
    t = _on_device(shape)
    _, _, _, it_all, xh_all = _dcc(shape, t, n_iter)
    others = [f for f in range(dr.FRAMES) if f != 4]
    rc, e1, n1, it1, x1 = _dcc(shape, _per_frame(t, [4]), n_iter, per_group=1)
    assert rc == 0
    rc, ea, na, ita, xa = _dcc(shape, _per_frame(t, [4] + others), n_iter, per_group=1)
    assert rc == 0
    rc, eb, nb, itb, xb = _dcc(shape, _per_frame(t, others + [4]), n_iter, per_group=1)
    assert rc == 0
    for x in (xa[0], xb[-1], xh_all[4]):
        assert torch.equal(torch.view_as_real(x), torch.view_as_real(x1[0]))
    assert torch.equal(ita[0], it1[0]) and torch.equal(itb[-1], it1[0])
    assert int(ea[0]) == int(eb[-1]) == int(e1[0]) == int(it1[0, -1]) and int(na[0]) == int(n1[0])
    # one frame per group adds up to the groups of three
    rc, _, _, itf, xf = _dcc(shape, _per_frame(t, list(range(dr.FRAMES))), n_iter, per_group=1)
    assert rc == 0 and torch.equal(torch.view_as_real(xf), torch.view_as_real(xh_all))
    grp = torch.arange(dr.FRAMES, device="cuda") // dr.PER_GROUP
    assert torch.equal(torch.zeros_like(it_all).index_add_(0, grp, itf), it_all)


def test_counters_do_not_depend_on_xhat_and_no_bits_means_no_counting():
    import torch
    shape = dr.SHAPES[3]
    n_iter = shape[5]
    t = _on_device(shape)
    _, err, nb, it, xh = _dcc(shape, t, n_iter)
    rc, err2, nb2, it2, none = _dcc(shape, t, n_iter, want_xhat=False)
    assert rc == 0 and none is None
    assert torch.equal(err, err2) and torch.equal(nb, nb2) and torch.equal(it, it2)
    rc, err3, nb3, none, _ = _dcc(shape, t, n_iter, want_iter=False)
    assert rc == 0 and none is None and torch.equal(err, err3) and torch.equal(nb, nb3)
    rc, err4, nb4, it4, xh4 = _dcc(shape, t, n_iter, count=False, fill=12345)
    assert rc == 0
    assert bool((err4 == 12345).all()) and bool((nb4 == 12345).all()) and bool((it4 == 12345).all())
    assert torch.equal(torch.view_as_real(xh4), torch.view_as_real(xh))
    # the counters are added to, not overwritten
    rc, err5, nb5, it5, _ = _dcc(shape, t, n_iter, fill=5)
    assert torch.equal(err5, err + 5) and torch.equal(nb5, nb + 5) and torch.equal(it5, it + 5)


def test_frame_source_method_is_the_entry_point_and_checks_its_clip_level():
    import torch
    from esn_ofdm_mimo_amd.montecarlo import FrameSource, LinkParams
    src = FrameSource(LinkParams(n_t=3, n_r=5, n_sub=16, isi=4), seed=5)
    taps = src.taps(3, 0, 0)
    bits, _, y = src.frames(taps, 3, 15.0, 0, 0, 1)
    bits, y = bits[:7].contiguous(), y[:7].contiguous()
    H = src.true_channel(taps)
    e0, n0, x0 = src.mmse_detect_count(H, y, bits, 3, 15.0, want_xhat=True)
    e, nb, xh, it = src.mmse_dcc_detect_count(H, y, bits, 3, 15.0, n_iter=0, want_xhat=True, want_iter_counts=True)
    assert torch.equal(e, e0) and torch.equal(nb, n0) and torch.equal(it[:, 0], e0)
    assert torch.equal(torch.view_as_real(xh), torch.view_as_real(x0))
    # the default clip level is the generator's; a per-group vector of it and a scalar are the same call
    a = src.p.a_clip(15.0)
    base = src.mmse_dcc_detect_count(H, y, bits, 3, 15.0, want_xhat=True, want_iter_counts=True)
    for clip in (a, [a, a, a], torch.full((3,), a, dtype=torch.float64, device=src.device)):
        out = src.mmse_dcc_detect_count(H, y, bits, 3, 15.0, a_clip=clip, want_xhat=True, want_iter_counts=True)
        assert all(torch.equal(torch.view_as_real(u) if u.is_complex() else u,
                               torch.view_as_real(v) if v.is_complex() else v) for u, v in zip(out, base))
    assert torch.equal(base[3][:, -1], base[0]) and base[3].shape == (3, 3)
    xonly = src.mmse_dcc_detect_count(H, y, None, 3, 15.0, want_xhat=True)
    assert xonly[0] is None and xonly[1] is None and torch.equal(torch.view_as_real(xonly[2]), torch.view_as_real(base[2]))
    for bad in (0.0, -1.0, float("nan"), float("inf"), [a, a]):
        with pytest.raises(ValueError, match="a_clip"):
            src.mmse_dcc_detect_count(H, y, bits, 3, 15.0, a_clip=bad)
    with pytest.raises(ValueError, match="n_iter"):
        src.mmse_dcc_detect_count(H, y, bits, 3, 15.0, n_iter=9)
    with pytest.raises(ValueError, match="X_hat"):
        src.mmse_dcc_detect_count(H, y, None, 3, 15.0)


def test_point_counters_do_not_depend_on_the_chunking_and_no_pass_is_the_mmse_leg():
    import torch
    from esn_ofdm_mimo_amd import montecarlo as mc
    src = mc.FrameSource(mc.LinkParams(), seed=3)
    kw = dict(frames_per_block=3, n_iter=2)
    whole = mc.dcc_point(src, 12.0, 1, 4, want_mmse=True, **kw)
    ones = mc.dcc_point(src, 12.0, 1, 4, chunk_blocks=1, want_mmse=True, **kw)
    threes = mc.dcc_point(src, 12.0, 1, 4, chunk_blocks=3, want_mmse=True, **kw)
    for other in (ones, threes):
        assert all(torch.equal(a, b) for a, b in zip(whole, other))
    lo = mc.dcc_point(src, 12.0, 1, 1, **kw)
    hi = mc.dcc_point(src, 12.0, 1, 3, first_block=1, **kw)
    assert torch.equal(torch.cat([lo[0], hi[0]]), whole[0]) and torch.equal(torch.cat([lo[1], hi[1]]), whole[1])
    assert torch.equal(lo[2] + hi[2], whole[2])
    assert whole[0].dtype == torch.int64 and whole[0].shape == (4,) and whole[2].shape == (3,)
    assert int(whole[2][2]) == int(whole[0].sum()) and int(whole[2][0]) == int(whole[3].sum()) > 0
    assert bool((whole[1] == 3 * 128 * 4 * 4).all())
    none = mc.dcc_point(src, 12.0, 1, 4, frames_per_block=3, n_iter=0)
    eq = mc.equalized_esn_point(src, 12.0, 1, 4, frames_per_block=3, want_mmse=True)
    assert torch.equal(none[0], eq[2]) and torch.equal(none[1], eq[3]) and torch.equal(none[0], whole[3])
    # a clip level told wrong is another detector
    off = mc.dcc_point(src, 12.0, 1, 4, a_clip_db_error=3.0, **kw)
    assert int(off[2][0]) == int(whole[2][0]) and not torch.equal(off[0], whole[0])


def test_two_passes_leave_at_most_a_fifth_of_the_mmse_errors_at_21_db():
    """21 dB, 16 blocks x 8 frames, the seed whose oracle counterpart is held to the same factor on the CPU (there 7348 ->
    211, a factor of 35; the issue's table has 29): a fifth of the oracle's factor is the margin for 16 blocks."""
    from esn_ofdm_mimo_amd import montecarlo as mc
    src = mc.FrameSource(mc.LinkParams(), seed=dr.POINT_SEED)
    err, nb, it = mc.dcc_point(src, dr.POINT_EBNO, 7, dr.POINT_BLOCKS, frames_per_block=dr.POINT_FRAMES, n_iter=2)
    it = it.cpu().numpy()
    print("bit errors after 0, 1, 2 passes", it.tolist(), "of", int(nb.sum()))
    assert int(nb.sum()) == dr.POINT_BLOCKS * dr.POINT_FRAMES * 128 * 4 * 4
    assert it[0] >= dr.POINT_GAIN * it[2] and it[0] > 0
