"""The Monte-Carlo harness as four modules behind esn_ofdm_mimo_amd.montecarlo, and the two named parts of
DetectorSweep that need no GPU: the radius cache (on CPU tensors) and the layout of a chunk's result vector."""
import importlib

import numpy as np
import pytest

HOMES = {"link": ["LinkParams"],
         "frames": ["FrameSource", "percentiles_linear", "summarize_channel_metrics", "complex_as_io", "_view_real"],
         "sweep": ["DetectorSweep", "draw_reservoir", "blocks_for_rank", "reduce_counters"],
         "points": ["coded_ber_point", "block_fading_point"]}


@pytest.mark.parametrize("module", sorted(HOMES))
def test_montecarlo_re_exports_the_objects_of_the_four_modules(module):
    door = importlib.import_module("esn_ofdm_mimo_amd.montecarlo")
    home = importlib.import_module("esn_ofdm_mimo_amd." + module)          # (no GPU on this machine)
    for name in HOMES[module]:
        assert getattr(door, name) is getattr(home, name), name


def _cache(base=4, n=8):
    from esn_ofdm_mimo_amd.sweep import RadiusCache
    return RadiusCache(base, n, "cpu")


def _values(blocks):
    """(radius, status) that name the block they belong to."""
    import torch
    b = torch.as_tensor(list(blocks))
    return b.double() + 0.5, (b % 3).to(torch.int32)


def test_radius_cache_serves_a_chunk_slot_by_slot_once_all_of_it_is_stored():
    cache = _cache()
    assert cache.lookup(4, 4) is None                                      # nothing stored yet
    radius, status = _values([4, 5, 6, 7])                                 # first_block 4: slots 0..3 = blocks 4..7
    cache.store(4, 4, radius, status)
    got = cache.lookup(4, 4)
    assert got[0].tolist() == radius.tolist() and got[1].tolist() == status.tolist()
    assert got[0].dtype == radius.dtype and got[1].dtype == status.dtype
    assert cache.lookup(5, 4) is None                                      # block 8 is not stored yet
    assert cache.lookup(8, 4) is None
    radius, status = _values([8, 5, 6, 7])                                 # first_block 5: block b in slot b % 4
    cache.store(5, 4, radius, status)
    got = cache.lookup(5, 4)
    assert got[0].tolist() == [8.5, 5.5, 6.5, 7.5] and got[1].tolist() == status.tolist()
    assert cache.lookup(4, 5)[0].tolist() == [5.5, 6.5, 7.5, 8.5, 4.5]     # blocks 4..8 in slots b % 5
    assert cache.lookup(4, 6) is None                                      # block 9 is missing


def test_radius_cache_neither_stores_nor_serves_a_chunk_outside_its_range():
    cache = _cache(base=4, n=8)                                            # blocks 4 .. 11
    for first, n in ((4, 4), (8, 4)):
        cache.store(first, n, *_values(first + (np.arange(n) - first) % n))
    before = (cache.radius.clone(), cache.status.clone(), cache.filled.copy())
    for first, n in ((3, 4), (0, 2), (10, 4), (4, 9)):                     # starts before the base / runs past the end
        cache.store(first, n, *_values([99] * n))
        assert cache.lookup(first, n) is None
    assert cache.radius.equal(before[0]) and cache.status.equal(before[1]) and (cache.filled == before[2]).all()
    assert cache.lookup(4, 8) is not None                                  # the whole range is still served


@pytest.mark.parametrize("L,F", [(3, 2), (0, 2), (3, 0), (0, 0)])
def test_chunk_layout_tiles_the_vector_in_order(L, F):
    import torch
    from esn_ofdm_mimo_amd.sweep import ChunkLayout
    lay = ChunkLayout(L, F)
    assert lay.size == 3 + L + 2 * F
    cells = np.arange(lay.size)
    parts = [cells[lay.totals], cells[lay.flagged:lay.flagged + 1], cells[lay.choices], cells[lay.symbols]]
    assert [len(x) for x in parts] == [2, 1, L, 2 * F]
    assert np.concatenate(parts).tolist() == cells.tolist()               # errors, bits, flagged, L bins, 2 F counts
    one = lambda v: torch.tensor(v, dtype=torch.int64)
    choices = torch.arange(100, 100 + L) if L else None
    symbols = torch.arange(200, 200 + 2 * F).view(F, 2) if F else None
    vec = ChunkLayout.pack(torch, one(7), one(8), one(9), choices, symbols)
    assert vec.shape == (lay.size,) and vec.dtype == torch.int64
    assert vec[lay.totals].tolist() == [7, 8] and int(vec[lay.flagged]) == 9
    assert vec[lay.choices].tolist() == list(range(100, 100 + L))
    assert vec[lay.symbols].tolist() == list(range(200, 200 + 2 * F))
