"""elm_point and fnn_point refuse the arguments they share -- slice, weights, precision, window, chunk_blocks,
first_block -- in the same words, and before they touch their FrameSource (no GPU needed: nothing is opened)."""
import re

import pytest

from esn_ofdm_mimo_amd import points

REFUSALS = [
    (dict(slice="early"), "slice must be 'aligned' or 'reference', not 'early'"),
    (dict(weights="fresh"), "weights must be 'shared' or 'per_block', not 'fresh'"),
    (dict(precision="bf16"), "precision must be 'f64' or 'f16', not 'bf16'"),
    (dict(precision="f32"), "precision must be 'f64' or 'f16', not 'f32'"),
    (dict(window=0), "window must be an integer in 1..16, not 0"),
    (dict(window=17), "window must be an integer in 1..16, not 17"),
    (dict(window=2.5), "window must be an integer in 1..16, not 2.5"),
    (dict(chunk_blocks=0), "chunk_blocks = 0 must be positive"),
    (dict(first_block=-1), "n_blocks = 2 must be positive and first_block = -1 non-negative"),
]


class NoDevice:
    def __getattr__(self, name):
        raise AssertionError("the FrameSource was touched: " + name)


@pytest.mark.parametrize("point", [points.elm_point, points.fnn_point], ids=["elm_point", "fnn_point"])
@pytest.mark.parametrize("kw,text", REFUSALS, ids=[next(iter(r[0])) + "=" + str(next(iter(r[0].values()))) for r in REFUSALS])
def test_a_bad_shared_argument_is_refused_in_the_same_words_before_the_source_is_touched(point, kw, text):
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        point(NoDevice(), 12.0, 0, 2, **kw)
