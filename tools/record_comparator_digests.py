"""Records SHA-256 digests of what the Adam-trained comparator banks (FnnBank, CnnBank, LstmBank) train and predict and of
what elm_point, fnn_point, cnn_point and lstm_point count, into tests/golden/comparator_digests.json for
tests/test_gpu_comparator_digests.py: a rewrite of the banks' and the points' host side that is meant to keep the results
keeps every byte.  Needs a GPU.

Run it from the tree of the commit whose results are to be pinned (the package next to this tool is the one loaded; only
its public surface is used):

    python tools/record_comparator_digests.py --commit <hash>

Banks, each at the "everything odd" row of the SHAPES of its tests/test_gpu_*.py and the LSTM also at H = 128 (columns of
W_hh streamed): all four scalings set, per group and non-zero; two rotating initial sets with a group offset where the row
has them; every trained array and the loss; then 7 frames at frames_per_group 5 (a ragged second group), transient 2 --
for the FNN also at "f16".  The H = 128 row trains one group, so its prediction reads that trained set from a bank that
holds it twice.  Points, each at the 2x2, N = 64, QPSK link of the tests' POINT_CASES: 3 blocks of 4 frames in chunks of 2
(a chunk with a remainder), weights "per_block" and "shared", the errors and bits tensors; elm_point at n_hidden = 64."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "comparator_digests.json")
SEED = 20261021
LR = 0.01
FRAMES, FRAMES_PER_GROUP, PREDICT_TRANSIENT = 7, 5, 2
# name -> (module, bank class, constructor arguments after (n_in, n_out), {parameter: shape of one set}, prediction
#          precisions, (n_in, n_out, T_in, T, n_groups, n_isets, group_offset, transient, epochs))
ODD = (4, 3, 19, 23, 2, 2, 1, 2, 10)        # n_in .. epochs of the "everything odd" rows
BANKS = {
    "fnn": ("fnn", "FnnBank", (17, 3), dict(W1=(17, 12), b1=(17,), W2=(3, 17), b2=(3,)), ("f64", "f16"), ODD),
    "cnn": ("cnn", "CnnBank", ((7, 19), 3),
            dict(W1=(7, 4, 3), b1=(7,), W2=(19, 7, 3), b2=(19,), W3=(3, 19, 3), b3=(3,)), ("f64",), ODD),
    "lstm": ("lstm", "LstmBank", (7,),
             dict(W_ih=(28, 4), W_hh=(28, 7), b_ih=(28,), b_hh=(28,), W_fc=(3, 7), b_fc=(3,)), ("f64",), ODD),
    "lstm_h128": ("lstm", "LstmBank", (128,),
                  dict(W_ih=(512, 6), W_hh=(512, 128), b_ih=(512,), b_hh=(512,), W_fc=(2, 128), b_fc=(2,)), ("f64",),
                  (6, 2, 13, 17, 1, 1, 0, 0, 5)),
}
LINK = dict(n_t=2, n_r=2, n_sub=64, m=2, channel="exp")
SOURCE_SEED, EBNO, SNR_IDX, POINT_SEED = 11, 15.0, 2, 3
POINT_KW = dict(frames_per_block=4, chunk_blocks=2, seed=POINT_SEED)
N_BLOCKS = 3
POINTS = {"elm": dict(n_hidden=64), "fnn": {}, "cnn": {}, "lstm": {}}


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def arrays(name):
    """Host arrays of one bank row: init (n_isets sets), the four scalings [n_groups, .], U, D and the frames to predict
    for ceil(FRAMES / FRAMES_PER_GROUP) groups -- from a seeded generator, so this tool and the test build the same."""
    shapes, (n_in, n_out, t_in, T, G, S) = list(BANKS[name][3].values()), BANKS[name][5][:6]
    rs = np.random.RandomState([SEED, list(BANKS).index(name)])
    a = 1.0 / np.sqrt(shapes[1][0])
    n_pred = max(G, -(-FRAMES // FRAMES_PER_GROUP))
    sign = lambda *s: np.where(rs.rand(*s) < 0.5, -1.0, 1.0)       # noqa: E731
    c = dict(init=tuple(rs.uniform(-a, a, (S,) + s) for s in shapes),
             in_scale=rs.uniform(0.5, 2.0, (n_pred, n_in)),
             in_shift=sign(n_pred, n_in) * rs.uniform(0.05, 0.2, (n_pred, n_in)),
             t_scale=rs.uniform(0.5, 2.0, (n_pred, n_out)),
             t_shift=sign(n_pred, n_out) * rs.uniform(0.05, 0.2, (n_pred, n_out)))
    c["U"] = rs.randn(G, t_in, n_in) / c["in_scale"][:G, None, :]
    c["D"] = rs.randn(G, T, n_out)
    c["frames"] = rs.randn(FRAMES, t_in, n_in) / c["in_scale"][np.arange(FRAMES) // FRAMES_PER_GROUP][:, None, :]
    return c


def bank_digests(name):
    """{array or prediction: digest} of one row of BANKS, from the package next to this tool."""
    import importlib
    module, cls, ctor, names, precisions, (n_in, n_out, t_in, T, G, S, off, transient, epochs) = BANKS[name]
    mod = importlib.import_module("esn_ofdm_mimo_amd." + module)
    c = arrays(name)
    scaling = [c[k] for k in ("in_scale", "in_shift", "t_scale", "t_shift")]
    bank = getattr(mod, cls)(n_in, n_out, *ctor, n_groups=G)
    bank.set_scaling(*[s[:G] for s in scaling])
    bank.train(c["U"], c["D"], c["init"], transient=transient, epochs=epochs, lr=LR, group_offset=off, want_loss=True)
    out = {n: sha(getattr(bank, n)) for n in list(names) + ["loss"]}
    n_pred = scaling[0].shape[0]
    if n_pred > G:                                  # one trained set, held for every group of the prediction
        trained = [getattr(bank, n).repeat((n_pred,) + (1,) * (getattr(bank, n).ndim - 1)) for n in names]
        bank = getattr(mod, cls)(n_in, n_out, *ctor, n_groups=n_pred)
        bank.set_scaling(*scaling)
        bank.set_weights(*trained)
    for precision in precisions:
        out["predict_" + precision] = sha(bank.predict(c["frames"], FRAMES_PER_GROUP, T=T, transient=PREDICT_TRANSIENT,
                                                       precision=precision))
    return out


def point_digests(name):
    """{weights + " errors" / " bits": digest} of one point function, from the package next to this tool."""
    from esn_ofdm_mimo_amd import montecarlo as mc
    src = mc.FrameSource(mc.LinkParams(**LINK), seed=SOURCE_SEED)
    out = {}
    for weights in ("per_block", "shared"):
        errors, bits = getattr(mc, name + "_point")(src, EBNO, SNR_IDX, N_BLOCKS, weights=weights, **POINT_KW,
                                                    **POINTS[name])
        out[weights + " errors"], out[weights + " bits"] = sha(errors), sha(bits)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit this tree is")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    doc = {"commit": args.commit, "seed": SEED, "banks": {n: bank_digests(n) for n in BANKS},
           "points": {n: point_digests(n) for n in POINTS}}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {sum(len(v) for v in doc['banks'].values())} bank and "
          f"{sum(len(v) for v in doc['points'].values())} point digests")


if __name__ == "__main__":
    main()
