"""Records what the seven *_point functions of esn_ofdm_mimo_amd.points and the constructor of DetectorSweep answer to
calls they must refuse -- the exception's class name and its full message -- into tests/golden/point_refusals.json, for
tests/test_point_refusals_cpu.py to replay: a rewrite of the argument checks that is meant to keep their answers keeps
every byte of every message and which check fires first.  Needs no GPU.

Run it from the tree of the commit whose answers are to be pinned (the package next to this tool is the one loaded):

    python tools/record_point_refusals.py --commit <hash>

Every row is refused from the arguments alone.  A point is called as fn(source, ebno_db=12.0, snr_idx=0, n_blocks=2,
**keywords) on a stub source: where a row's link is null, one whose every attribute raises (nothing of the source may be
read before the refusal); else types.SimpleNamespace(p=LinkParams(**link), seed=0, torch=None, device=None), for the
checks that read the link's shape.  The constructor is called as DetectorSweep(LinkParams(n_t=2, n_r=2, n_sub=64, **link),
**keywords).  Per function: every fault its checks know, once, and rows with two faults at once, which pin the order of
the checks.

Only rows that answer ValueError are written, and a row that answers anything else stops the recording.  Left out for
that reason: the three checks the recorded commit's constructor makes after it has opened the device -- ridge with
ridge_grid at one pilot, radius and radius_precision -- which answer EsnHipError on a machine without a GPU there
(tests/test_point_refusals_cpu.py holds them to ValueError on their own)."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "point_refusals.json")
SWEEP = "DetectorSweep"
POINTS = ("baseline_tracking_point", "elm_point", "fnn_point", "cnn_point", "lstm_point", "ensemble_point",
          "equalized_esn_point")
GRID, GRID17 = [1e-3, 1e-2], [10.0 ** -k for k in range(17)]
SMALL = dict(n_t=2, n_r=2, n_sub=64)                 # a link every comparator's training kernel serves
CONT = dict(continuation=True)

BLOCKS = [dict(n_blocks=0), dict(first_block=-1), dict(chunk_blocks=0), dict(frames_per_block=0)]
WINDOWED = [dict(slice="early"), dict(weights="fresh")]
ADAM = [dict(epochs=0), dict(epochs=2.5), dict(lr=-1.0)]

# function -> [(link or None, keywords)]: single faults first, then the rows with two faults
CASES = {
    "baseline_tracking_point": [(None, kw) for kw in [
        dict(track="directed"), dict(track="genie", window=0), dict(track="decisions", window=9), dict(window=1.5)]
        + BLOCKS + [
        dict(track="directed", window=0), dict(window=9, n_blocks=0), dict(n_blocks=0, chunk_blocks=0),
        dict(first_block=-1, frames_per_block=0), dict(chunk_blocks=0, frames_per_block=0)]],
    "elm_point": [(None, kw) for kw in WINDOWED + [
        dict(precision="bf16"), dict(window=0), dict(window=17), dict(window=2.5)] + BLOCKS + [
        dict(method="pinv"), dict(n_hidden=0), dict(n_hidden=2048), dict(n_hidden=64.0), dict(gain=0.0), dict(ridge=-1.0),
        dict(slice="early", weights="fresh"), dict(precision="bf16", window=0), dict(window=17, n_blocks=0),
        dict(frames_per_block=0, method="pinv"), dict(method="pinv", n_hidden=0), dict(n_hidden=0, gain=0.0),
        dict(gain=0.0, ridge=-1.0)]] + [
        (dict(n_t=4, n_r=9), dict(window=16)), (dict(n_t=4, n_r=9), dict(window=16, ridge=-1.0))],
    "fnn_point": [(None, kw) for kw in WINDOWED + [
        dict(precision="f32"), dict(window=0), dict(window=17)] + BLOCKS + [
        dict(n_hidden=0), dict(n_hidden=100.0),
        dict(slice="early", n_hidden=0), dict(chunk_blocks=0, n_hidden=0), dict(n_hidden=0, epochs=0)]] + [
        (SMALL, kw) for kw in ADAM + [dict(n_hidden=600), dict(epochs=0, lr=-1.0), dict(lr=-1.0, n_hidden=600)]] + [
        ({}, dict(n_hidden=128))],
    "cnn_point": [(None, kw) for kw in WINDOWED + BLOCKS + [
        dict(channels=(32,)), dict(channels=(32, 0)), dict(channels=(32, 64.0)), dict(kernel=5.0),
        dict(weights="fresh", channels=(32,)), dict(frames_per_block=0, kernel=5.0), dict(channels=(32,), kernel=5.0),
        dict(kernel=5.0, epochs=0)]] + [
        (SMALL, kw) for kw in ADAM + [dict(kernel=4), dict(channels=(32, 200)), dict(epochs=0, kernel=4),
                                      dict(lr=-1.0, channels=(32, 200))]],
    "lstm_point": [(None, kw) for kw in WINDOWED + BLOCKS + [
        dict(n_hidden=0), dict(n_hidden=100.0),
        dict(slice="early", weights="fresh"), dict(weights="fresh", n_blocks=0), dict(first_block=-1, n_hidden=0),
        dict(n_hidden=0, epochs=0)]] + [
        (SMALL, kw) for kw in ADAM + [dict(n_hidden=129), dict(epochs=0, n_hidden=129), dict(lr=-1.0, n_hidden=129)]],
    "ensemble_point": [(None, kw) for kw in [
        dict(n_members=0), dict(n_members=2.0), dict(n_members=1000), dict(reservoirs="pool"), dict(method="svd"),
        dict(io="f16"), dict(io="f32", precision="f64"), dict(ridge=1.0, ridge_grid=GRID), dict(ridge=-1.0)] + BLOCKS + [
        dict(n_members=0, reservoirs="pool"), dict(reservoirs="pool", method="svd"), dict(method="svd", io="f16"),
        dict(io="f32", precision="f64", ridge=1.0, ridge_grid=GRID), dict(ridge=-1.0, ridge_grid=GRID),
        dict(ridge=-1.0, n_blocks=0)]] + [
        (CONT, {}), (CONT, dict(frames_per_block=0))],
    "equalized_esn_point": [(None, kw) for kw in [
        dict(reservoirs="fresh"), dict(reservoirs="pool"), dict(method="svd"), dict(io="f16"), dict(io="f32"),
        dict(ridge=-1.0)] + BLOCKS + [
        dict(n_reservoir=1), dict(n_reservoir=8.0), dict(delay=-1), dict(delay=1.0), dict(reservoirs="per_block", pool=0),
        dict(reservoirs="fresh", method="svd"), dict(method="svd", io="f16"), dict(io="f16", ridge=-1.0),
        dict(io="f32", ridge=-1.0), dict(chunk_blocks=0, n_reservoir=1), dict(n_reservoir=1, delay=-1),
        dict(delay=-1, reservoirs="per_block", pool=0)]] + [
        (CONT, {}), (dict(n_t=5, n_r=8), {}), ({}, dict(sparsity=1.0)),
        (CONT, dict(reservoirs="per_block", pool=0)), (dict(n_t=5, n_r=8, continuation=True), {}),
        (dict(n_t=5, n_r=8), dict(sparsity=1.0))],
    SWEEP: [({}, kw) for kw in [
        dict(io="f16"), dict(io="f32", precision="f64"), dict(track_forget=1.5), dict(track_forget=-0.1),
        dict(track="directed"), dict(track="genie", track_window=0), dict(track="decisions", ridge_grid=GRID),
        dict(track="decisions", train_ebno=12.0), dict(track="genie", io="f32", precision="f32"),
        dict(n_pilots=1.5), dict(n_pilots=0, ridge_grid=GRID),
        dict(solve_method="gram"), dict(solve_method="gram", ridge_grid=GRID),
        dict(n_pilots=2, track="decisions"), dict(n_pilots=2, train_ebno=12.0),
        dict(n_pilots=2, ridge=1.0, ridge_grid=GRID),
        dict(n_pilots=2, ridge_grid=GRID17), dict(n_pilots=2, ridge_grid=[]),
        # two faults and more
        dict(io="f16", track="directed"), dict(io="f32", precision="f64", track_forget=1.5),
        dict(track_forget=1.5, track="directed"), dict(track="directed", n_pilots=0),
        dict(track="genie", track_window=0, ridge_grid=GRID), dict(track="genie", track_window=0, n_pilots=1.5),
        dict(track="decisions", ridge_grid=GRID, train_ebno=12.0),
        dict(track="decisions", ridge_grid=GRID, io="f32", precision="f32"),
        dict(track="decisions", train_ebno=12.0, io="f32", precision="f32"),
        dict(track="decisions", ridge_grid=GRID, train_ebno=12.0, io="f32", precision="f32"),
        dict(track="decisions", solve_method="gram", ridge_grid=GRID),
        dict(track="decisions", solve_method="gram", ridge=1.0, train_ebno=12.0),
        dict(track="decisions", ridge_grid=GRID, n_pilots=2), dict(track="decisions", train_ebno=12.0, n_pilots=2),
        dict(track="decisions", n_pilots=0),
        dict(n_pilots=2, track="decisions", train_ebno=12.0), dict(n_pilots=2, track="decisions", ridge_grid=GRID17),
        dict(n_pilots=2, train_ebno=12.0, ridge=1.0, ridge_grid=GRID),
        dict(n_pilots=2, train_ebno=12.0, ridge_grid=GRID17),
        dict(n_pilots=2, ridge=1.0, ridge_grid=GRID17),
        dict(n_pilots=2, solve_method="gram"), dict(n_pilots=2, solve_method="gram", ridge=1.0, ridge_grid=GRID),
        dict(n_pilots=2, solve_method="gram", ridge=1.0, train_ebno=12.0),
        dict(n_pilots=2, solve_method="gram", ridge_grid=GRID17),
        dict(n_pilots=1.5, solve_method="gram"), dict(solve_method="gram", track="genie", track_window=0)]] + [
        (CONT, kw) for kw in [
        dict(track="decisions"), dict(track="decisions", ridge_grid=GRID), dict(track="decisions", train_ebno=12.0),
        dict(track="genie", io="f32", precision="f32"), dict(solve_method="gram", ridge=1.0), dict(solve_method="gram"),
        dict(solve_method="gram", ridge_grid=GRID), dict(solve_method="gram", ridge=1.0, track="decisions"),
        dict(n_pilots=2), dict(n_pilots=2, track="decisions"), dict(n_pilots=2, train_ebno=12.0),
        dict(n_pilots=2, ridge=1.0, ridge_grid=GRID), dict(n_pilots=2, ridge_grid=GRID17),
        dict(n_pilots=2, solve_method="gram", ridge=1.0)]],
}


class NoDevice:
    """A source nothing may be read of."""

    def __getattr__(self, name):
        raise AssertionError("the FrameSource was touched: " + name)


def cases():
    """[(function, link keywords or None, keywords)], JSON-ready (tuples as lists)."""
    return json.loads(json.dumps([(fn, link, kw) for fn, rows in CASES.items() for link, kw in rows]))


def answer(fn, link, kw):
    """(class name, message) of the exception the call raises; (None, None) if it returns."""
    from esn_ofdm_mimo_amd import points
    from esn_ofdm_mimo_amd.link import LinkParams
    from esn_ofdm_mimo_amd.sweep import DetectorSweep
    try:
        if fn == SWEEP:
            DetectorSweep(LinkParams(**dict(SMALL, **link)), **kw)
        else:
            src = NoDevice() if link is None else types.SimpleNamespace(p=LinkParams(**link), seed=0, torch=None,
                                                                        device=None)
            getattr(points, fn)(src, **dict(dict(ebno_db=12.0, snr_idx=0, n_blocks=2), **kw))
    except Exception as e:      # noqa: BLE001 (the class is what is recorded)
        return type(e).__name__, str(e)
    return None, None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit this tree is")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    rows = []
    for fn, link, kw in cases():
        cls, text = answer(fn, link, kw)
        if cls != "ValueError":
            sys.exit(f"{fn} {link} {kw}: answered {cls}: {text}; nothing written")
        rows.append({"fn": fn, "link": link, "kw": kw, "class": cls, "error": text})
    with open(args.out, "w") as f:
        f.write('{"commit": %s, "rows": [\n' % json.dumps(args.commit))
        f.write(",\n".join(json.dumps(r, sort_keys=True) for r in rows))          # one call per line
        f.write("\n]}\n")
    print(f"{args.out}: {len(rows)} rows")


if __name__ == "__main__":
    main()
