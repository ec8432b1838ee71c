#!/usr/bin/env python3
"""What painted hint layers cost against a layer-free batch and against the same hints as a rectangle list, on one box in one process (not a
bench.py leg, no pass / fail number).  One batch of ``--batch`` RGB sources of 1024 x 768 submitted alone through ``forward_async_layers``,
out='net', pinned buffers, in five forms:

  free        no layers: the launches of ``forward_async_images`` unchanged -- the baseline of the same run
  1024x768    an RGBA layer of the source's size per image (3.1 MB each: four thirds of the RGB source)
  256x256     a net-size layer per image (0.26 MB each)
  rects       the hints of the 256x256 layer as one 1 x 1 IDC_HINT_RGB rectangle per painted net cell (the workaround layers replace);
              left out where the list would pass IDC_BATCH_MAX_HINTS

at three paint densities: about 2 %, about 30 % and all of the net's cells painted (whole cells are painted, so both layer sizes hint the same
cells).  Per form the H2D and compute spans of ``idc_pipeline_times`` (end - start of the stage); the forms alternate on the two slots, one
batch at a time (nothing else is in flight while a span is taken), ``--warmup`` untimed rounds first, then ``--runs`` timed ones; median
(min / max) in ms, and form - free of the medians.  The rectangle lists take three timed runs: marshalling one takes seconds on the host.

usage: python tools/layer_timing.py [--precision bf16] [--batch 32] [--size 256] [--runs 7] [--warmup 2] [--out f.json]
Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np

MAX_HINTS = 1 << 20


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "runs": int(v.size)}


def pinned(e, arrays):
    out = [e.pinned_empty(a.shape, a.dtype) for a in arrays]
    for o, a in zip(out, arrays):
        o[...] = a
    return out


def paint(rs, H, W, lh, lw, cells):
    """An (lh,lw,4) layer whose painted pixels are exactly those over the net cells ``cells`` (H,W) bool; lh, lw multiples of H, W."""
    a = np.zeros((lh, lw, 4), np.uint8)
    m = np.repeat(np.repeat(cells, lh // H, 0), lw // W, 1)
    a[..., :3] = rs.randint(0, 256, (lh, lw, 3))
    a[..., 3] = np.where(m, 255, 0)
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256, help="net size (a smaller one only to rehearse the script)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs < 3:
        ap.error("--runs: at least three timed runs")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    from interactive_deep_colorization_amd import engine, workloads
    H = W = args.size
    n = args.batch
    rs = np.random.RandomState(args.seed)
    e = engine.HipColorizer(H, W, max_batch=n, precision=args.precision)
    e.load_state_dict(workloads.random_state_dict(0, "he"))
    src = pinned(e, [rs.randint(0, 256, (1024, 768, 3)).astype(np.uint8) for _ in range(n)])
    outs = [e.pinned_empty((H, W, 3), np.uint8) for _ in range(n)]
    res = {"precision": args.precision, "net": "%dx%d" % (H, W), "batch": n, "source_mb": sum(a.nbytes for a in src) / 1e6, "ms": {}}
    for label, density in (("2%", 0.02), ("30%", 0.30), ("full", 1.0)):
        cells = [rs.random_sample((H, W)) < density for _ in range(n)]
        big = pinned(e, [paint(rs, H, W, 4 * H, 3 * W, c) for c in cells])
        net = pinned(e, [paint(rs, H, W, H, W, c) for c in cells])
        rects = [[(int(y), int(x), int(y), int(x)) + tuple(int(v) for v in l[y, x, :3]) for y, x in zip(*np.nonzero(c))] for l, c in zip(net, cells)]
        forms = {"free": dict(layers=None, hints=None), "%dx%d" % (4 * H, 3 * W): dict(layers=big, hints=None),
                 "%dx%d" % (H, W): dict(layers=net, hints=None)}
        if sum(len(r) for r in rects) <= MAX_HINTS:
            forms["rects"] = dict(layers=None, hints=rects)
        got = {name: {"h2d": [], "compute": []} for name in forms}
        counts = {}
        k = 0
        for r in range(args.warmup + args.runs):
            for name, f in forms.items():
                if name == "rects" and not args.warmup - 1 <= r < args.warmup + 3:      # (marshalling a long list takes seconds on the host: three timed runs)
                    continue
                _, c = e.forward_async_layers(k & 1, src, f["layers"], f["hints"], out_rgb=outs, mode="rgb", out="net")
                e.wait(k & 1)
                t = e.pipeline_times(k & 1)
                if c is not None:
                    counts[name] = int(np.array(c).sum())
                if r >= args.warmup:
                    got[name]["h2d"].append(float(t[1] - t[0]))
                    got[name]["compute"].append(float(t[3] - t[2]))
                k += 1
        row = {name: {stage: spread(v) for stage, v in stages.items()} for name, stages in got.items()}
        for name in forms:
            if name != "free":
                row[name]["minus_free"] = {s: row[name][s]["median"] - row["free"][s]["median"] for s in ("h2d", "compute")}
        row["painted_cells"] = int(sum(c.sum() for c in cells))
        row["cells_reported"] = counts
        row["rectangles"] = sum(len(r) for r in rects)
        row["layer_mb"] = {"%dx%d" % (4 * H, 3 * W): sum(a.nbytes for a in big) / 1e6, "%dx%d" % (H, W): sum(a.nbytes for a in net) / 1e6}
        res["ms"][label] = row
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
