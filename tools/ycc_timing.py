#!/usr/bin/env python3
"""What the YCbCr 4:2:0 output planes cost and save against interleaved RGB, on one box in one process (not a bench.py leg, no pass / fail
number).  One batch of ``--batch`` RGB images, out='source', through three output formats of ``set_batch_output``:

  rgb    (a) ``forward_async_images`` with the format off: the yardstick, the parent's launches unchanged, 3 bytes a pixel back
  i420   (b) the same call under 'i420' / 'jfif': the post-pass kernel behind the epilogue, 1.5 bytes a pixel back
  nv12   (c) the same call under 'nv12' / 'bt709'

Per format the H2D, compute and D2H spans of ``idc_pipeline_times`` (end - start of each stage; the post-pass counts under compute) and
img/s = batch / (end of D2H - start of H2D).  The formats alternate on the two slots, one batch at a time (nothing else is in flight while a
span is taken), ``--warmup`` untimed rounds first, then ``--runs`` timed ones; median (min / max) in ms.  Sources and results are pinned, so a
span is the transfer itself, not a staging copy.  Sources: noise of 1024 x 768 and 203 x 187, or ``--sizes h1xw1,h2xw2``.

usage: python tools/ycc_timing.py [--precision bf16] [--batch 32] [--size 256] [--sizes 1024x768,203x187] [--runs 7] [--warmup 2] [--out f.json]
Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np

ROUTES = (("rgb", "rgb", "jfif"), ("i420", "i420", "jfif"), ("nv12", "nv12", "bt709"))


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "runs": int(v.size)}


def spans(e, images, runs, warmup):
    from interactive_deep_colorization_amd import engine
    src = [e.pinned_empty(a.shape, np.uint8) for a in images]
    for s, a in zip(src, images):
        s[...] = a
    outs = {"rgb": [e.pinned_empty(a.shape, np.uint8) for a in images]}
    for name in ("i420", "nv12"):
        outs[name] = [e.pinned_empty((engine.ycc420_bytes(a.shape[0], a.shape[1]),), np.uint8) for a in images]
    got = {name: {"h2d": [], "compute": [], "d2h": [], "img_per_s": []} for name, _, _ in ROUTES}
    k = 0
    try:
        for r in range(warmup + runs):
            for name, fmt, matrix in ROUTES:
                e.set_batch_output(fmt, matrix)
                e.forward_async_images(k & 1, src, None, out_rgb=outs[name], out="source")
                e.wait(k & 1)
                t = e.pipeline_times(k & 1)
                if r >= warmup:
                    got[name]["h2d"].append(float(t[1] - t[0]))
                    got[name]["compute"].append(float(t[3] - t[2]))
                    got[name]["d2h"].append(float(t[5] - t[4]))
                    got[name]["img_per_s"].append(len(images) / (float(t[5] - t[0]) * 1e-3))
                k += 1
    finally:
        e.set_batch_output("rgb")
    res = {name: {stage: spread(v) for stage, v in stages.items()} for name, stages in got.items()}
    for name in ("i420", "nv12"):
        res[name]["d2h_vs_rgb"] = res[name]["d2h"]["median"] / res["rgb"]["d2h"]["median"]
        res[name]["compute_minus_rgb_ms"] = res[name]["compute"]["median"] - res["rgb"]["compute"]["median"]
        res[name]["bytes_out"] = int(sum(o.size for o in outs[name]))
    res["rgb"]["bytes_out"] = int(sum(o.size for o in outs["rgb"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256, help="net size (a smaller one only to rehearse the script)")
    ap.add_argument("--sizes", default="1024x768,203x187")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: at least five timed runs")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    from interactive_deep_colorization_amd import engine, workloads
    H = W = args.size
    rs = np.random.RandomState(args.seed)
    e = engine.HipColorizer(H, W, max_batch=args.batch, precision=args.precision)
    e.load_state_dict(workloads.random_state_dict(0, "he"))
    res = {"precision": args.precision, "net": "%dx%d" % (H, W), "batch": args.batch, "ms": {}}
    for spec in args.sizes.split(","):
        sh, sw = (int(v) for v in spec.split("x"))
        images = [rs.randint(0, 256, (sh, sw, 3)).astype(np.uint8) for _ in range(args.batch)]
        res["ms"][spec] = spans(e, images, args.runs, args.warmup)
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
