#!/usr/bin/env python3
"""What a greyscale source costs against the same image replicated to RGB, on one box in one process (not a bench.py leg, no pass / fail
number).  One batch of ``--batch`` single-channel images, out='source', through four routes:

  rgb      (a) ``forward_async_images`` on the plane replicated to three channels on the host: the yardstick, the parent's launches unchanged
  gray8    (b) ``forward_async_gray`` on the uint8 plane
  gray16   (c) ``forward_async_gray`` on the uint16 plane, 8-bit result
  gray16d  (d) ``forward_async_gray`` on the uint16 plane, 16-bit result (``depth=16``)

The uint16 kernels convert sRGB to linear with one float64 pow per sample (the uint8 ones read a 256-entry LDS table); the 65 536-entry table
in global memory that would replace it was not built, so (c) and (d) report that one form.

Per route the H2D, compute and D2H spans of ``idc_pipeline_times`` (end - start of each stage) and img/s = batch / (end of D2H - start of
H2D).  The routes alternate on the two slots, one batch at a time (nothing else is in flight while a span is taken), ``--warmup`` untimed
rounds first, then ``--runs`` timed ones; median (min / max) in ms.  Sources and results are pinned, so a span is the transfer itself, not a
staging copy.  Sources: noise of 203 x 187 and 1024 x 768, or ``--sizes h1xw1,h2xw2``.

usage: python tools/gray_timing.py [--precision bf16] [--batch 32] [--size 256] [--sizes 203x187,1024x768] [--runs 7] [--warmup 2] [--out f.json]
Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "runs": int(v.size)}


def pinned(e, arrays):
    out = [e.pinned_empty(a.shape, a.dtype) for a in arrays]
    for o, a in zip(out, arrays):
        o[...] = a
    return out


def spans(e, g16, runs, warmup):
    g8 = [(g >> 8).astype(np.uint8) for g in g16]
    src = {"rgb": pinned(e, [np.repeat(g[..., None], 3, 2) for g in g8]), "gray8": pinned(e, g8), "gray16": pinned(e, g16)}
    src["gray16d"] = src["gray16"]
    outs = {name: [e.pinned_empty(g.shape + (3,), np.uint16 if name == "gray16d" else np.uint8) for g in g16] for name in ("rgb", "gray8", "gray16", "gray16d")}
    got = {name: {"h2d": [], "compute": [], "d2h": [], "img_per_s": []} for name in outs}
    k = 0
    for r in range(warmup + runs):
        for name in ("rgb", "gray8", "gray16", "gray16d"):
            if name == "rgb":
                e.forward_async_images(k & 1, src[name], None, out_rgb=outs[name], out="source")
            else:
                e.forward_async_gray(k & 1, src[name], None, out_rgb=outs[name], out="source", depth=16 if name == "gray16d" else 8)
            e.wait(k & 1)
            t = e.pipeline_times(k & 1)
            if r >= warmup:
                got[name]["h2d"].append(float(t[1] - t[0]))
                got[name]["compute"].append(float(t[3] - t[2]))
                got[name]["d2h"].append(float(t[5] - t[4]))
                got[name]["img_per_s"].append(len(g16) / (float(t[5] - t[0]) * 1e-3))
            k += 1
    res = {name: {stage: spread(v) for stage, v in stages.items()} for name, stages in got.items()}
    for name in ("gray8", "gray16", "gray16d"):
        res[name]["h2d_vs_rgb"] = res[name]["h2d"]["median"] / res["rgb"]["h2d"]["median"]
        res[name]["compute_vs_rgb"] = res[name]["compute"]["median"] / res["rgb"]["compute"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256, help="net size (a smaller one only to rehearse the script)")
    ap.add_argument("--sizes", default="203x187,1024x768")
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
    res = {"precision": args.precision, "net": "%dx%d" % (H, W), "batch": args.batch, "srgb_to_linear_16": "pow per sample", "ms": {}}
    for spec in args.sizes.split(","):
        sh, sw = (int(v) for v in spec.split("x"))
        g16 = [rs.randint(0, 65536, (sh, sw)).astype(np.uint16) for _ in range(args.batch)]
        res["ms"][spec] = spans(e, g16, args.runs, args.warmup)
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
