#!/usr/bin/env python3
"""What the joint bilateral upsampling (``set_batch_upsample('joint')``) adds to a source-size batch, on one box in one process (not a
bench.py leg, no pass / fail number).  The figure is the compute span of ``idc_pipeline_times`` (compute end - compute start) of one batch of
``--batch`` images through ``forward_async_images``, which is what ``colorize_images(out='source')`` enqueues:

  net      out='net': prologue, network, ``lab_post_kernel`` -- no source-size epilogue at all
  linear   out='source' with the linear zoom (``packed_fullres_kernel``)
  joint    out='source' with ``joint_fullres_kernel`` in its place (both templates over the source format; these legs run RGB8) (R, sigma_s, sigma_r from ``--radius`` / ``--sigma-s`` / ``--sigma-r``)

The three legs alternate on the two slots, one batch at a time (nothing else is in flight while a span is taken), ``--warmup`` untimed rounds
first, then ``--runs`` timed ones; median (min / max) in ms.  ``epilogue`` = a leg's median minus the 'net' median: what the source-size step
costs; ``added`` = joint minus linear.  Sources: noise (every range weight is exercised; the kernel's work does not depend on the content
otherwise) of 203 x 187 and 1024 x 768, or ``--sizes h1xw1,h2xw2``.

usage: python tools/joint_timing.py [--precision bf16] [--batch 32] [--size 256] [--sizes 203x187,1024x768] [--runs 7] [--warmup 2]
                                    [--radius 2] [--sigma-s 1.0] [--sigma-r 8.0] [--out f.json]
Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "runs": int(v.size)}


def spans(e, images, runs, warmup):
    legs = [("net", "net", "linear"), ("linear", "source", "linear"), ("joint", "source", "joint")]
    srcs = [e.pinned_empty(a.shape, np.uint8) for a in images]
    for s, a in zip(srcs, images):
        s[...] = a
    got = {name: [] for name, _, _ in legs}
    k = 0
    for r in range(warmup + runs):
        for name, out, up in legs:
            e.set_batch_upsample(up)
            e.forward_async_images(k & 1, srcs, None, out=out)
            e.wait(k & 1)
            t = e.pipeline_times(k & 1)
            if r >= warmup:
                got[name].append(float(t[3] - t[2]))
            k += 1
    e.set_batch_upsample("linear")
    res = {name: spread(v) for name, v in got.items()}
    res["epilogue_linear_ms"] = res["linear"]["median"] - res["net"]["median"]
    res["epilogue_joint_ms"] = res["joint"]["median"] - res["net"]["median"]
    res["added_ms"] = res["joint"]["median"] - res["linear"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256, help="net size (a smaller one only to rehearse the script)")
    ap.add_argument("--sizes", default="203x187,1024x768")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--sigma-s", type=float, default=1.0)
    ap.add_argument("--sigma-r", type=float, default=8.0)
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
    e.set_joint_upsample(args.radius, args.sigma_s, args.sigma_r)
    res = {"precision": args.precision, "net": "%dx%d" % (H, W), "batch": args.batch, "radius": args.radius, "sigma_s": args.sigma_s,
           "sigma_r": args.sigma_r, "compute_ms": {}}
    for spec in args.sizes.split(","):
        sh, sw = (int(v) for v in spec.split("x"))
        images = [rs.randint(0, 256, (sh, sw, 3)).astype(np.uint8) for _ in range(args.batch)]
        res["compute_ms"][spec] = spans(e, images, args.runs, args.warmup)
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
