#!/usr/bin/env python3
"""What antialiased ingestion costs against the point-sampled rule, on one box in one process (not a bench.py leg, no pass / fail number).
Three workloads, each with the ingest filter off and on:

  203x187      one batch of ``--batch`` RGB sources of 203 x 187 through ``forward_async_images``, out='net'
               (not down-scaled on a 256 x 256 net: the filter launches nothing, so the two figures show the noise of the measurement)
  1024x768     one batch of ``--batch`` RGB sources of 1024 x 768, the same call: the pre-pass reads 2.4 MB per image
  gray4000x3000  one batch of ``--gray-batch`` uint16 planes of 4000 x 3000 through ``forward_async_gray``, out='net': 24 MB per image

The filter-off figure is the parent's launches unchanged (the filter off adds no launch and changes no plan byte), so it is the baseline.
Per workload and setting the H2D, compute and D2H spans of ``idc_pipeline_times`` (end - start of each stage).  The two settings alternate
on the two slots, one batch at a time (nothing else is in flight while a span is taken), ``--warmup`` untimed rounds first, then ``--runs``
timed ones; median (min / max) in ms, and on - off of the compute medians = the pre-pass together with what the ingestion kernels save by
reading a net-size image.  Sources and results are pinned, so a span is the transfer itself, not a staging copy.

usage: python tools/resample_timing.py [--precision bf16] [--batch 32] [--gray-batch 4] [--size 256] [--runs 7] [--warmup 2] [--out f.json]
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


def spans(e, images, runs, warmup):
    gray = images[0].ndim == 2
    src = pinned(e, images)
    outs = [e.pinned_empty((e.H, e.W, 3), np.uint8) for _ in images]
    got = {name: {"h2d": [], "compute": [], "d2h": []} for name in ("off", "on")}
    k = 0
    for r in range(warmup + runs):
        for name in ("off", "on"):
            e.set_ingest_filter("antialias" if name == "on" else "bilinear")
            if gray:
                e.forward_async_gray(k & 1, src, None, out_rgb=outs, out="net")
            else:
                e.forward_async_images(k & 1, src, None, out_rgb=outs, out="net")
            e.wait(k & 1)
            t = e.pipeline_times(k & 1)
            if r >= warmup:
                got[name]["h2d"].append(float(t[1] - t[0]))
                got[name]["compute"].append(float(t[3] - t[2]))
                got[name]["d2h"].append(float(t[5] - t[4]))
            k += 1
    e.set_ingest_filter("bilinear")
    res = {name: {stage: spread(v) for stage, v in stages.items()} for name, stages in got.items()}
    res["compute_on_minus_off"] = res["on"]["compute"]["median"] - res["off"]["compute"]["median"]
    res["source_mb"] = sum(a.nbytes for a in images) / 1e6
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--gray-batch", type=int, default=4)
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
    rs = np.random.RandomState(args.seed)
    e = engine.HipColorizer(H, W, max_batch=max(args.batch, args.gray_batch), precision=args.precision)
    e.load_state_dict(workloads.random_state_dict(0, "he"))
    res = {"precision": args.precision, "net": "%dx%d" % (H, W), "batch": args.batch, "gray_batch": args.gray_batch, "ms": {}}
    for sh, sw in ((203, 187), (1024, 768)):
        images = [rs.randint(0, 256, (sh, sw, 3)).astype(np.uint8) for _ in range(args.batch)]
        res["ms"]["%dx%d" % (sh, sw)] = spans(e, images, args.runs, args.warmup)
    planes = [rs.randint(0, 65536, (4000, 3000)).astype(np.uint16) for _ in range(args.gray_batch)]
    res["ms"]["gray4000x3000"] = spans(e, planes, args.runs, args.warmup)
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
