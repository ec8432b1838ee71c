#!/usr/bin/env python3
"""What the hint tracking along the motion vectors costs, on one box (not a bench.py leg, no pass / fail number).  One batch of ``--batch``
RGB images of the net's size, out='net', submitted alone, the temporal filter and motion compensation (search 4) on in both legs:

  motion  tracking off: the parent's launches, unchanged and in the parent's order (network, then search, diff, one blend a frame)
  track   ``set_hint_tracking()``: the search in front of the network, ONE launch of idc_track.hip's kernel for all frames, three state copies,
          the network on the tracked planes; run_temporal then skips its search

Per leg the compute span of ``idc_pipeline_times`` (end - start of the compute stage) and img/s = batch / (end of D2H - start of H2D).  The
legs alternate on the two slots, one batch at a time (nothing else is in flight while a span is taken), ``--warmup`` untimed rounds first,
then ``--runs`` timed ones; median (min / max) in ms.  The frames are crops of one noise image, the window moving (1, 2) pixels a frame, and
frame 0 alone is hinted (four rectangles): along the pan L repeats exactly, so no walk is cut short by ``tol`` -- a pixel of frame f without
a hint behind it walks all f frames back and the carried hints live to the last frame: the longest walks the rule allows.

``--trace DIR``: BEFORE any of that, one ``rocprofv3 --kernel-trace`` run of a child of its own (this script with --child: the track leg alone,
warm-up and runs as above) writes its database under DIR; the tracking kernel's and the search kernel's own times are read from it.
Tracing slows the host, so the spans above are taken with the profiler off.

usage: python tools/track_timing.py [--precision bf16] [--batch 32] [--size 256] [--runs 7] [--warmup 2] [--trace DIR] [--out f.json]
Prints one JSON object."""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys

import numpy as np

LEGS = (("motion", False), ("track", True))
KERNELS = ("track_hints_kernel", "motion_search_kernel")


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "runs": int(v.size)}


def frames(size, batch, seed):
    rs = np.random.RandomState(seed)
    big = rs.randint(0, 256, (size + batch, size + 2 * batch, 3)).astype(np.uint8)
    return [np.ascontiguousarray(big[f:f + size, 2 * f:2 * f + size]) for f in range(batch)]


def first_frame_hints(size, batch):
    q = size // 4
    rects = [(q + 3, 3 * q - 20, q + 18, 3 * q + 5, 40.0, -30.0), (2 * q, 2 * q, 2 * q + 11, 2 * q + 30, -20.0, 50.0),
             (3 * q - 9, 3 * q - 9, 3 * q + 9, 3 * q + 9, 10.0, 10.0), (size - 12, size - 40, size - 5, size - 9, 60.0, 0.0)]
    return [rects] + [None] * (batch - 1)


def engine_for(args):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    from interactive_deep_colorization_amd import engine, workloads
    e = engine.HipColorizer(args.size, args.size, max_batch=args.batch, precision=args.precision)
    e.load_state_dict(workloads.random_state_dict(0, "he"))
    return e


def one_call(e, k, track, src, hints, outs):
    if track:
        e.set_hint_tracking()
    else:
        e.set_hint_tracking(None)
    e.temporal_reset()
    e.forward_async_images(k & 1, src, hints, out_rgb=outs, out="net")
    e.wait(k & 1)
    return e.pipeline_times(k & 1)


def spans(e, images, hints, runs, warmup, legs):
    src = [e.pinned_empty(a.shape, np.uint8) for a in images]
    for s, a in zip(src, images):
        s[...] = a
    outs = [e.pinned_empty(a.shape, np.uint8) for a in images]
    got = {name: {"compute": [], "img_per_s": []} for name, _ in legs}
    info = {}
    k = 0
    e.set_temporal_filter(cut=0.0)
    e.set_temporal_motion(search=4)
    try:
        for r in range(warmup + runs):
            for name, track in legs:
                t = one_call(e, k, track, src, hints, outs)
                if track and r == warmup + runs - 1:     # (16 MB from the device: once, behind the last span)
                    mask, age = e.tracked_hints(k & 1, len(images), want=("mask", "age"))[1:]
                    info[name] = {"hinted_pixels_frame0": int((mask[0] != 0).sum()), "hinted_pixels_last_frame": int((mask[-1] != 0).sum()),
                                  "oldest_age": int(age.max())}
                if r >= warmup:
                    got[name]["compute"].append(float(t[3] - t[2]))
                    got[name]["img_per_s"].append(len(images) / (float(t[5] - t[0]) * 1e-3))
                k += 1
    finally:
        e.set_hint_tracking(None)
        e.set_temporal_motion(None)
        e.set_temporal_filter(None)
    res = {name: {stage: spread(v) for stage, v in stages.items()} for name, stages in got.items()}
    for name, extra in info.items():
        res[name].update(extra)
    return res


def traced(args):
    """One rocprofv3 --kernel-trace run of a child of this script -> per kernel the launches' own times in microseconds."""
    os.makedirs(args.trace, exist_ok=True)
    child = [sys.executable, os.path.abspath(__file__), "--child", "--precision", args.precision, "--batch", str(args.batch), "--size", str(args.size),
             "--runs", str(args.runs), "--warmup", str(args.warmup), "--seed", str(args.seed)]
    subprocess.run(["rocprofv3", "--kernel-trace", "-d", args.trace, "-o", "track", "--"] + child, check=True, stdout=subprocess.DEVNULL)
    dbs = sorted(glob.glob(os.path.join(args.trace, "**", "*.db"), recursive=True), key=os.path.getmtime)
    if not dbs:
        raise RuntimeError("rocprofv3 left no database under %s" % args.trace)
    con = sqlite3.connect(dbs[-1])
    rows = list(con.execute("select name, duration from kernels order by start"))
    con.close()
    out = {}
    per_leg = args.warmup + args.runs
    for kern in KERNELS:
        d = [float(r[1]) / 1e3 for r in rows if kern in r[0]]
        if len(d) != per_leg:
            raise RuntimeError("%s: %d dispatches in the trace, %d expected (one a call)" % (kern, len(d), per_leg))
        out[kern] = {"launches_per_call": 1, "per_call_us": spread(d[args.warmup:])}
    return {"database": os.path.relpath(dbs[-1], args.trace), "kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256, help="net size (a smaller one only to rehearse the script)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--trace", default=None, help="directory for one rocprofv3 --kernel-trace run of a child of this script")
    ap.add_argument("--child", action="store_true", help="(the traced child: the track leg alone, no output)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: at least five timed runs")
    images = frames(args.size, args.batch, args.seed)
    hints = first_frame_hints(args.size, args.batch)
    if args.child:
        e = engine_for(args)
        spans(e, images, hints, args.runs, args.warmup, LEGS[1:])
        e.close()
        return
    trace = traced(args) if args.trace else None          # first: this process has not opened the device yet
    e = engine_for(args)
    res = {"precision": args.precision, "net": "%dx%d" % (args.size, args.size), "batch": args.batch,
           "ms": spans(e, images, hints, args.runs, args.warmup, LEGS)}
    e.close()
    on, off = res["ms"]["track"]["compute"], res["ms"]["motion"]["compute"]
    res["tracking"] = {"added_compute_ms": on["median"] - off["median"]}
    if trace:
        res["trace"] = trace
        res["tracking"]["kernel_ms"] = trace["kernels"]["track_hints_kernel"]["per_call_us"]["median"] * 1e-3
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
