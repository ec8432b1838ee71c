#!/usr/bin/env python3
"""What the motion compensation of the temporal ab filter costs, on one box (not a bench.py leg, no pass / fail number).  One batch of
``--batch`` RGB images of the net's size, out='net', submitted alone, the temporal filter on in every leg:

  plain   motion off: the two launches of idc_temporal.hip, the parent's
  s4      ``set_temporal_motion(search=4)``: idc_motion.hip's search, diff and one blend launch per frame, and the two state copies
  s7      the same at search 7 (225 candidates a block)

Per leg the compute span of ``idc_pipeline_times`` (end - start of the compute stage) and img/s = batch / (end of D2H - start of H2D).  The
legs alternate on the two slots, one batch at a time (nothing else is in flight while a span is taken), ``--warmup`` untimed rounds first,
then ``--runs`` timed ones; median (min / max) in ms.  The frames are crops of one noise image, the window moving (1, 2) pixels a frame, so
the search has a pan to find and every frame but the first is blended (cut = 0).

``--trace DIR``: BEFORE any of that, one ``rocprofv3 --kernel-trace`` run of a child of its own (this script with --child: s4 then s7,
warm-up and runs as above, nothing else) writes its database under DIR; the three kernels' own times are read from it per leg, per launch
(the blend: per frame, and summed over the call).  Tracing slows the host, so the spans above are taken with the profiler off.

usage: python tools/motion_timing.py [--precision bf16] [--batch 32] [--size 256] [--runs 7] [--warmup 2] [--trace DIR] [--out f.json]
Prints one JSON object."""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys

import numpy as np

LEGS = (("plain", None), ("s4", 4), ("s7", 7))
KERNELS = ("motion_search_kernel", "motion_diff_kernel", "motion_blend_kernel")


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "runs": int(v.size)}


def frames(size, batch, seed):
    rs = np.random.RandomState(seed)
    big = rs.randint(0, 256, (size + batch, size + 2 * batch, 3)).astype(np.uint8)
    return [np.ascontiguousarray(big[f:f + size, 2 * f:2 * f + size]) for f in range(batch)]


def engine_for(args):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    from interactive_deep_colorization_amd import engine, workloads
    e = engine.HipColorizer(args.size, args.size, max_batch=args.batch, precision=args.precision)
    e.load_state_dict(workloads.random_state_dict(0, "he"))
    return e


def one_call(e, k, search, src, outs):
    if search is None:
        e.set_temporal_motion(None)
    else:
        e.set_temporal_motion(search=search)
    e.temporal_reset()
    e.forward_async_images(k & 1, src, None, out_rgb=outs, out="net")
    e.wait(k & 1)
    return e.pipeline_times(k & 1)


def spans(e, images, runs, warmup, legs, alternate=True):
    src = [e.pinned_empty(a.shape, np.uint8) for a in images]
    for s, a in zip(src, images):
        s[...] = a
    outs = [e.pinned_empty(a.shape, np.uint8) for a in images]
    got = {name: {"compute": [], "img_per_s": []} for name, _ in legs}
    info = {}
    k = 0
    e.set_temporal_filter(cut=0.0)
    try:
        order = [(r, leg) for r in range(warmup + runs) for leg in legs] if alternate else [(r, leg) for leg in legs for r in range(warmup + runs)]
        for r, (name, search) in order:
            t = one_call(e, k, search, src, outs)
            if search is not None:
                v = e.temporal_vectors(k & 1, len(images))
                info[name] = {"blocks_with_the_pan": float((v[1:, 1:-1, 1:-1] == np.array([1, 2], np.int8)).all(-1).mean()) if search >= 2 else None,
                              "frames_passed": int(e.temporal_info(k & 1, len(images))[0].sum())}
            if r >= warmup:
                got[name]["compute"].append(float(t[3] - t[2]))
                got[name]["img_per_s"].append(len(images) / (float(t[5] - t[0]) * 1e-3))
            k += 1
    finally:
        e.set_temporal_motion(None)
        e.set_temporal_filter(None)
    res = {name: {stage: spread(v) for stage, v in stages.items()} for name, stages in got.items()}
    for name, extra in info.items():
        res[name].update(extra)
    return res


def traced(args):
    """One rocprofv3 --kernel-trace run of a child of this script -> per leg and kernel the launches' own times in microseconds."""
    os.makedirs(args.trace, exist_ok=True)
    child = [sys.executable, os.path.abspath(__file__), "--child", "--precision", args.precision, "--batch", str(args.batch), "--size", str(args.size),
             "--runs", str(args.runs), "--warmup", str(args.warmup), "--seed", str(args.seed)]
    subprocess.run(["rocprofv3", "--kernel-trace", "-d", args.trace, "-o", "motion", "--"] + child, check=True, stdout=subprocess.DEVNULL)
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
        per_call = args.batch if kern == "motion_blend_kernel" else 1
        if len(d) != 2 * per_leg * per_call:
            raise RuntimeError("%s: %d dispatches in the trace, %d expected" % (kern, len(d), 2 * per_leg * per_call))
        for i, name in enumerate(("s4", "s7")):           # the child runs s4 to the end, then s7
            mine = np.asarray(d[i * per_leg * per_call:(i + 1) * per_leg * per_call]).reshape(per_leg, per_call)[args.warmup:]
            out.setdefault(name, {})[kern] = {"launches_per_call": per_call, "per_launch_us": spread(mine.reshape(-1)),
                                              "per_call_us": spread(mine.sum(axis=1))}
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
    ap.add_argument("--child", action="store_true", help="(the traced child: the two motion legs one after the other, no output)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: at least five timed runs")
    images = frames(args.size, args.batch, args.seed)
    if args.child:
        e = engine_for(args)
        spans(e, images, args.runs, args.warmup, LEGS[1:], alternate=False)
        e.close()
        return
    trace = traced(args) if args.trace else None          # first: this process has not opened the device yet
    e = engine_for(args)
    res = {"precision": args.precision, "net": "%dx%d" % (args.size, args.size), "batch": args.batch,
           "ms": spans(e, images, args.runs, args.warmup, LEGS)}
    e.close()
    base = res["ms"]["plain"]["compute"]["median"]
    res["motion"] = {name: {"added_compute_ms": res["ms"][name]["compute"]["median"] - base} for name in ("s4", "s7")}
    if trace:
        res["trace"] = trace
        for name in ("s4", "s7"):
            kernels_ms = sum(trace["kernels"][name][k]["per_call_us"]["median"] for k in KERNELS) * 1e-3
            res["motion"][name]["kernels_ms"] = kernels_ms
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
