#!/usr/bin/env python3
"""Host-clock timing of the colour picker's maths (lab_gamut) on the host route against the device route (not a bench.py leg).

Every comparison alternates the two routes in ONE process: 5 warm-up pairs, then the median (and the 10th / 90th percentile) of 50 timed
pairs.  Each timed call is blocking: the device route's ends in the library's own stream synchronisation, after the result has reached
the host, so the figure is what a GUI thread waits for.

  update_gamut   abGrid(110, 1).update_gamut(50): 221 x 221 points
  snap_ab        one colour (255, 0, 255) at L = 50
  snap_ab_many   256 seeded (L, colour) pairs in one call

The device route needs a handle but no weights (64 x 64, bf16).

usage: python tools/gamut_timing.py [--calls 50] [--warmup 5] [--out result.json]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from interactive_deep_colorization_amd import engine, lab_gamut  # noqa: E402


def alternate(fn, eng, calls, warmup):
    """fn() on the host route and with `eng` bound, alternating: {host_ms, device_ms} medians with p10 / p90 of `calls` timed pairs."""
    acc = {None: [], eng: []}
    try:
        for k in range(warmup + calls):
            for route in (None, eng):
                lab_gamut.set_engine(route)
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if k >= warmup:
                    acc[route].append(dt * 1e3)
    finally:
        lab_gamut.set_engine(None)
    out = {}
    for name, ts in (("host", acc[None]), ("device", acc[eng])):
        out[name + "_ms"] = float(np.median(ts))
        out[name + "_p10_p90_ms"] = [float(np.percentile(ts, 10)), float(np.percentile(ts, 90))]
    out["ratio"] = out["host_ms"] / out["device_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 50:
        ap.error("--calls must be at least 50")
    eng = engine.HipColorizer(64, 64, max_batch=1, precision="bf16")
    rs = np.random.RandomState(0)
    ls, rgbs = rs.uniform(0, 100, 256), rs.randint(0, 256, (256, 3)).astype(np.uint8)
    grid = lab_gamut.abGrid(110, 1)
    colour = np.array([255, 0, 255], np.uint8)
    res = {"calls": args.calls, "warmup": args.warmup}
    res["update_gamut_221x221"] = alternate(lambda: grid.update_gamut(50.0), eng, args.calls, args.warmup)
    res["snap_ab_1"] = alternate(lambda: lab_gamut.snap_ab(50.0, colour), eng, args.calls, args.warmup)
    res["snap_ab_many_256"] = alternate(lambda: lab_gamut.snap_ab_many(ls, rgbs), eng, args.calls, args.warmup)
    # the two routes computed the same thing (the device's last bits may move a value across an edge: tests/test_gamut_gpu.py has the bars)
    host = lab_gamut.snap_ab_many(ls, rgbs)
    lab_gamut.set_engine(eng)
    dev = lab_gamut.snap_ab_many(ls, rgbs)
    lab_gamut.set_engine(None)
    res["snap_ab_many_256"]["values_differing"] = int((host != dev).sum())
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
