#!/usr/bin/env python3
"""What the temporal ab filter costs, on one box in one process (not a bench.py leg, no pass / fail number).  One batch of ``--batch`` RGB
images of the net's size, out='net', submitted alone, with the filter off and on:

  off    ``forward_async_images`` with the filter off: the yardstick, the parent's launches unchanged
  on     the same call under ``set_temporal_filter()``: the two kernels of idc_temporal.hip between the network and the Lab -> RGB epilogue

Per setting the compute span of ``idc_pipeline_times`` (end - start of the compute stage) and img/s = batch / (end of D2H - start of H2D).
The settings alternate on the two slots, one batch at a time (nothing else is in flight while a span is taken), ``--warmup`` untimed rounds
first, then ``--runs`` timed ones; median (min / max) in ms.  The frames are one image with seeded grain, so no frame is a cut and every one
but the first is blended.
The two kernels move 48 bytes a pixel and frame (diff: two L planes read, g written, 16; blend: x read and written, g read by both channels,
32); their time is the difference of the two compute medians, and the rate is given as a fraction of what a float4 device-to-device copy of
256 MiB reaches in the same process (the HIP runtime's own copy kernel).

usage: python tools/temporal_timing.py [--precision bf16] [--batch 32] [--size 256] [--runs 7] [--warmup 2] [--out f.json]
Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "runs": int(v.size)}


def copy_rate():
    """bytes / s (read + written) of a device-to-device copy of 256 MiB through the HIP runtime (its own vectorised copy kernel), median of 7;
    None where the runtime library cannot be loaded"""
    import ctypes
    hip = None
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = ctypes.CDLL(name)
            break
        except OSError:
            pass
    if hip is None:
        return None
    vp, nbytes = ctypes.c_void_p, 256 << 20
    a, b, e0, e1 = vp(), vp(), vp(), vp()
    hip.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    hip.hipMemcpyAsync.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
    hip.hipMemset.argtypes = [vp, ctypes.c_int, ctypes.c_size_t]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    hip.hipFree.argtypes = [vp]
    hip.hipEventDestroy.argtypes = [vp]
    if hip.hipMalloc(ctypes.byref(a), nbytes) or hip.hipMalloc(ctypes.byref(b), nbytes):
        return None
    ms = []
    try:
        if hip.hipEventCreate(ctypes.byref(e0)) or hip.hipEventCreate(ctypes.byref(e1)) or hip.hipMemset(a, 0, nbytes):
            return None
        for r in range(9):
            t = ctypes.c_float(0)
            if (hip.hipEventRecord(e0, None) or hip.hipMemcpyAsync(b, a, nbytes, 3, None) or hip.hipEventRecord(e1, None) or
                    hip.hipEventSynchronize(e1) or hip.hipEventElapsedTime(ctypes.byref(t), e0, e1)):
                return None
            if r >= 2:
                ms.append(t.value)
    finally:
        hip.hipFree(a), hip.hipFree(b)
        if e0:
            hip.hipEventDestroy(e0)
        if e1:
            hip.hipEventDestroy(e1)
    return 2.0 * nbytes / (float(np.median(ms)) * 1e-3)


def spans(e, images, runs, warmup):
    src = [e.pinned_empty(a.shape, np.uint8) for a in images]
    for s, a in zip(src, images):
        s[...] = a
    outs = [e.pinned_empty(a.shape, np.uint8) for a in images]
    got = {name: {"compute": [], "img_per_s": []} for name in ("off", "on")}
    cuts = None
    k = 0
    try:
        for r in range(warmup + runs):
            for name in ("off", "on"):
                if name == "on":
                    e.set_temporal_filter()
                    e.temporal_reset()
                else:
                    e.set_temporal_filter(None)
                e.forward_async_images(k & 1, src, None, out_rgb=outs, out="net")
                e.wait(k & 1)
                t = e.pipeline_times(k & 1)
                if name == "on":
                    cuts = int(e.temporal_info(k & 1, len(images))[0].sum())
                if r >= warmup:
                    got[name]["compute"].append(float(t[3] - t[2]))
                    got[name]["img_per_s"].append(len(images) / (float(t[5] - t[0]) * 1e-3))
                k += 1
    finally:
        e.set_temporal_filter(None)
    res = {name: {stage: spread(v) for stage, v in stages.items()} for name, stages in got.items()}
    res["on"]["frames_passed"] = cuts
    return res


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
    if args.runs < 5:
        ap.error("--runs: at least five timed runs")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    from interactive_deep_colorization_amd import engine, workloads
    H = W = args.size
    rs = np.random.RandomState(args.seed)
    e = engine.HipColorizer(H, W, max_batch=args.batch, precision=args.precision)
    e.load_state_dict(workloads.random_state_dict(0, "he"))
    base = rs.randint(40, 216, (H, W, 3)).astype(np.int16)
    images = [np.clip(base + rs.randint(-4, 5, base.shape), 0, 255).astype(np.uint8) for _ in range(args.batch)]
    res = {"precision": args.precision, "net": "%dx%d" % (H, W), "batch": args.batch, "ms": spans(e, images, args.runs, args.warmup)}
    e.close()
    added = res["ms"]["on"]["compute"]["median"] - res["ms"]["off"]["compute"]["median"]
    moved = 48 * args.batch * H * W
    rate = copy_rate()
    res["filter"] = {"added_compute_ms": added, "bytes_moved": moved, "bytes_per_s": moved / (added * 1e-3) if added > 0 else None,
                     "copy_bytes_per_s": rate, "fraction_of_copy": (moved / (added * 1e-3) / rate) if (rate and added > 0) else None}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
