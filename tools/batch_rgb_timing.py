#!/usr/bin/env python3
"""Images per second of three routes from uint8 photographs to colourised uint8 images, on one box in one process (not a bench.py leg,
no pass / fail number).

  (a) host colour work around the pipelined planes: per image the host resize to the net size and rgb2lab, ``forward_async`` on the two
      slots with pinned planes, then per image the host lab2rgb (for source-size output: the reference's get_img_fullres on the host --
      refresh output_ab through uint8, scipy zoom order 1, lab2rgb under the source's own L)
  (b) the blocking device route: ``set_image_rgb`` + ``forward_resident`` (+ ``fullres_rgb`` per image for source-size output)
  (c) ``colorize_stream``: ``idc_forward_async_rgb`` on the two slots

Two workloads at N = 32: 256 x 256 sources with net-size output and 512 x 384 sources with source-size output; no hints on any route.
A run is ``--batches`` batches through one route, ending in a synchronisation (every route hands back host arrays); the routes alternate,
``--warmup`` untimed rounds then ``--runs`` timed ones, and each rate is reported as its median with the minimum and maximum over the
runs.  Route (a) is bound by host numpy, so it runs ``--host-batches`` batches per run.  Also printed: the median compute span of
``idc_pipeline_times`` (compute end - compute start) for ``forward_async`` and for ``forward_async_rgb``, each over a pinned run of its
own on the two slots after two warm-up batches -- their
difference is the price of the prologue and epilogue kernels -- and the median H2D / D2H spans of the uint8 route.

usage: python tools/batch_rgb_timing.py [--precision bf16] [--batch 32] [--batches 8] [--host-batches 1] [--runs 7] [--warmup 2] [--out f.json]
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from interactive_deep_colorization_amd import colorspace, engine, workloads  # noqa: E402


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "runs": int(v.size)}


def host_fullres(src, out_ab, L_net):
    """The reference's get_img_fullres on the host (colorize_image.py:123-131 after :196-198)."""
    from scipy.ndimage import zoom
    rgb_net = colorspace.lab2rgb_transpose(L_net[None], out_ab.astype(np.float64))
    ab = colorspace.rgb2lab_transpose(rgb_net)[1:]
    sh, sw = src.shape[:2]
    ab_full = zoom(ab, (1, 1. * sh / ab.shape[1], 1. * sw / ab.shape[2]), order=1)
    return colorspace.lab2rgb_transpose(colorspace.rgb2lab(src)[..., 0][None], ab_full)


def workload(e, n, sh, sw, out, args):
    H, W = e.H, e.W
    rs = np.random.RandomState(sh + sw)
    batches = [rs.randint(0, 256, (n, sh, sw, 3)).astype(np.uint8) for _ in range(2)]      # two distinct batches, taken in turn
    for i in range(n):
        e.set_hints([], img=i)
    pin = [[e.pinned_empty((n, c, H, W)) for c in (1, 2, 1, 2)] for _ in range(2)]           # L, ab, mask, out per slot
    for arrs in pin:
        arrs[1][...] = 0
        arrs[2][...] = 0
    spans = {"planes": [], "rgb": [], "rgb_h2d": [], "rgb_d2h": []}

    def route_a(count):
        done = 0
        inflight = [None, None]

        def finish(slot):
            src, L_net = inflight[slot]
            e.wait(slot)
            ab = pin[slot][3]
            for i in range(n):
                if out == "source":
                    host_fullres(src[i], ab[i], L_net[i])
                else:
                    colorspace.lab2rgb_transpose(L_net[i][None], ab[i].astype(np.float64))
            inflight[slot] = None

        for k in range(count):
            slot = k & 1
            if inflight[slot] is not None:
                finish(slot)
            src = batches[k & 1]
            L_net = np.empty((n, H, W))
            for i in range(n):
                img = src[i] if (sh, sw) == (H, W) else colorspace.resize_bilinear_u8(src[i], H, W)
                L_net[i] = colorspace.rgb2lab(img)[..., 0]
            pin[slot][0][:, 0] = L_net - 50.0
            e.forward_async(slot, pin[slot][0], pin[slot][1], pin[slot][2], pin[slot][3], 0.0)
            inflight[slot] = (src, L_net)
            done += n
        for slot in (count & 1, (count + 1) & 1):
            if inflight[slot] is not None:
                finish(slot)
        return done

    def route_b(count):
        for k in range(count):
            e.set_image_rgb(batches[k & 1], keep_source=(out == "source"), want_rgb=False, want_lab=False)
            e.forward_resident(n, want_ab=False, want_lab=(out == "source"))
            if out == "source":
                for i in range(n):
                    e.fullres_rgb("output_ab", "linear", "image", img=i)
        return count * n

    def route_c(count):
        return sum(res.shape[0] for res in e.colorize_stream(((batches[k & 1], None) for k in range(count)), out=out))

    def plane_spans(count):
        """forward_async on the two slots with pinned planes, reading each batch's stamps."""
        for k in range(count + 2):
            slot = k & 1
            if k >= 2:
                e.wait(slot)
                if k >= 4:                      # the first two batches warm the slots up
                    t = e.pipeline_times(slot)
                    spans["planes"].append(float(t[3] - t[2]))
            if k < count:
                e.forward_async(slot, pin[slot][0], pin[slot][1], pin[slot][2], pin[slot][3], 0.0)

    def rgb_spans(count):
        """forward_async_rgb on the two slots with pinned buffers, reading each batch's stamps."""
        shape = (n, sh, sw, 3) if out == "source" else (n, H, W, 3)
        bufs = [(e.pinned_empty((n, sh, sw, 3), np.uint8), e.pinned_empty(shape, np.uint8)) for _ in range(2)]
        for k in range(2):
            bufs[k][0][...] = batches[k]
        for k in range(count + 2):
            slot = k & 1
            if k >= 2:
                e.wait(slot)
                t = e.pipeline_times(slot)
                if k >= 4:                      # the first two batches warm the slots up
                    spans["rgb"].append(float(t[3] - t[2]))
                    spans["rgb_h2d"].append(float(t[1] - t[0]))
                    spans["rgb_d2h"].append(float(t[5] - t[4]))
            if k < count:
                e.forward_async_rgb(slot, bufs[slot][0], None, bufs[slot][1], out=out)

    rates = {"a": [], "b": [], "c": []}
    for r in range(args.warmup + args.runs):
        for name, fn, count in (("a", route_a, args.host_batches), ("b", route_b, args.batches), ("c", route_c, args.batches)):
            t0 = time.perf_counter()
            images = fn(count)
            dt = time.perf_counter() - t0
            if r >= args.warmup:
                rates[name].append(images / dt)
    plane_spans(max(args.batches, 6))
    rgb_spans(max(args.batches, 6))
    res = {"sources": "%dx%d" % (sh, sw), "output": out, "n": n,
           "a_host_colour_forward_async_img_per_s": spread(rates["a"]),
           "b_set_image_rgb_forward_resident_img_per_s": spread(rates["b"]),
           "c_colorize_stream_img_per_s": spread(rates["c"]),
           "compute_span_forward_async_ms": spread(spans["planes"]),
           "compute_span_forward_async_rgb_ms": spread(spans["rgb"]),
           "h2d_span_forward_async_rgb_ms": spread(spans["rgb_h2d"]),
           "d2h_span_forward_async_rgb_ms": spread(spans["rgb_d2h"])}
    res["compute_span_difference_ms"] = res["compute_span_forward_async_rgb_ms"]["median"] - res["compute_span_forward_async_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--host-batches", type=int, default=1)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=256, help="net size (a smaller one only to rehearse the script)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    e = engine.HipColorizer(args.size, args.size, max_batch=args.batch, precision=args.precision)
    e.load_state_dict(workloads.random_state_dict(0, "he"))
    res = {"precision": args.precision, "batches_per_run": args.batches, "host_batches_per_run": args.host_batches, "runs": args.runs,
           "warmup": args.warmup, "net": "%dx%d" % (args.size, args.size),
           "workloads": [workload(e, args.batch, args.size, args.size, "net", args),
                         workload(e, args.batch, args.size * 2, args.size * 3 // 2, "source", args)]}
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
