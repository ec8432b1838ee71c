#!/usr/bin/env python3
"""Host-clock timing of image ingestion on the device against the host route the library also keeps (not a bench.py leg).

Every comparison alternates the two routes in ONE process: 3 warm-up pairs, then the median of 20 timed pairs, each timed call ending in a
synchronisation of its own (the calls are blocking).

  load      ColorizeImageTorch.load_image (host resize + two float64 rgb2lab) vs load_image_device (idc_set_image_rgb, full-resolution
            Lab deferred), for a 256 x 256 and a 1080 x 1920 PNG (both routes pay the same PNG decode)
  fullres   get_img_fullres of the 1080 x 1920 image: idc_upsample_lab2rgb with the float64 L plane from the host vs idc_fullres_rgb
            from the resident uint8 source
  batch     images per second of set_image_rgb(n = 32) + forward_resident(32) with rgb out, against host rgb2lab of the same 32 uint8
            images + forward_rgb

usage: python tools/ingest_timing.py [--precision bf16] [--pairs 20] [--warmup 3] [--out result.json]
Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from interactive_deep_colorization_amd import api, colorspace, engine, workloads  # noqa: E402


def alternate(route_a, route_b, pairs, warmup):
    """Median seconds of each route over `pairs` alternating runs after `warmup` untimed pairs."""
    ta, tb = [], []
    for k in range(warmup + pairs):
        for fn, acc in ((route_a, ta), (route_b, tb)):
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if k >= warmup:
                acc.append(dt)
    return float(np.median(ta)), float(np.median(tb))


def png(directory, h, w, seed):
    from PIL import Image
    path = os.path.join(directory, "src_%dx%d.png" % (h, w))
    Image.fromarray(np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)).save(path)
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sd = workloads.random_state_dict(0, "he")
    res = {"precision": args.precision, "pairs": args.pairs, "warmup": args.warmup}
    with tempfile.TemporaryDirectory() as tmp:
        def model():
            m = api.ColorizeImageTorch(Xd=256, precision=args.precision)
            m.prep_net(path="", state_dict=sd)
            return m
        host, dev = model(), model()
        for (h, w) in ((256, 256), (1080, 1920)):
            path = png(tmp, h, w, h)
            a, b = alternate(lambda: host.load_image(path), lambda: dev.load_image_device(path), args.pairs, args.warmup)
            t0 = time.perf_counter()
            colorspace.imread_rgb(path)
            res["load_%dx%d" % (h, w)] = {"load_image_ms": a * 1e3, "load_image_device_ms": b * 1e3, "png_decode_ms": (time.perf_counter() - t0) * 1e3}
        # both objects now hold the 1080 x 1920 image; one click each, then the full-resolution getter
        hab, hm = workloads.hints_config2(256, 5, 3, 0)
        host.net_forward(hab, hm)
        dev.net_forward(hab, hm)
        _ = host.img_l_fullres
        a, b = alternate(host.get_img_fullres, dev.get_img_fullres, args.pairs, args.warmup)
        assert dev._src_resident and not host._src_resident
        res["fullres_1080x1920"] = {"upsample_lab2rgb_host_L_ms": a * 1e3, "fullres_rgb_ms": b * 1e3}
        host.net.close()
        dev.net.close()
    n = args.batch
    e = engine.HipColorizer(256, 256, max_batch=n, precision=args.precision)
    e.load_state_dict(sd)
    imgs = np.random.RandomState(1).randint(0, 256, (n, 256, 256, 3)).astype(np.uint8)
    ab, mask = np.zeros((n, 2, 256, 256), np.float32), np.zeros((n, 1, 256, 256), np.float32)      # no hints on either side
    for i in range(n):
        e.set_hints([], img=i)

    def host_route():
        L = (colorspace.rgb2lab(imgs)[..., 0] - 50.0)[:, None]
        e.forward_rgb(L, ab, mask, want_lab=False)

    def device_route():
        e.set_image_rgb(imgs, want_rgb=False, want_lab=False)
        e.forward_resident(n, want_lab=False)

    a, b = alternate(host_route, device_route, args.pairs, args.warmup)
    res["batch_%d" % n] = {"host_rgb2lab_forward_rgb_img_per_s": n / a, "set_image_rgb_forward_resident_img_per_s": n / b}
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
