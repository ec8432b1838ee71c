#!/usr/bin/env python3
"""What scoring on the device (``idc_forward_async_eval``) costs and buys, on one box in one process (not a bench.py leg, no pass / fail
number).  A stream of ``--count`` ground-truth images, ``--points`` simulated points each (``evaluate.simulate_points``), net-size output.

  colorize  ``colorize_images(out='net', mode='ab')``: what scoring needed before -- the hint colours come from the host (computed before the
            clock starts: the host's share is NOT in this figure), every colourised image comes back, and the caller would still have to
            square-sum it.  The call is unchanged by the evaluation batches, so this leg is the parent's.
  evaluate  ``evaluate_images(out='net', mode='reveal')``: the colours are revealed and the result is scored on the device; 24 bytes per image
            come back.
Images per second = images / wall time of the whole stream, ending in the wait for the last batch.  The two legs alternate ``--rounds``
times after one untimed pass each, so that each figure comes with its own run-to-run spread.  Sources: ``--sources uniform`` (203 x 187) or
``mixed`` (sides drawn once from 64..512); 37 distinct images with their own points, repeated along the stream.

  compute   the compute span of ``idc_pipeline_times`` (compute end - compute start) of one batch through ``forward_async_images`` in 'ab'
            mode and through ``forward_async_eval`` in 'reveal' mode with the same rectangles: the difference is the reveal, ground-truth and
            score kernels together.
  sweep     (``--sweep``) one ``evaluate.psnr_sweep`` table per precision of ``--sweep`` (comma separated) on 8 crops of the golden photograph:
            a usage example -- the values depend on the weights, which here are random.

usage: python tools/eval_timing.py [--precision bf16] [--batch 32] [--size 256] [--count 8192] [--points 10] [--rounds 3] [--sources uniform]
                                   [--sweep bf16,fp16x3] [--out f.json]
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "runs": int(v.size)}


def host_hints(colorspace, img, rects, H, W):
    """The rows ``colorize_images`` needs for the same simulated user: mean ab of the net-size image under each clipped rectangle, on the host."""
    lab = colorspace.rgb2lab(colorspace.resize_bilinear_u8(img, H, W))
    rows = []
    for y0, x0, y1, x1 in rects:
        cy0, cx0, cy1, cx1 = max(y0, 0), max(x0, 0), min(y1, H - 1), min(x1, W - 1)
        if cy0 > cy1 or cx0 > cx1:
            continue
        a, b = lab[cy0:cy1 + 1, cx0:cx1 + 1, 1:].reshape(-1, 2).mean(0)
        rows.append((int(y0), int(x0), int(y1), int(x1), float(a), float(b)))
    return rows


def compute_spans(e, images, rects, hints, batches):
    """Median compute span of one batch: forward_async_images('ab') and forward_async_eval('reveal'), alternating on the two slots."""
    spans = {"images_ab": [], "eval_reveal": []}
    for k in range(2 * (batches + 1)):
        if k & 1:
            e.forward_async_eval(1, images, rects, mode="reveal", out="net")
        else:
            e.forward_async_images(0, images, hints, mode="ab", out="net")
        e.wait(k & 1)
        t = e.pipeline_times(k & 1)
        if k >= 2:
            spans["eval_reveal" if k & 1 else "images_ab"].append(float(t[3] - t[2]))
    return {k: spread(v) for k, v in spans.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256, help="net size (a smaller one only to rehearse the script)")
    ap.add_argument("--count", type=int, default=8192, help="images in the stream (about a second per pass at the bf16 rate)")
    ap.add_argument("--points", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sources", default="uniform", choices=["uniform", "mixed"])
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--sweep", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    from interactive_deep_colorization_amd import colorspace, engine, evaluate, workloads
    H = W = args.size
    rs = np.random.RandomState(args.seed)
    # 37 distinct images, reused along the stream (37: no batch of 32 repeats the one before)
    sizes = [(203, 187)] * 37 if args.sources == "uniform" else [(int(rs.randint(64, 513)), int(rs.randint(64, 513))) for _ in range(37)]
    base = [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in sizes]
    points = [evaluate.simulate_points(H, W, args.points, np.random.RandomState(args.seed + j)) for j in range(37)]
    given = [host_hints(colorspace, a, r, H, W) for a, r in zip(base, points)]
    images, rects, hints = [[v[j % 37] for j in range(args.count)] for v in (base, points, given)]
    e = engine.HipColorizer(H, W, max_batch=args.batch, precision=args.precision)
    e.load_state_dict(workloads.random_state_dict(0, "he"))

    def colorize():
        t0 = time.perf_counter()
        n = sum(1 for _ in e.colorize_images(zip(images, hints), batch=args.batch, out="net", mode="ab"))
        return n / (time.perf_counter() - t0)

    def evaluate_leg():
        t0 = time.perf_counter()
        n = sum(1 for _ in e.evaluate_images(zip(images, rects), batch=args.batch, out="net", mode="reveal"))
        return n / (time.perf_counter() - t0)

    colorize(); evaluate_leg()                                      # untimed: code objects, buffers, the pinned pool
    rates = {"colorize_images": [], "evaluate_images": []}
    for _ in range(args.rounds):
        rates["colorize_images"].append(colorize())
        rates["evaluate_images"].append(evaluate_leg())
    res = {"precision": args.precision, "net": "%dx%d" % (H, W), "batch": args.batch, "images": args.count, "points": args.points,
           "sources": args.sources, "img_per_s": {k: spread(v) for k, v in rates.items()},
           "compute_ms": compute_spans(e, images[:args.batch], rects[:args.batch], hints[:args.batch], 12)}
    e.close()
    if args.sweep:
        mortar = np.load(os.path.join(repo, "tests", "golden", "mortar_pestle_256_rgb.npy"))
        crops = [np.ascontiguousarray(mortar[y:y + 160, x:x + 160]) for y in (0, 96) for x in (0, 32, 64, 96)]
        res["sweep"] = {"counts": [0, 1, 2, 5, 10, 20, 50, 100], "images": len(crops), "mean_psnr_db": {}}
        for precision in args.sweep.split(","):
            s = engine.HipColorizer(H, W, max_batch=8, precision=precision)
            s.load_state_dict(workloads.random_state_dict(0, "he"))
            table = evaluate.psnr_sweep(s, crops, counts=res["sweep"]["counts"], seed=0)
            res["sweep"]["mean_psnr_db"][precision] = [round(float(v), 4) for v in table.mean(1)]
            s.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
