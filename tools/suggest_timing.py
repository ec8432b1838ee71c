#!/usr/bin/env python3
"""What the distribution batches cost, on one box in one process (not a bench.py leg, no pass / fail number).  Three measurements:

  suggestions  ``--queries`` (256) colour suggestions at random pixels of a resident distribution: one ``suggest_colors_batch`` call against
               that many ``suggest_colors`` calls (the parent's route: two stream synchronisations and four blocking copies around a
               one-workgroup launch each).  Wall time of the blocking calls, host clock; the two legs alternate ``--rounds`` times after one
               untimed pass each.  The results of the two routes are compared bit for bit before anything is timed.
  stream       images per second of ``suggest_images`` (P = ``--peaks`` peaks per image, suggestions at the peaks, N = ``--draws`` draws, K = 5)
               against ``colorize_images`` on the SAME engine (so both pay the same network except for the head), net-size output, a stream
               of ``--count`` images: the price of the head plus the taps.  Wall time of the whole stream, ending in the wait for the last
               batch; alternating legs.  With it the compute span of one batch (``idc_pipeline_times``) through ``forward_async_images`` and
               through ``forward_async_dist`` with no taps (the head alone), with the peaks only, and with peaks and suggestions.
  picker       the uncertainty picker alone at its worst case, the 313 head's full-resolution grid at P = ``--worst-peaks`` (64): blocking
               ``dist_peaks`` (entropy launch + picker + copy back) minus blocking ``dist_entropy`` (entropy launch + copy back) on the same
               resident distribution, per call for ``--batch313`` images and for one.

usage: python tools/suggest_timing.py [--precision bf16] [--batch 32] [--size 256] [--count 2048] [--peaks 8] [--draws 32] [--queries 256]
                                      [--rounds 5] [--worst-peaks 64] [--batch313 4] [--out f.json]
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


def grid529():
    axis = np.arange(-110, 120, 10)
    return np.ascontiguousarray(np.array(np.meshgrid(axis, axis)).reshape((2, 529)).T.astype(np.float32))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256, help="net size (a smaller one only to rehearse the script)")
    ap.add_argument("--count", type=int, default=2048, help="images in the stream")
    ap.add_argument("--peaks", type=int, default=8)
    ap.add_argument("--draws", type=int, default=32)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--worst-peaks", type=int, default=64)
    ap.add_argument("--batch313", type=int, default=4)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    from interactive_deep_colorization_amd import engine, workloads
    from oracle import weights
    H = W = args.size
    rs = np.random.RandomState(args.seed)
    base = [rs.randint(0, 256, (203, 187, 3)).astype(np.uint8) for _ in range(37)]      # 37: no batch of 32 repeats the one before
    images = [base[j % 37] for j in range(args.count)]
    centres = grid529()
    res = {"precision": args.precision, "net": "%dx%d" % (H, W), "batch": args.batch, "images": args.count, "peaks": args.peaks,
           "draws": args.draws, "queries": args.queries}

    e = engine.HipColorizer(H, W, max_batch=args.batch, precision=args.precision, dist=True)
    e.load_state_dict(workloads.random_state_dict(0, "he"))
    # ---- suggestions: one batched call against one call per pixel, on the distribution of one resident batch
    nres = min(args.batch, 8)
    for i in range(nres):
        e.set_image_rgb(base[i], img=i, want_rgb=False, want_lab=False)
    e.forward_resident(nres, want_ab=False, want_rgb=False)
    queries = [(int(rs.randint(0, nres)), int(rs.randint(0, H)), int(rs.randint(0, W)), 1000 + q) for q in range(args.queries)]

    def one_by_one():
        return [e.suggest_colors(y, x, centres, K=5, N_draws=25000, seed=s, img=i) for i, y, x, s in queries]

    def batched():
        return e.suggest_colors_batch(queries, centres, K=5, N_draws=25000)

    singles, (bc, bf) = one_by_one(), batched()                     # untimed, and the same bits
    same = all(bc[q].tobytes() == c.tobytes() and bf[q].tobytes() == f.tobytes() for q, (c, f) in enumerate(singles))
    ms = {"suggest_colors_x%d" % args.queries: [], "suggest_colors_batch": []}
    for _ in range(args.rounds):
        ms["suggest_colors_x%d" % args.queries].append(1e3 * timed(one_by_one))
        ms["suggest_colors_batch"].append(1e3 * timed(batched))
    res["suggestions"] = {"bit_identical": bool(same), "N_draws": 25000, "K": 5, "ms": {k: spread(v) for k, v in ms.items()}}

    # ---- the stream: colourise alone against colourise + head + peaks + suggestions at the peaks
    def colorize():
        t0 = time.perf_counter()
        n = sum(1 for _ in e.colorize_images(images, batch=args.batch, out="net"))
        return n / (time.perf_counter() - t0)

    def suggest():
        t0 = time.perf_counter()
        n = sum(1 for _ in e.suggest_images(images, centres, batch=args.batch, out="net", peaks=args.peaks, radius=2, K=5, N_draws=args.draws))
        return n / (time.perf_counter() - t0)

    colorize(); suggest()                                           # untimed: code objects, buffers, the pinned pool
    rates = {"colorize_images": [], "suggest_images": []}
    for _ in range(args.rounds):
        rates["colorize_images"].append(colorize())
        rates["suggest_images"].append(suggest())
    res["img_per_s"] = {k: spread(v) for k, v in rates.items()}
    group = images[:args.batch]
    legs = {"images": lambda s: e.forward_async_images(s, group, None, out="net"),
            "dist_head_only": lambda s: e.forward_async_dist(s, group, None, want_rgb=True, peaks=0),
            "dist_peaks": lambda s: e.forward_async_dist(s, group, None, want_rgb=True, peaks=args.peaks, radius=2, skip_hints=True),
            "dist_peaks_suggest": lambda s: e.forward_async_dist(s, group, None, want_rgb=True, peaks=args.peaks, radius=2, skip_hints=True,
                                                                 queries="peaks", K=5, N_draws=args.draws, centres=centres)}
    spans = {k: [] for k in legs}
    for k in range(13):                                             # the first round untimed; one batch in flight at a time
        for name, fn in legs.items():
            fn(0)
            e.wait(0)
            t = e.pipeline_times(0)
            if k:
                spans[name].append(float(t[3] - t[2]))
    res["compute_ms"] = {k: spread(v) for k, v in spans.items()}
    e.close()

    # ---- the picker alone, worst case: the 313 head's full-resolution grid
    n3 = args.batch313
    sd = weights.add_pred313_head(weights.make_state_dict(2, "he", include_class=False), 2)
    e3 = engine.HipColorizer(H, W, max_batch=n3, precision=args.precision, dist313=True)
    e3.load_state_dict(sd)
    e3.keep_dist(True)
    for i in range(n3):
        e3.set_image_rgb(base[i], img=i, want_rgb=False, want_lab=False)
    e3.forward_resident(n3, want_ab=False, want_rgb=False)
    picker = {}
    for n in sorted({1, n3}):
        e3.dist_entropy(n); e3.dist_peaks(n, P=args.worst_peaks, radius=2)
        ent, both = [], []
        for _ in range(max(args.rounds, 5)):
            ent.append(1e3 * timed(lambda: e3.dist_entropy(n)))
            both.append(1e3 * timed(lambda: e3.dist_peaks(n, P=args.worst_peaks, radius=2)))
        picker["n%d" % n] = {"dist_entropy_ms": spread(ent), "dist_peaks_ms": spread(both),
                             "picker_ms_by_difference": float(np.median(both) - np.median(ent))}
    res["picker_313"] = {"grid": "%dx%d" % (H, W), "P": args.worst_peaks, "radius": 2, "calls": picker}
    e3.close()
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
