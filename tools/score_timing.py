#!/usr/bin/env python3
"""What the distribution score costs, on one box in one process (not a bench.py leg, no pass / fail number).  For each head -- the 529-bin head
at H/4 x W/4 and the 313-bin head at H x W -- the compute span of one pipelined batch (``idc_pipeline_times``: device events on the slot's
compute stream) through ``forward_async_dist`` in these forms, alternating, one batch in flight at a time, the first round untimed:

  head_only     no tap at all: the network and the distribution head (the baseline both others are measured against)
  entropy       + the ``dist_entropy`` launch on the same distribution (``want_entropy``): the launch the score's streaming pass is modelled on
  score_nnK     + the score (truth launch, score launch, finishing launch) with K neighbours, K in ``--nn`` (1, 5, 16), sigma 5, two thresholds

and from the medians: the entropy launch's and the score's addition to the compute span (by difference from head_only) and their ratio.  The
score reads the distribution once, as the entropy launch does, plus nn + 1 gathers per cell; the neighbour search is nn passes over the centres.
Before anything is timed the pipelined score is compared bit for bit with the blocking ``dist_score`` on the blocking route's distribution.

usage: python tools/score_timing.py [--precision bf16] [--batch 32] [--size 256] [--rounds 12] [--nn 1 5 16] [--heads 529 313] [--out f.json]
Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "runs": int(v.size)}


def grid529():
    axis = np.arange(-110, 120, 10)
    return np.ascontiguousarray(np.array(np.meshgrid(axis, axis)).reshape((2, 529)).T.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256, help="net size (a smaller one only to rehearse the script)")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--nn", type=int, nargs="+", default=[1, 5, 16])
    ap.add_argument("--heads", type=int, nargs="+", default=[529, 313])
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    from interactive_deep_colorization_amd import color_bins, engine, workloads
    from oracle import weights
    H = W = args.size
    rs = np.random.RandomState(args.seed)
    base = [rs.randint(0, 256, (203, 187, 3)).astype(np.uint8) for _ in range(args.batch)]
    res = {"precision": args.precision, "net": "%dx%d" % (H, W), "batch": args.batch, "rounds": args.rounds, "heads": {}}
    for bins in args.heads:
        if bins == 529:
            e = engine.HipColorizer(H, W, max_batch=args.batch, precision=args.precision, dist=True)
            e.load_state_dict(workloads.random_state_dict(0, "he"))
            centres = grid529()
        else:
            e = engine.HipColorizer(H, W, max_batch=args.batch, precision=args.precision, dist313=True)
            e.load_state_dict(weights.add_pred313_head(weights.make_state_dict(2, "he", include_class=False), 2))
            e.keep_dist(True)
            centres = np.ascontiguousarray(np.asarray(color_bins.pts_in_hull(), np.float32))
        hd, wd = e._dist_grid()
        # the same bits both ways, on a few images
        few = base[:min(args.batch, 3)]
        for i, img in enumerate(few):
            e.set_image_rgb(img, img=i, keep_source=True, want_rgb=False, want_lab=False)
            e.set_hints([], img=i)
        e.forward_resident(len(few), want_ab=False, want_rgb=False)
        want = e.dist_score(centres, n=len(few), nn=5, want_maps=True)
        got = e.forward_async_dist(0, few, None, peaks=0, score=dict(centres=centres, nn=5, want_maps=True))
        e.wait(0)
        same = all(np.asarray(getattr(got.score, k)).tobytes() == getattr(want, k).tobytes()
                   for k in ("xent", "hits", "xent_map", "rank_map", "target", "truth_ab"))
        legs = {"head_only": lambda s: e.forward_async_dist(s, base, None, peaks=0),
                "entropy": lambda s: e.forward_async_dist(s, base, None, peaks=0, want_entropy=True)}
        for k in args.nn:
            legs["score_nn%d" % k] = (lambda k: lambda s: e.forward_async_dist(s, base, None, peaks=0, score=dict(centres=centres, nn=k)))(k)
        spans = {k: [] for k in legs}
        for r in range(args.rounds + 1):
            for name, fn in legs.items():
                fn(0)
                e.wait(0)
                t = e.pipeline_times(0)
                if r:
                    spans[name].append(float(t[3] - t[2]))
        med = {k: float(np.median(v)) for k, v in spans.items()}
        ent_ms = med["entropy"] - med["head_only"]
        head = {"grid": "%dx%d" % (hd, wd), "bit_identical_to_blocking": bool(same), "distribution_bytes": int(args.batch) * bins * hd * wd * 4,
                "compute_ms": {k: spread(v) for k, v in spans.items()}, "entropy_launch_ms_by_difference": ent_ms, "score": {}}
        for k in args.nn:
            add = med["score_nn%d" % k] - med["head_only"]
            head["score"]["nn%d" % k] = {"added_ms_by_difference": add, "ratio_to_entropy_launch": add / ent_ms if ent_ms > 0 else None}
        res["heads"][str(bins)] = head
        e.close()
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
