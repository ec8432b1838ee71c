#!/usr/bin/env python3
"""What a batch of images of individual sizes (``idc_forward_async_images``) costs and buys, on one box in one process (not a bench.py leg,
no pass / fail number).  Pinned buffers, source-size output, no hints, the two pipeline slots in turn.

  uniform   ``--batch`` sources of 1024 x 768 through ``forward_async_rgb`` and through ``forward_async_images``: the compute span of
            ``idc_pipeline_times`` (compute end - compute start) per batch.  The same arithmetic runs; the new call adds the table lookup.
            The two routes alternate ``--rounds`` times, so that each figure comes with its own run-to-run spread.
  mixed     ``--batch`` sources whose sides are drawn once (``--seed``) from 256..1536: images per second through ONE
            ``forward_async_images`` call per batch, against what a caller had to do before -- the same images grouped by size through
            ``forward_async_rgb``, which for distinct sizes is one call of n = 1 per image.  Wall time of ``--batches`` batches per slot with
            both slots busy, ending in the wait for the last one.

Every route runs ``--warmup`` untimed batches per slot first, then ``--batches`` (at least 5) timed ones per slot; medians with minimum and
maximum.  ``--repo`` imports the package (and its library) from another checkout, e.g. one of the parent commit: a package without
``forward_async_images`` runs the ``forward_async_rgb`` routes only, which gives the parent's own figure and spread for the uniform case.

usage: python tools/ragged_timing.py [--precision bf16] [--batch 32] [--size 256] [--batches 6] [--warmup 2] [--rounds 2] [--repo DIR] [--out f.json]
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


def pinned_copy(e, a):
    p = e.pinned_empty(a.shape, a.dtype)
    p[...] = a
    return p


def run_slots(e, submit, count, warm):
    """``count + warm`` batches per slot through submit(slot); -> (compute spans of the timed batches, their wall time in seconds)."""
    spans, total = [], 2 * (count + warm)
    t0 = None
    for k in range(total + 2):
        slot = k & 1
        if k >= 2:
            e.wait(slot)
            if k - 2 >= 2 * warm:
                t = e.pipeline_times(slot)
                spans.append(float(t[3] - t[2]))
        if k == 2 * warm:
            t0 = time.perf_counter()             # (the two warm batches still in flight are waited for inside the timed part: a small over-count)
        if k < total:
            submit(slot)
    return spans, time.perf_counter() - t0


def uniform(e, args, new_call):
    n, sh, sw = args.batch, 768, 1024
    rs = np.random.RandomState(1)
    src = [pinned_copy(e, rs.randint(0, 256, (n, sh, sw, 3)).astype(np.uint8)) for _ in range(2)]
    dst = [e.pinned_empty((n, sh, sw, 3), np.uint8) for _ in range(2)]
    per_image = [([src[s][i] for i in range(n)], [dst[s][i] for i in range(n)]) for s in range(2)]
    res = {"sources": "%d x %dx%d" % (n, sw, sh), "forward_async_rgb_compute_ms": [], "forward_async_images_compute_ms": []}
    for _ in range(args.rounds):
        spans, _ = run_slots(e, lambda s: e.forward_async_rgb(s, src[s], None, dst[s], out="source"), args.batches, args.warmup)
        res["forward_async_rgb_compute_ms"].append(spread(spans))
        if new_call:
            spans, _ = run_slots(e, lambda s: e.forward_async_images(s, per_image[s][0], None, per_image[s][1], out="source"), args.batches,
                                 args.warmup)
            res["forward_async_images_compute_ms"].append(spread(spans))
    return res


def mixed(e, args, new_call):
    n = args.batch
    rs = np.random.RandomState(args.seed)
    sizes = [(int(rs.randint(256, 1537)), int(rs.randint(256, 1537))) for _ in range(n)]
    src = [[pinned_copy(e, rs.randint(0, 256, (h, w, 3)).astype(np.uint8)) for h, w in sizes] for _ in range(2)]
    dst = [[e.pinned_empty((h, w, 3), np.uint8) for h, w in sizes] for _ in range(2)]
    res = {"sources": n, "seed": args.seed, "sides": "256..1536", "megapixels": sum(h * w for h, w in sizes) / 1e6}
    if new_call:
        spans, wall = run_slots(e, lambda s: e.forward_async_images(s, src[s], None, dst[s], out="source"), args.batches, args.warmup)
        res["forward_async_images"] = {"img_per_s": 2 * args.batches * n / wall, "compute_ms": spread(spans)}
    # before: one forward_async_rgb call of n = 1 per image (no two sizes are equal), the slots in turn
    state = {"i": 0}

    def one(slot):
        i = state["i"] % n
        state["i"] += 1
        e.forward_async_rgb(slot, src[slot][i][None], None, dst[slot][i][None], out="source")
    assert len(set(sizes)) == n
    spans, wall = run_slots(e, one, args.batches * n // 2, args.warmup * n // 2)
    res["forward_async_rgb_n1"] = {"img_per_s": 2 * (args.batches * n // 2) / wall, "compute_ms_per_image": spread(spans)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256, help="net size (a smaller one only to rehearse the script)")
    ap.add_argument("--batches", type=int, default=6, help="timed batches per slot")
    ap.add_argument("--warmup", type=int, default=2, help="untimed batches per slot")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.batches < 5:
        ap.error("--batches: at least 5 timed batches per slot")
    sys.path.insert(0, os.path.abspath(args.repo))
    from interactive_deep_colorization_amd import engine, workloads
    e = engine.HipColorizer(args.size, args.size, max_batch=args.batch, precision=args.precision)
    e.load_state_dict(workloads.random_state_dict(0, "he"))
    new_call = hasattr(e, "forward_async_images")
    res = {"repo": os.path.abspath(args.repo), "forward_async_images": new_call, "precision": args.precision, "net": "%dx%d" % (args.size, args.size),
           "batches_per_slot": args.batches, "warmup_per_slot": args.warmup, "uniform": uniform(e, args, new_call), "mixed": mixed(e, args, new_call)}
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
