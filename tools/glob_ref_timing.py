#!/usr/bin/env python3
"""What a reference photograph costs on its way to the net's global input, on one box in one process (not a bench.py leg, no pass / fail
number).  A 256 x 256 bf16 Global-Hints handle, 512 x 512 noise references.

  install   median of ``--runs`` calls, host clock around calls that end synchronised:
              host    the route before idc_set_global_refs: ``colorspace.resize_bilinear_u8`` to the net size on the host,
                      ``global_histogram`` (counts to the host, normalised there), ``set_global_hints``
              device  ``set_global_refs`` with the photograph as it comes                    (where the engine has it)
  spans     median compute span of ``idc_pipeline_times`` for an N = ``--batch`` batch of 256 x 256 sources on the two slots with pinned
            buffers, after two warm-up batches per slot: with N distinct references, with one shared by all, with an empty reference
            list, and the plain call (``refs=None``)                                         (where the engine has them)

``--repo DIR`` measures the package of another checkout (say the parent commit's, for the host route there) with this script.
usage: python tools/glob_ref_timing.py [--repo DIR] [--runs 20] [--batch 32] [--batches 12] [--size 256] [--out f.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--size", type=int, default=256, help="net size (a smaller one only to rehearse the script)")
    ap.add_argument("--ref-size", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    from interactive_deep_colorization_amd import color_bins, colorspace, engine  # noqa: E402
    from oracle import weights  # noqa: E402

    S, R, n = args.size, args.ref_size, args.batch
    c = np.ascontiguousarray(color_bins.pts_in_hull(), dtype=np.float32)
    rs = np.random.RandomState(1)
    refs = [rs.randint(0, 256, (R, R, 3)).astype(np.uint8) for _ in range(n)]
    sd = weights.add_global_branch(weights.make_state_dict(0, "he", include_class=False), 0)
    e = engine.HipColorizer(S, S, max_batch=n, precision="bf16", global_hints=True)
    e.load_state_dict(sd)
    res = {"repo": os.path.abspath(args.repo), "net": "%dx%d" % (S, S), "reference": "%dx%d" % (R, R), "batch": n}

    def host_route(ref):
        net = colorspace.resize_bilinear_u8(ref, S, S)
        hist, _ = e.global_histogram(net, c)
        g = np.zeros((1, 314), np.float32)
        g[0, :313], g[0, 313] = hist[0], 1.0
        e.set_global_hints(g)

    routes = [("host", host_route)]
    if hasattr(e, "set_global_refs"):
        routes.append(("device", lambda ref: e.set_global_refs([ref], c)))
    times = {name: [] for name, _ in routes}
    for r in range(3 + args.runs):                                   # three warm-up rounds; the routes alternate
        for name, fn in routes:
            t0 = time.perf_counter()
            fn(refs[r % n])
            dt = time.perf_counter() - t0
            if r >= 3:
                times[name].append(dt * 1e3)
    res["install_ms"] = {name: spread(v) for name, v in times.items()}

    if hasattr(e, "set_global_refs"):
        batch = rs.randint(0, 256, (n, S, S, 3)).astype(np.uint8)
        bufs = [(e.pinned_empty(batch.shape, np.uint8), e.pinned_empty((n, S, S, 3), np.uint8)) for _ in range(2)]
        for src, _ in bufs:
            src[...] = batch
        cases = [("distinct", dict(refs=refs, ref_index=None, centres=c)), ("shared", dict(refs=refs[:1], ref_index=[0] * n, centres=c)),
                 ("none", dict(refs=[])), ("plain_call", dict())]
        spans = {name: {"compute": [], "h2d": []} for name, _ in cases}
        for rnd in range(2):                                         # the cases alternate, twice
            for name, kw in cases:
                count = args.batches
                for k in range(count + 2):
                    slot = k & 1
                    if k >= 2:
                        e.wait(slot)
                        t = e.pipeline_times(slot)
                        if k >= 6:                                   # two batches per slot warm up
                            spans[name]["compute"].append(float(t[3] - t[2]))
                            spans[name]["h2d"].append(float(t[1] - t[0]))
                    if k < count:
                        e.forward_async_rgb(slot, bufs[slot][0], None, bufs[slot][1], **kw)
        res["compute_span_ms"] = {name: spread(v["compute"]) for name, v in spans.items()}
        res["h2d_span_ms"] = {name: spread(v["h2d"]) for name, v in spans.items()}
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
