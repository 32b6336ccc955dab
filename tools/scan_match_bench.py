"""Times of the scan match on the GPU.  Reads nothing outside the repository.

    python tools/scan_match_bench.py [--runs 50] [--blocks 5]

On one 640 x 480 depth frame (synth.depth_image, every 4th valid pixel kept; the scene of tools/occupancy_bench.py), a
400 x 400 window of 0.1 m cells that five updates have filled, the default window of 21 headings x 441 translations:
  gpu      wall time from the end of an ingest (synced) to the eight words in host memory: Engine.scan_match_async +
           scan_match_results().  p50 of --runs, repeated --blocks times: the median of the blocks' p50 with their min - max.
  host     the route the stage replaces, on the same commit: the resident points fetched (the difference between
           ingest_depth with and without its parity tap, p50 each), then scan_match.match_np.
  kernels  the three kernels from Engine.kernel_times() (a device event pair around each launch).
  work     what one match looks up: scan cells, candidates, gathers.
Prints one JSON line per row.  The stage off is measured by tools/occupancy_bench.py, on this commit beside its parent.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pp_amd as pp  # noqa: E402

CFG = dict(resolution=0.1, width=400, height=400, z_min=-0.8, z_max=1.0, max_range=20.0)


def p50_blocks(fn, runs, blocks):
    p = []
    for _ in range(blocks):
        t = []
        for _ in range(runs):
            t.append(fn())
        p.append(float(np.median(t)))
    return {"p50_us": round(float(np.median(p)), 1), "p50_min_us": round(min(p), 1), "p50_max_us": round(max(p), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    eng = pp.Engine(pp.config.pedestrian_d435i_config(1), max_batch=1, max_points_per_frame=pp.ingest.depth_kept_bound(640, 480))
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    eng.set_occupancy(CFG)
    scan = pp.scan_match.ScanMatchConfig()
    eng.set_scan_match(scan)
    img, intr = pp.synth.depth_image(0)
    imgs, intr = [img], [intr]
    ref = pp.occupancy.OccupancyMap(CFG)

    def pose(k):
        return pp.sweeps.pose_from_xyyaw(0.05 * k, -0.02 * k, 0.01 * k)

    for k in range(5):
        pts = eng.ingest_depth(imgs, intr, return_points=True)
        eng.occupancy_update_async(pose(k)[None])
        eng.occupancy_maps()
        ref.update(pts[0], pose(k))
    n_pts = len(pts[0])
    prior = pp.sweeps.pose_from_xyyaw(0.05 * 5 + 0.2, -0.02 * 5 - 0.1, 0.01 * 5 + 0.03)[None]
    # the stage computes what the restatement computes, at the shape that is timed
    eng.scan_match_async(prior)
    words, scores = eng.scan_match_results(scores=True)
    w_ref, s_ref = pp.scan_match.match_np(ref, pts[0], prior[0], scan)
    if words[0].tolist() != w_ref.tolist() or not np.array_equal(scores[0], s_ref):
        raise SystemExit(f"scan_match_bench: the stage gives {words[0].tolist()}, the restatement {w_ref.tolist()}")

    def gpu():
        eng.ingest_depth(imgs, intr)
        eng.sync()
        t0 = time.perf_counter()
        eng.scan_match_async(prior)
        eng.scan_match_results()
        return 1e6 * (time.perf_counter() - t0)

    def ingest(tap):
        def run():
            t0 = time.perf_counter()
            eng.ingest_depth(imgs, intr, return_points=tap)
            eng.sync()
            return 1e6 * (time.perf_counter() - t0)
        return run

    def host():
        t0 = time.perf_counter()
        pp.scan_match.match_np(ref, pts[0], prior[0], scan)
        return 1e6 * (time.perf_counter() - t0)

    base = {"points": n_pts, "window": [CFG["width"], CFG["height"]], "candidates": scan.candidates, "scan_cells": int(words[0, 6]),
            "runs": a.runs, "blocks": a.blocks}
    print(json.dumps({"what": "gpu: end of ingest -> words on the host", **base, **p50_blocks(gpu, a.runs, a.blocks)}), flush=True)
    with_tap, without = p50_blocks(ingest(True), a.runs, a.blocks), p50_blocks(ingest(False), a.runs, a.blocks)
    print(json.dumps({"what": "host: fetch the points (ingest with - without its tap)", **base,
                      "p50_us": round(with_tap["p50_us"] - without["p50_us"], 1), "with": with_tap, "without": without}), flush=True)
    print(json.dumps({"what": "host: scan_match.match_np", **base, **p50_blocks(host, max(a.runs // 10, 3), a.blocks)}), flush=True)
    # ---- the kernels, profiled in runs of their own ----
    eng.ingest_depth(imgs, intr)
    eng.sync()
    eng.set_profiling(True)
    per = {}
    for _ in range(a.runs):
        eng.scan_match_async(prior)
        eng.sync()
        for tag, ms in eng.kernel_times():
            per.setdefault(tag, []).append(1e3 * ms)
    eng.set_profiling(False)
    for tag, us in per.items():
        print(json.dumps({"what": tag, "median_us": round(float(np.median(us)), 2), "min_us": round(min(us), 2),
                          "max_us": round(max(us), 2)}), flush=True)
    print(json.dumps({"what": "work of one match", "scan_cells": int(words[0, 6]), "rows_ignored": int(words[0, 7]),
                      "candidates": scan.candidates, "gathers": int(words[0, 6]) * scan.candidates, "words": words[0].tolist()}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
