"""Times of the rolling occupancy map on the GPU.  Reads nothing outside the repository.

    python tools/occupancy_bench.py [--runs 50] [--blocks 5]

On one 640 x 480 depth frame (synth.depth_image, every 4th valid pixel kept; the scene of tools/costmap_bench.py), a
400 x 400 window of 0.1 m cells, the pose moving 5 cm and turning 0.01 rad per frame:
  gpu      wall time from the end of an ingest (synced) to the map in host memory: Engine.occupancy_update_async +
           occupancy_maps().  p50 of --runs, repeated --blocks times: the median of the blocks' p50 with their min - max.
  host     the route the stage replaces, on the same commit: the resident points fetched (the difference between
           ingest_depth with and without its parity tap, p50 each), then OccupancyMap.update.
  kernels  the three kernels from Engine.kernel_times() (a device event pair around each launch).
  rays     what one frame walks: the cells that took an endpoint (one ray each), the longest ray in cells, the cells all
           rays mark together.
Prints one JSON line per row.
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
    img, intr = pp.synth.depth_image(0)
    imgs, intr = [img], [intr]
    step = [0]

    def pose():
        step[0] += 1
        return pp.sweeps.pose_from_xyyaw(0.05 * step[0], -0.02 * step[0], 0.01 * step[0])[None]

    for _ in range(3):
        pts = eng.ingest_depth(imgs, intr, return_points=True)
        eng.occupancy_update_async(pose())
        eng.occupancy_maps()
    n_pts = len(pts[0])

    def gpu():
        eng.ingest_depth(imgs, intr)
        eng.sync()
        P = pose()
        t0 = time.perf_counter()
        eng.occupancy_update_async(P)
        eng.occupancy_maps()
        return 1e6 * (time.perf_counter() - t0)

    def ingest(tap):
        def run():
            t0 = time.perf_counter()
            eng.ingest_depth(imgs, intr, return_points=tap)
            eng.sync()
            return 1e6 * (time.perf_counter() - t0)
        return run

    ref = pp.occupancy.OccupancyMap(CFG)

    def host():
        P = pose()
        t0 = time.perf_counter()
        ref.update(pts[0], P[0])
        return 1e6 * (time.perf_counter() - t0)

    base = {"points": n_pts, "window": [CFG["width"], CFG["height"]], "runs": a.runs, "blocks": a.blocks}
    print(json.dumps({"what": "gpu: end of ingest -> map on the host", **base, **p50_blocks(gpu, a.runs, a.blocks)}), flush=True)
    with_tap, without = p50_blocks(ingest(True), a.runs, a.blocks), p50_blocks(ingest(False), a.runs, a.blocks)
    print(json.dumps({"what": "host: fetch the points (ingest with - without its tap)", **base,
                      "p50_us": round(with_tap["p50_us"] - without["p50_us"], 1), "with": with_tap, "without": without}), flush=True)
    print(json.dumps({"what": "host: OccupancyMap.update", **base, **p50_blocks(host, max(a.runs // 10, 3), a.blocks)}), flush=True)
    # ---- the kernels, profiled in runs of their own ----
    eng.ingest_depth(imgs, intr)
    eng.sync()
    eng.set_profiling(True)
    per = {}
    for _ in range(a.runs):
        eng.occupancy_update_async(pose())
        eng.sync()
        for tag, ms in eng.kernel_times():
            per.setdefault(tag, []).append(1e3 * ms)
    eng.set_profiling(False)
    for tag, us in per.items():
        print(json.dumps({"what": tag, "median_us": round(float(np.median(us)), 2), "min_us": round(min(us), 2),
                          "max_us": round(max(us), 2)}), flush=True)
    info = {k: int(v[0]) for k, v in eng.occupancy_info().items()}
    # ---- what a frame walks ----
    c = pp.occupancy.OccupancyConfig(**CFG)
    P = pose()[0]
    hit, ground, _ = pp.occupancy.end_cells(c, pts[0], P, pp.occupancy.window_origin(c, P))
    ey, ex = np.nonzero(hit | ground)
    longest = int(np.maximum(np.abs(ex - c.width // 2), np.abs(ey - c.height // 2)).max()) if len(ex) else 0
    marked = int(pp.occupancy._passed_by_rays(ex, ey, c.width // 2, c.height // 2, (c.height, c.width)).sum())
    print(json.dumps({"what": "rays of one frame", "end_cells": int(len(ex)), "longest_ray_cells": longest,
                      "cells_marked_by_rays": marked, "last_update_info": info}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
