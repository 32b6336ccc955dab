"""Times of the navigation function on the GPU.  Reads nothing outside the repository.

    python tools/navfn_bench.py [--runs 50] [--blocks 5] [--host-runs 3]

Behind the costmap's point layer and its inflation (the defaults of InflationConfig, R = 10 cells) on a 400 x 400 window of
0.1 m cells at batch 1 (unknown cells allowed: the point layer leaves empty cells unknown), the goal at the window's far
edge, the start the sensor's own cell, two scenes: `open` (a synth.d435i_cloud frame) and `wall` (the same frame and a
wall of points across the window 10 m ahead, open at one end only, which forces a detour).  Measured from the end of the
inflation (synced):
  path     wall time to the path in host memory: Engine.navfn_async + navfn_paths.  p50 of --runs, repeated --blocks
           times: the median of the blocks' p50 with their min - max.
  field    the same to the field uint32 [400, 400] in host memory (navfn_fields).
  host     the route the stage replaces, on the same commit: the inflated grid fetched, then navfn.navfn_np +
           navfn.descend_np on it -- the restatement, a Python heap Dijkstra, not a tuned CPU planner.
  relax    k_navfn_relax from Engine.kernel_times() (a device event pair around each launch): the median over the rounds
           that ran, and the rounds.
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

COSTMAP = dict(x_min=0.0, y_min=-20.0, resolution=0.1, width=400, height=400, z_min=-0.8, z_max=1.0)
GOAL = np.array([[39.95, 0.05]])


def p50_blocks(fn, runs, blocks):
    p = []
    for _ in range(blocks):
        p.append(float(np.median([fn() for _ in range(runs)])))
    return {"p50_us": round(float(np.median(p)), 1), "p50_min_us": round(min(p), 1), "p50_max_us": round(max(p), 1)}


def scene(name):
    pts = np.asarray(pp.synth.d435i_cloud(900, 4096), np.float32)
    if name == "wall":
        y = np.arange(-19.95, 16.0, 0.05, dtype=np.float32)
        wall = np.zeros((len(y), pts.shape[1]), np.float32)
        wall[:, 0], wall[:, 1], wall[:, 2] = 10.05, y, 0.2
        pts = np.concatenate([pts, wall])
    return pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    a = ap.parse_args()
    N = pp.navfn
    eng = pp.Engine(pp.config.pedestrian_d435i_config(1), max_batch=1, max_points_per_frame=16384)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    eng.set_costmap(COSTMAP)
    eng.set_inflation(True, "costmap")
    eng.set_navfn(dict(allow_unknown=1), "costmap")      # the point layer leaves the cells no return fell into unknown
    cfg = eng.navfn_config("costmap")
    for name in ("open", "wall"):
        eng.upload([scene(name)])

        def inflated():
            """The inflation on the resident frame, finished."""
            eng.costmap_async()
            eng.inflate_async("costmap")
            eng._costmap_queued = False
            eng.sync()

        inflated()
        grid = eng._inflated(0, None, False)[0][0]
        eng.navfn_async(GOAL)
        pot = eng.navfn_fields()[0]
        paths, states = eng.navfn_paths()
        info = {k: v.tolist() for k, v in eng.navfn_info().items()}
        goal = N.goal_cells(GOAL, (COSTMAP["x_min"], COSTMAP["y_min"]), COSTMAP["resolution"], grid.shape)[0]
        start = N.goal_cells((0.0, 0.0), (COSTMAP["x_min"], COSTMAP["y_min"]), COSTMAP["resolution"], grid.shape)[0]
        want = N.navfn_np(grid, goal, cfg)
        assert np.array_equal(pot, want), "the stage does not equal navfn_np"
        wpath, wstate = N.descend_np(want, grid, start, cfg)
        assert np.array_equal(paths[0], wpath) and states[0] == wstate, "the path does not equal descend_np"

        def to_path():
            inflated()
            t0 = time.perf_counter()
            eng.navfn_async(GOAL)
            eng.navfn_paths()
            return 1e6 * (time.perf_counter() - t0)

        def to_field():
            inflated()
            t0 = time.perf_counter()
            eng.navfn_async(GOAL)
            eng.navfn_fields()
            return 1e6 * (time.perf_counter() - t0)

        def host():
            inflated()
            t0 = time.perf_counter()
            g = eng._inflated(0, None, False)[0][0]
            N.descend_np(N.navfn_np(g, goal, cfg), g, start, cfg)
            return 1e6 * (time.perf_counter() - t0)

        base = {"scene": name, "batch": 1, "window": [400, 400], "path_cells": len(paths[0]), "path_state": int(states[0]),
                "info": info, "runs": a.runs, "blocks": a.blocks}
        print(json.dumps({"what": "gpu: end of the inflation -> path on the host", **base, **p50_blocks(to_path, a.runs, a.blocks)}), flush=True)
        print(json.dumps({"what": "gpu: end of the inflation -> field on the host", **base, **p50_blocks(to_field, a.runs, a.blocks)}), flush=True)
        print(json.dumps({"what": "host: fetch the inflated grid + navfn_np + descend_np (the restatement)", **base,
                          **p50_blocks(host, a.host_runs, 1)}), flush=True)
        # ---- the kernels, profiled in runs of their own ----
        inflated()
        eng.set_profiling(True)
        relax, init, finish = [], [], []
        for _ in range(max(a.runs // 5, 3)):
            eng.navfn_async(GOAL)
            eng.sync()
            for k, ms in eng.kernel_times():
                {"k_navfn_relax": relax, "k_navfn_init": init, "k_navfn_finish": finish}[k].append(1e3 * ms)
        eng.set_profiling(False)
        print(json.dumps({"what": "kernels", **base, "relax_median_us": round(float(np.median(relax)), 2), "relax_max_us": round(max(relax), 2),
                          "relax_launches_per_call": len(relax) // max(a.runs // 5, 3), "init_median_us": round(float(np.median(init)), 2),
                          "finish_median_us": round(float(np.median(finish)), 2)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
