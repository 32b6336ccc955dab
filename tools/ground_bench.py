"""Times of the ground stage on the GPU.  Reads nothing outside the repository.

    python tools/ground_bench.py [--runs 50] [--blocks 5]

On tools/costmap_bench.py's scene -- a 640 x 480 depth frame (synth.depth_image, every 4th valid pixel kept) at batch 1,
cfg-A -- for K = 128 and K = 512 hypotheses, refine 0 and 1:
  check    the stage is first held to the restatement at that shape: plane bits, info words, both bit planes, sums, counts
  kernels  the stage's launches from Engine.kernel_times() (a device event pair around each launch); for k_ground_score
           the float64 operations it issues (5 per test of a candidate row against a valid hypothesis: 2 multiplies, 3
           adds) per second
  wall     from the end of an ingest (synced) to the plane and the info words in host memory: ground_async() + ground();
           beside it, fetching the points and running ground_np on the host
  floor    k_ground_score once more on an open floor of as many rows, where nearly every hypothesis is valid
  readers  k_occ_endpoints, k_scan_cells and k_costmap_points with the classes named in `consumers` and without
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

GRID = dict(x_min=0.0, y_min=-5.0, resolution=0.05, width=200, height=200, z_min=-0.8, z_max=1.0, objects=0)
OCC = dict(resolution=0.05, z_min=-0.8, z_max=1.0, max_range=12.0, width=400, height=400)
SCAN = dict(nx=4, ny=4, nt=4, xy_step=1024, theta_step=8, min_cells=50, min_mean=0)
GROUND = dict(seed=1, max_range=12.0, cand_z_max=0.5, max_slope=0.3, h_min=-0.5, h_max=3.0, inlier_dist=0.05, min_inliers=500,
              ground_dist=0.1, overhead_max=2.0, fallback_c=-1.4)
READERS = {"occupancy": "k_occ_endpoints", "scan_match": "k_scan_cells", "costmap": "k_costmap_points"}


def stats(us):
    return {"median_us": round(float(np.median(us)), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}


def p50_blocks(fn, runs, blocks):
    p = [float(np.median([fn() for _ in range(runs)])) for _ in range(blocks)]
    return {"p50_us": round(float(np.median(p)), 1), "p50_min_us": round(min(p), 1), "p50_max_us": round(max(p), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    g = pp.ground
    B = 1
    eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=pp.ingest.depth_kept_bound(640, 480))
    eng.set_costmap(GRID)
    eng.set_occupancy(OCC)
    eng.set_scan_match(SCAN)
    imgs, intr = zip(*[pp.synth.depth_image(i) for i in range(B)])
    imgs, intr = list(imgs), list(intr)
    pose = np.stack([pp.sweeps.pose_from_xyyaw(0.0, 0.0, 0.0)] * B)
    pts = eng.ingest_depth(imgs, intr, return_points=True)
    n_pts = int(sum(len(p) for p in pts))
    base = {"batch": B, "points": n_pts, "runs": a.runs, "blocks": a.blocks}

    for K in (128, 512):
        for refine in (0, 1):
            cfg = dict(GROUND, hypotheses=K, refine=refine, consumers=())
            eng.set_ground(cfg)
            t = g.draw_triples(cfg["seed"], 0, B, K)
            # ---- the stage against the restatement at this shape ----
            eng.ground_async(t)
            planes, info, gnd, obs, sums, counts = eng.ground(bits=True, debug=True)
            t0 = time.perf_counter()
            want = [g.ground_np(pts[b], cfg, t[b]) for b in range(B)]
            host_s = time.perf_counter() - t0
            for b in range(B):
                w = want[b]
                assert planes[b].tobytes() == w["plane"].tobytes() and [int(info[k][b]) for k in g.INFO] == w["info"].tolist(), b
                assert np.array_equal(gnd[b], w["ground"]) and np.array_equal(obs[b], w["obstacle"]), b
                assert sums[b].tolist() == w["sums"].tolist() and counts[b].tolist() == w["counts"].tolist(), b
            row = {"K": K, "refine": refine, **base}
            print(json.dumps({"what": "check: the stage equals the restatement", **row, "plane": planes[0].tolist(),
                              "info": {k: int(info[k][0]) for k in g.INFO}, "ground_np_s": round(host_s, 3)}), flush=True)

            # ---- the launches ----
            eng.set_profiling(True)
            per = {}
            for _ in range(a.runs):
                eng.ground_async(t)
                eng.sync()
                for tag, ms in eng.kernel_times():
                    per.setdefault(tag, []).append(1e3 * ms)
            eng.set_profiling(False)
            tests = int(info["candidates"][0]) * int(info["valid"][0])
            for tag, us in per.items():
                extra = {}
                if tag == "k_ground_score":
                    extra = {"tests": tests, "fp64_ops": 5 * tests, "fp64_Gops_per_s": round(5 * tests / (float(np.median(us)) * 1e3), 1)}
                print(json.dumps({"what": tag, **row, **stats(us), **extra}), flush=True)
            print(json.dumps({"what": "launches", **row, "launches": len(per)}), flush=True)

            # ---- end of ingest -> plane and info words on the host ----
            def wall():
                eng.ingest_depth(imgs, intr)
                eng.sync()
                t0 = time.perf_counter()
                eng.ground_async(t)
                eng.ground()
                return 1e6 * (time.perf_counter() - t0)

            print(json.dumps({"what": "wall: end of ingest -> plane and info words on the host", **row, **p50_blocks(wall, a.runs, a.blocks)}),
                  flush=True)

    # ---- an open floor: the same number of rows, nearly every row a candidate and nearly every hypothesis valid ----
    rng = np.random.default_rng(3)
    x, y = rng.uniform(0.5, 10.0, n_pts), rng.uniform(-4.0, 4.0, n_pts)
    z = 0.02 * x - 0.01 * y - 1.2 + rng.uniform(-0.01, 0.01, n_pts)
    z[::10] += rng.uniform(0.2, 1.0, len(z[::10]))                      # a tenth of the rows on things that stand on it
    floor = [np.ascontiguousarray(np.stack([x, y, z], 1).astype(np.float32))]
    eng.upload(floor)
    for K in (128, 512):
        cfg = dict(GROUND, hypotheses=K, refine=1, consumers=())
        eng.set_ground(cfg)
        t = g.draw_triples(cfg["seed"], 0, B, K)
        eng.ground_async(t)
        planes, info, gnd, obs, sums, counts = eng.ground(bits=True, debug=True)
        w = g.ground_np(floor[0], cfg, t[0])
        assert planes[0].tobytes() == w["plane"].tobytes() and [int(info[k][0]) for k in g.INFO] == w["info"].tolist()
        assert np.array_equal(gnd[0], w["ground"]) and np.array_equal(obs[0], w["obstacle"]) and counts[0].tolist() == w["counts"].tolist()
        eng.set_profiling(True)
        us = []
        for _ in range(a.runs):
            eng.ground_async(t)
            eng.sync()
            us += [1e3 * ms for tag, ms in eng.kernel_times() if tag == "k_ground_score"]
        eng.set_profiling(False)
        tests = int(info["candidates"][0]) * int(info["valid"][0])
        print(json.dumps({"what": "k_ground_score, open floor", "K": K, "points": n_pts, "candidates": int(info["candidates"][0]),
                          "valid": int(info["valid"][0]), **stats(us), "tests": tests, "fp64_ops": 5 * tests,
                          "fp64_Gops_per_s": round(5 * tests / (float(np.median(us)) * 1e3), 1)}), flush=True)

    # ---- the three readers' kernels with the classes and without ----
    calls = {"occupancy": lambda: eng.occupancy_update_async(pose), "scan_match": lambda: eng.scan_match_async(pose),
             "costmap": lambda: eng.costmap_async()}
    eng.ingest_depth(imgs, intr)
    eng.set_ground(None)
    eng.occupancy_update_async(pose)          # a map for the scan match
    for named in (False, True, False, True):
        eng.set_ground(dict(GROUND, hypotheses=128, consumers=tuple(READERS) if named else ()))
        eng.ground_async()
        eng.set_profiling(True)
        per = {}
        for _ in range(a.runs):
            for name, call in calls.items():
                call()
                eng.sync()
                for tag, ms in eng.kernel_times():
                    if tag == READERS[name]:
                        per.setdefault(tag, []).append(1e3 * ms)
        eng.set_profiling(False)
        for tag, us in per.items():
            print(json.dumps({"what": tag, "classes": named, "batch": B, **stats(us)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
