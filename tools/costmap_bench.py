"""Times of the costmap stage on the GPU.  Reads nothing outside the repository.

    python tools/costmap_bench.py [--runs 50] [--blocks 5]

On 640 x 480 depth frames (synth.depth_image, every 4th valid pixel kept) at batch 1 and 4, cfg-A, tracking on, a
200 x 200 grid of 0.05 m cells with tracks and 4 predicted steps:
  gpu      wall time from the end of a pass (synced) to the grids in host memory: Engine.costmaps().  p50 of --runs,
           repeated --blocks times: the median of the blocks' p50 with their min - max.
  host     the route the stage replaces, on the same commit: the resident points fetched (the difference between
           ingest_depth with and without its parity tap, p50 each), then tracks() + costmap_np per frame.
  kernels  the three kernels from Engine.kernel_times() (a device event pair around each launch), against the time the
           bytes they must touch take at the device's copy rate (Engine.device_copy_GBps): the rows read once, the count
           words cleared, written and read, the grid and the count tap written.
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

GRID = dict(x_min=0.0, y_min=-5.0, resolution=0.05, width=200, height=200, z_min=-0.8, z_max=1.0, objects="tracks",
            horizon_steps=4, horizon_dt=0.25)


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
    rect, trv, _ = pp.synth.default_calib()
    for B in (1, 4):
        eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=pp.ingest.depth_kept_bound(640, 480))
        eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
        eng.set_tracking(pp.tracking.TrackConfig(birth_score=0.0))
        eng.set_costmap(GRID)
        imgs, intr = zip(*[pp.synth.depth_image(i) for i in range(B)])
        imgs, intr = list(imgs), list(intr)
        eng.set_calib(np.stack([rect] * B), np.stack([trv] * B), B)
        for _ in range(3):
            pts = eng.ingest_depth(imgs, intr, return_points=True)
            eng.detect_async()
            eng.sync()
            eng.costmaps()
        tr, nt, _ = eng.tracks()
        n_pts = int(sum(len(p) for p in pts))

        def gpu():
            eng.detect_async()
            eng.sync()
            t0 = time.perf_counter()
            eng.costmaps()
            return 1e6 * (time.perf_counter() - t0)

        def ingest(tap):
            def run():
                t0 = time.perf_counter()
                eng.ingest_depth(imgs, intr, return_points=tap)
                eng.sync()
                return 1e6 * (time.perf_counter() - t0)
            return run

        def host():
            eng.detect_async()
            eng.sync()
            t0 = time.perf_counter()
            t, n, _ = eng.tracks()
            for b in range(B):
                pp.costmap.costmap_np(pts[b], GRID, tracks=t[b], n_tracks=n[b])
            return 1e6 * (time.perf_counter() - t0)

        base = {"batch": B, "points": n_pts, "tracks_mean": round(float(nt.mean()), 2), "runs": a.runs, "blocks": a.blocks}
        print(json.dumps({"what": "gpu: end of pass -> grids on the host", **base, **p50_blocks(gpu, a.runs, a.blocks)}), flush=True)
        with_tap, without = p50_blocks(ingest(True), a.runs, a.blocks), p50_blocks(ingest(False), a.runs, a.blocks)
        rest = p50_blocks(host, max(a.runs // 5, 5), a.blocks)
        print(json.dumps({"what": "host: fetch the points (ingest with - without its tap)", **base,
                          "p50_us": round(with_tap["p50_us"] - without["p50_us"], 1), "with": with_tap, "without": without}), flush=True)
        print(json.dumps({"what": "host: tracks() + costmap_np", **base, **rest}), flush=True)
        # ---- the kernels, profiled in a pass of their own ----
        eng.ingest_depth(imgs, intr)
        eng.detect_async()
        eng.sync()
        eng.set_profiling(True)
        per = {}
        for _ in range(a.runs):
            eng.costmap_async()
            eng.sync()
            for tag, ms in eng.kernel_times():
                per.setdefault(tag, []).append(1e3 * ms)
        eng.set_profiling(False)
        eng.costmaps()
        rate = eng.device_copy_GBps()
        cells = B * 200 * 200
        nbytes = {"k_costmap_objects": B * (64 * 136 + 64 * 5 * 72),
                  "k_costmap_points": n_pts * eng.d.num_point_features * 4 + cells * 4,
                  "k_costmap_compose": cells * (4 + 1 + 4) + B * 64 * 5 * 72}
        for tag, us in per.items():
            floor = nbytes.get(tag, 0) / (rate * 1e3)
            print(json.dumps({"what": tag, "batch": B, "median_us": round(float(np.median(us)), 2), "min_us": round(min(us), 2),
                              "max_us": round(max(us), 2), "bytes": nbytes.get(tag), "copy_rate_GBps": round(rate, 1),
                              "copy_rate_us": round(floor, 3)}), flush=True)
        print(json.dumps({"what": "clear of the count words", "batch": B, "bytes": cells * 4, "copy_rate_us": round(cells * 4 / (rate * 1e3), 3)}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
