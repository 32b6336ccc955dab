"""Times of the obstacle inflation on the GPU.  Reads nothing outside the repository.

    python tools/inflation_bench.py [--runs 50] [--blocks 5]

On 640 x 480 depth frames (synth.depth_image, every 4th valid pixel kept; the scene of tools/occupancy_bench.py) at batch
1 and 4, a 400 x 400 window of 0.1 m cells behind either source -- the costmap's point layer, the rolling occupancy maps
(the pose moving 5 cm and turning 0.01 rad per frame) -- and the defaults of InflationConfig, R = 10 cells:
  gpu      wall time from the end of costmap_async / occupancy_update_async (synced) to the inflated grids in host memory:
           Engine.inflate_async + the fetch.  p50 of --runs, repeated --blocks times: the median of the blocks' p50 with
           their min - max.
  host     the route the stage replaces, on the same commit: the plain grids fetched (costmaps() / occupancy_maps() of the
           run that is already on the device), then inflation.inflate_np on each.
  kernel   k_inflate from Engine.kernel_times() (a device event pair around the launch).
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
OCC = dict(resolution=0.1, width=400, height=400, z_min=-0.8, z_max=1.0, max_range=20.0)
INFL = dict(lethal_threshold=65)          # one hit of the occupancy defaults reads 70; the costmap's points read 100


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
    for B in (1, 4):
        eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=pp.ingest.depth_kept_bound(640, 480))
        eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
        eng.set_costmap(COSTMAP)
        eng.set_occupancy(OCC)
        for source in pp.inflation.SOURCES:
            eng.set_inflation(INFL, source)
        cfg = eng.inflation_config("costmap")
        imgs, intr = zip(*[pp.synth.depth_image(i) for i in range(B)])
        imgs, intr = list(imgs), list(intr)
        step = [0]

        def poses():
            step[0] += 1
            return np.stack([pp.sweeps.pose_from_xyyaw(0.05 * step[0] + b, -0.02 * step[0], 0.01 * step[0]) for b in range(B)])

        def source_run(source):
            """The source stage on fresh frames, finished."""
            eng.ingest_depth(imgs, intr)
            if source == "costmap":
                eng.costmap_async()
            else:
                eng.occupancy_update_async(poses())
            eng.sync()

        def fetch(source, inflated):
            if source == "costmap":
                return eng.inflated_costmaps() if inflated else eng.costmaps()
            return (eng.inflated_occupancy_maps() if inflated else eng.occupancy_maps())[0]

        for source in pp.inflation.SOURCES:
            for _ in range(3):
                source_run(source)
                got = fetch(source, True)
            plain = fetch(source, False)                 # of the same run (the costmap stage runs again on the same frames)
            assert all(np.array_equal(got[b], pp.inflation.inflate_np(plain[b], cfg)) for b in range(B)), "the stage does not equal inflate_np"

            def gpu():
                source_run(source)
                t0 = time.perf_counter()
                fetch(source, True)
                return 1e6 * (time.perf_counter() - t0)

            def host():
                source_run(source)
                t0 = time.perf_counter()
                grids = fetch(source, False)
                for g in grids:
                    pp.inflation.inflate_np(g, cfg)
                return 1e6 * (time.perf_counter() - t0)

            def host_fetch():
                source_run(source)
                t0 = time.perf_counter()
                fetch(source, False)
                return 1e6 * (time.perf_counter() - t0)

            base = {"source": source, "batch": B, "window": [400, 400], "R": pp.inflation.radius_cells(cfg), "runs": a.runs, "blocks": a.blocks}
            print(json.dumps({"what": "gpu: end of the source stage -> inflated grids on the host", **base,
                              **p50_blocks(gpu, a.runs, a.blocks)}), flush=True)
            print(json.dumps({"what": "host: fetch the plain grids", **base, **p50_blocks(host_fetch, a.runs, a.blocks)}), flush=True)
            print(json.dumps({"what": "host: fetch the plain grids + inflate_np", **base,
                              **p50_blocks(host, max(a.runs // 10, 3), a.blocks)}), flush=True)
            # ---- the kernel, profiled in runs of its own ----
            source_run(source)
            eng.set_profiling(True)
            us = []
            for _ in range(a.runs):
                eng.inflate_async(source)
                eng.sync()
                times = eng.kernel_times()
                assert [k for k, _ in times] == ["k_inflate"], times
                us.append(1e3 * times[0][1])
            eng.set_profiling(False)
            info = {k: v.tolist() for k, v in eng.inflation_info(source).items()}
            cells = B * 400 * 400
            print(json.dumps({"what": "k_inflate", **base, "median_us": round(float(np.median(us)), 2), "min_us": round(min(us), 2),
                              "max_us": round(max(us), 2), "bytes_read_written": cells * (1 + 1 + 2), "info": info}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
