"""Times of the local planner's footprint on the GPU.  Reads nothing outside the repository.

    python tools/local_footprint_bench.py [--runs 50] [--blocks 5] [--host-runs 3] [--only-off]

The scenes, the window and the samples of tools/local_plan_bench.py: a 400 x 400 window of 0.1 m cells at batch 1, 33 x 41
samples, 64 steps.  The robot is a rectangle of 0.9 m x 0.5 m: 56 probes at the default spacing of half a cell, 256 at the
finest spacing that fits the table.  It stands at the pose along the x axis, among ten from 1 m to 20 m at which the
footprint is free, where the most samples survive under the footprint: the rollout's longest case (the sensor itself sits
on the window's edge, where the rear of the robot would lie outside).  With 0 and 8 movers
as tools/local_movers_bench.py makes them.  Measured from the settled field (navfn_fields has returned):
  off      no footprint, no movers: Engine.local_plan_async + local_commands with the default pose, the figure of
           tools/local_plan_bench.py and of tools/local_movers_bench.py's first row (--only-off stops behind it).
  command  the footprint on: the same two calls, which now queue the rollout and the finish with a footprint.
           p50 of --runs, repeated --blocks times: the median of the blocks' p50 with their min - max.
  host     the route the stage replaces, on the same commit: the inflated grid and the field fetched (and, with movers,
           tracks() and movers_np), then local_planner.best_np with the footprint -- the restatement in numpy, not a tuned
           CPU planner.
  kernels  the rollout and the finish from Engine.kernel_times().
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
from local_movers_bench import MOVERS, STEP_DT, walk  # noqa: E402
from local_plan_bench import LOCAL, WINDOW  # noqa: E402
from navfn_bench import COSTMAP, GOAL, p50_blocks, scene  # noqa: E402

ROBOT = (0.9, 0.5)      # metres: length, width


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--only-off", action="store_true")
    a = ap.parse_args()
    LP = pp.local_planner
    eng = pp.Engine(pp.config.pedestrian_d435i_config(1), max_batch=1, max_points_per_frame=16384)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    eng.set_costmap(COSTMAP)
    eng.set_inflation(True, "costmap")
    eng.set_navfn(dict(allow_unknown=1), "costmap")      # the point layer leaves the cells no return fell into unknown
    eng.set_local_planner(LOCAL, "costmap")
    eng.set_tracking(True)
    ncfg, cfg = eng.navfn_config("costmap"), eng.local_planner_config("costmap")
    org, res = (COSTMAP["x_min"], COSTMAP["y_min"]), COSTMAP["resolution"]
    feet = {"56 probes": LP.Footprint.rectangle(*ROBOT, resolution=res), "256 probes": LP.Footprint.rectangle(*ROBOT, resolution=res, spacing=0.11)}
    assert [len(f) for f in feet.values()] == [56, 256]
    for name in ("open", "wall"):
        eng.upload([scene(name)])
        eng.set_local_footprint(None)
        eng.set_local_movers(None, "costmap")
        eng._plan_async(GOAL, "costmap", None)
        pot = eng.navfn_fields()[0]                      # the settled field: the span starts here
        grid = eng._inflated(0, None, False)[0][0]
        gs = int(eng.navfn_info()["goal_state"][0])
        base = {"scene": name, "batch": 1, "window": [400, 400], "samples": [cfg.nv, cfg.nw], "steps": cfg.steps, "runs": a.runs, "blocks": a.blocks}
        where = [None]

        def to_command():
            t0 = time.perf_counter()
            eng.local_plan_async(where[0], WINDOW, dt=STEP_DT)
            eng.local_commands()
            return 1e6 * (time.perf_counter() - t0)

        print(json.dumps({"what": "gpu, no footprint: settled field -> command on the host", **base, **p50_blocks(to_command, a.runs, a.blocks)}), flush=True)
        if a.only_off:
            continue
        # the pose along the x axis at which the most samples survive under the footprint: the rollout's longest case
        xs = []
        for x in (1.0, 2.0, 3.0, 4.0, 5.0, 6.5, 8.0, 12.0, 16.0, 20.0):
            t = LP.pose_ticks((x, 0.0), 0.0, org, res)[0]
            if LP.stream_state_np(grid, pot, t, ncfg, gs) == 0 and LP.start_probe_np(grid, t, ncfg, feet["256 probes"]) < 0:
                xs.append((-int((LP.scores_np(grid, pot, t, WINDOW, ncfg, cfg, footprint=feet["56 probes"])[1] == LP.OK).sum()), x))
        assert xs, "no pose along the x axis at which the footprint is free"
        xs = [min(xs)[1]]
        where[0] = np.array([[xs[0], 0.0, 0.0]])
        pose = LP.pose_ticks((xs[0], 0.0), 0.0, org, res)[0]
        for label, foot in feet.items():
            for count in (0, 8):
                eng.set_local_footprint(foot)
                eng.set_local_movers(MOVERS if count else None, "costmap")
                mcfg = eng.local_movers_config("costmap")
                rows, n = walk(eng, count)
                eng.local_plan_async(where[0], WINDOW, dt=STEP_DT)
                info = eng.local_plan_info()
                more = {}
                if count:
                    table, n_movers, _ = LP.movers_np(rows, n, org, res, STEP_DT, mcfg)
                    more = dict(movers=table[:n_movers], mcfg=mcfg)
                want = LP.best_np(grid, pot, pose, WINDOW, ncfg, cfg, gs, footprint=foot, **more)
                names = LP.RESULT + LP.FOOT_INFO + (("n_dynamic", "near") if count else ())
                assert all(int(info[k][0]) == want[k] for k in names), "the stage does not equal best_np"
                assert int(info["score"][0]) == want["score"] and np.array_equal(eng.local_keys()[0], want["keys"])

                def host():
                    t0 = time.perf_counter()
                    kw = {}
                    if count:
                        tr, nt, _ = eng.tracks(1)
                        m, k, _ = LP.movers_np(tr[0], nt[0], org, res, STEP_DT, mcfg)
                        kw = dict(movers=m[:k], mcfg=mcfg)
                    g = eng._inflated(0, None, False)[0][0]
                    p = eng.navfn_fields()[0]
                    LP.best_np(g, p, pose, WINDOW, ncfg, cfg, gs, footprint=foot, **kw)
                    return 1e6 * (time.perf_counter() - t0)

                row = dict(base, footprint=label, movers=count, pose_x=float(xs[0]), info={k: int(v[0]) for k, v in info.items()})
                print(json.dumps({"what": "gpu: settled field -> command on the host", **row, **p50_blocks(to_command, a.runs, a.blocks)}), flush=True)
                print(json.dumps({"what": "host: fetch the inflated grid and the field (+ tracks and movers_np) + best_np (the restatement)", **row,
                                  **p50_blocks(host, a.host_runs, 1)}), flush=True)
                # ---- the kernels, profiled in runs of their own ----
                eng.set_profiling(True)
                times = {}
                for _ in range(max(a.runs // 5, 3)):
                    eng.local_plan_async(where[0], WINDOW, dt=STEP_DT)
                    eng.sync()
                    for k, ms in eng.kernel_times():
                        times.setdefault(k, []).append(1e3 * ms)
                eng.set_profiling(False)
                print(json.dumps({"what": "kernels", **row, **{k[2:] + "_median_us": round(float(np.median(v)), 2) for k, v in times.items()},
                                  **{k[2:] + "_max_us": round(max(v), 2) for k, v in times.items()}}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
