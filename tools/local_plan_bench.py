"""Times of the local planner on the GPU.  Reads nothing outside the repository.

    python tools/local_plan_bench.py [--runs 50] [--blocks 5] [--host-runs 3]

The scenes and the window of tools/navfn_bench.py: behind the costmap's point layer, its inflation and its navigation
function on a 400 x 400 window of 0.1 m cells at batch 1, the goal at the window's far edge, the robot at the sensor's own
cell along +x; 33 x 41 samples (sv 0 .. 1024 by 32, sw -160 .. 160 by 8), 64 steps, a lookahead of two cells.  Measured from
the settled field (navfn_fields has returned):
  command  wall time to the command in host memory: Engine.local_plan_async + local_commands.  p50 of --runs, repeated
           --blocks times: the median of the blocks' p50 with their min - max.
  host     the route the stage replaces, on the same commit: the inflated grid and the field fetched, then
           local_planner.best_np on them -- the restatement in numpy, not a tuned CPU planner.
  kernels  k_local_rollout and k_local_finish from Engine.kernel_times() (a device event pair around each launch).
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
from navfn_bench import COSTMAP, GOAL, p50_blocks, scene  # noqa: E402

LOCAL = dict(nv=33, nw=41, steps=64, lookahead=2048, pot_weight=32, occ_weight=16, speed_weight=1, turn_weight=1)
WINDOW = (0, 32, -160, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    a = ap.parse_args()
    LP = pp.local_planner
    eng = pp.Engine(pp.config.pedestrian_d435i_config(1), max_batch=1, max_points_per_frame=16384)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    eng.set_costmap(COSTMAP)
    eng.set_inflation(True, "costmap")
    eng.set_navfn(dict(allow_unknown=1), "costmap")      # the point layer leaves the cells no return fell into unknown
    eng.set_local_planner(LOCAL, "costmap")
    ncfg, cfg = eng.navfn_config("costmap"), eng.local_planner_config("costmap")
    for name in ("open", "wall"):
        eng.upload([scene(name)])
        eng._plan_async(GOAL, "costmap", None)
        pot = eng.navfn_fields()[0]                      # the settled field: the span starts here
        grid = eng._inflated(0, None, False)[0][0]
        gs = int(eng.navfn_info()["goal_state"][0])
        eng.local_plan_async(None, WINDOW)
        info = eng.local_plan_info()
        pose = LP.pose_ticks((0.0, 0.0), 0.0, (COSTMAP["x_min"], COSTMAP["y_min"]), COSTMAP["resolution"])[0]
        want = LP.best_np(grid, pot, pose, WINDOW, ncfg, cfg, gs)
        assert all(int(info[k][0]) == want[k] for k in LP.RESULT) and int(info["score"][0]) == want["score"], "the stage does not equal best_np"
        assert np.array_equal(eng.local_keys()[0], want["keys"]) and np.array_equal(eng.local_trajectories()[0], want["traj"])

        def to_command():
            t0 = time.perf_counter()
            eng.local_plan_async(None, WINDOW)
            eng.local_commands()
            return 1e6 * (time.perf_counter() - t0)

        def host():
            t0 = time.perf_counter()
            g = eng._inflated(0, None, False)[0][0]
            p = eng.navfn_fields()[0]
            LP.best_np(g, p, pose, WINDOW, ncfg, cfg, gs)
            return 1e6 * (time.perf_counter() - t0)

        base = {"scene": name, "batch": 1, "window": [400, 400], "samples": [cfg.nv, cfg.nw], "steps": cfg.steps,
                "info": {k: int(v[0]) for k, v in info.items()}, "runs": a.runs, "blocks": a.blocks}
        print(json.dumps({"what": "gpu: settled field -> command on the host", **base, **p50_blocks(to_command, a.runs, a.blocks)}), flush=True)
        print(json.dumps({"what": "host: fetch the inflated grid and the field + best_np (the restatement)", **base,
                          **p50_blocks(host, a.host_runs, 1)}), flush=True)
        # ---- the kernels, profiled in runs of their own ----
        eng.set_profiling(True)
        times = {"k_local_rollout": [], "k_local_finish": []}
        for _ in range(max(a.runs // 5, 3)):
            eng.local_plan_async(None, WINDOW)
            eng.sync()
            for k, ms in eng.kernel_times():
                times[k].append(1e3 * ms)
        eng.set_profiling(False)
        print(json.dumps({"what": "kernels", **base, "rollout_median_us": round(float(np.median(times["k_local_rollout"])), 2),
                          "rollout_max_us": round(max(times["k_local_rollout"]), 2),
                          "finish_median_us": round(float(np.median(times["k_local_finish"])), 2),
                          "finish_max_us": round(max(times["k_local_finish"]), 2)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
