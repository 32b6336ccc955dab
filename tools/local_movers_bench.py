"""Times of the local planner's movers on the GPU.  Reads nothing outside the repository.

    python tools/local_movers_bench.py [--runs 50] [--blocks 5] [--host-runs 3]

The scenes, the window and the samples of tools/local_plan_bench.py: a 400 x 400 window of 0.1 m cells at batch 1, 33 x 41
samples, 64 steps.  The tracker is fed 0, 8 or 64 pedestrians on a grid of 0.7 m x 0.8 m in front of the robot, walking
across its way at 0.5 m/s, three steps each so that every track is confirmed; a rollout step lasts 0.1 s, the horizon is
the whole rollout.  Measured from the settled field (navfn_fields has returned):
  off      the stage off: Engine.local_plan_async + local_commands, the figure of tools/local_plan_bench.py.
  command  the stage on: the same two calls, which now queue k_local_movers, the rollout and the finish with movers.
           p50 of --runs, repeated --blocks times: the median of the blocks' p50 with their min - max.
  host     the route the stage replaces, on the same commit: tracks(), local_planner.movers_np, the inflated grid and the
           field fetched, then local_planner.best_np with the movers -- the restatement in numpy, not a tuned CPU planner.
  kernels  k_local_movers, k_local_rollout_movers and k_local_finish_movers from Engine.kernel_times().
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
from local_plan_bench import LOCAL, WINDOW  # noqa: E402
from navfn_bench import COSTMAP, GOAL, p50_blocks, scene  # noqa: E402

MOVERS = dict(horizon=64, mover_weight=64, pad_hard=0.3, pad_soft=0.8, confirmed_only=True)
STEP_DT = 0.1           # seconds per rollout step: a cell per step is 1 m/s


def walk(eng, count):
    """Three tracking steps of 0.1 s on `count` pedestrians (0: the tables are emptied)."""
    eng.track_reset()
    d = np.zeros((1, max(count, 1)), pp.engine.DET_DTYPE)
    for k in range(3):
        for i in range(count):
            d["box3d_lidar"][0, i] = (1.0 + 0.7 * (i // 8), -2.8 + 0.8 * (i % 8) + 0.05 * k, 0.0, 0.5, 0.5, 1.7, 0.0)
            d["score"][0, i] = 0.9
        tr, n, _ = eng.track_update(d, [count], [0.1])
    assert n[0] == count and (tr["confirmed"][0, :count] == 1).all()
    return tr[0], int(n[0])


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
    eng.set_tracking(True)
    ncfg, cfg = eng.navfn_config("costmap"), eng.local_planner_config("costmap")
    org, res = (COSTMAP["x_min"], COSTMAP["y_min"]), COSTMAP["resolution"]
    pose = LP.pose_ticks((0.0, 0.0), 0.0, org, res)[0]
    for name in ("open", "wall"):
        eng.upload([scene(name)])
        eng._plan_async(GOAL, "costmap", None)
        pot = eng.navfn_fields()[0]                      # the settled field: the span starts here
        grid = eng._inflated(0, None, False)[0][0]
        gs = int(eng.navfn_info()["goal_state"][0])
        base = {"scene": name, "batch": 1, "window": [400, 400], "samples": [cfg.nv, cfg.nw], "steps": cfg.steps, "runs": a.runs, "blocks": a.blocks}

        def to_command():
            t0 = time.perf_counter()
            eng.local_plan_async(None, WINDOW, dt=STEP_DT)
            eng.local_commands()
            return 1e6 * (time.perf_counter() - t0)

        eng.set_local_movers(None, "costmap")
        print(json.dumps({"what": "gpu, the stage off: settled field -> command on the host", **base, **p50_blocks(to_command, a.runs, a.blocks)}), flush=True)
        eng.set_local_movers(MOVERS, "costmap")
        mcfg = eng.local_movers_config("costmap")
        for count in (0, 8, 64):
            rows, n = walk(eng, count)
            eng.local_plan_async(None, WINDOW, dt=STEP_DT)
            info = eng.local_plan_info()
            table, n_movers, skipped = LP.movers_np(rows, n, org, res, STEP_DT, mcfg)
            want = LP.best_np(grid, pot, pose, WINDOW, ncfg, cfg, gs, movers=table[:n_movers], mcfg=mcfg)
            assert n_movers == count and np.array_equal(eng.local_movers()[0][0], table), "the table does not equal movers_np"
            assert all(int(info[k][0]) == want[k] for k in LP.RESULT + ("n_movers", "n_dynamic", "near")), "the stage does not equal best_np"
            assert int(info["score"][0]) == want["score"] and np.array_equal(eng.local_keys()[0], want["keys"])

            def host():
                t0 = time.perf_counter()
                tr, nt, _ = eng.tracks(1)
                m, k, _ = LP.movers_np(tr[0], nt[0], org, res, STEP_DT, mcfg)
                g = eng._inflated(0, None, False)[0][0]
                p = eng.navfn_fields()[0]
                LP.best_np(g, p, pose, WINDOW, ncfg, cfg, gs, movers=m[:k], mcfg=mcfg)
                return 1e6 * (time.perf_counter() - t0)

            row = dict(base, movers=count, info={k: int(v[0]) for k, v in info.items()})
            print(json.dumps({"what": "gpu: settled field -> command on the host", **row, **p50_blocks(to_command, a.runs, a.blocks)}), flush=True)
            print(json.dumps({"what": "host: tracks + movers_np + fetch the inflated grid and the field + best_np (the restatement)", **row,
                              **p50_blocks(host, a.host_runs, 1)}), flush=True)
            # ---- the kernels, profiled in runs of their own ----
            eng.set_profiling(True)
            times = {"k_local_movers": [], "k_local_rollout_movers": [], "k_local_finish_movers": []}
            for _ in range(max(a.runs // 5, 3)):
                eng.local_plan_async(None, WINDOW, dt=STEP_DT)
                eng.sync()
                for k, ms in eng.kernel_times():
                    times[k].append(1e3 * ms)
            eng.set_profiling(False)
            print(json.dumps({"what": "kernels", **row, **{k[2:] + "_median_us": round(float(np.median(v)), 2) for k, v in times.items()},
                              **{k[2:] + "_max_us": round(max(v), 2) for k, v in times.items()}}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
