"""Feeding a 4-feature model (x y z intensity) a lidar's PointCloud2 message through the GPU ingest
(csrc/ingest.hip: k_ingest_scatter_f) vs parsing the message on the host and uploading the array; prints one JSON line.

One synthetic lidar-sized message -- 120 000 records in one row, point_step 32, FLOAT32 x y z at 0 / 4 / 8, FLOAT32
intensity at 16, UINT16 ring at 20, 5 % of the records NaN -- on a 4-feature KITTI-shaped engine under the identity mount,
first 0, decimate 1, all in one process; p50 over --reps repetitions of

  a  message:     Engine.detect_pointcloud2(features=[FeatureField("intensity")], mount=identity), batch 1 (host clock,
                  ends in a synchronise; pageable bytes)
  b  host parse:  ingest.pointcloud2_to_points on the host, then Engine.detect on the array (the same clock) -- what a
                  lidar user had to do before the feature ingest
  pass            the detection pass alone on the ingested frame (HIP-event stopwatch around pp_detect_async)

The legs alternate within a round, and the p50 is taken --rounds times: the minimum and maximum of the p50s are
reported, so the run-to-run spread is on the page.  Also the count / scan / scatter kernels' times at batch 1 and batch
16 from per-launch events (pp_set_profiling), the 3-feature scatter on the same bytes beside them.  The detections of the
two feeds are checked to be equal before anything is timed.

    python tools/ingest_features_bench.py [--reps 50] [--rounds 5]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pp_amd as pp  # noqa: E402

N_REC = 120000
NMAX = 120000
KERNELS4 = ("k_ingest_count", "k_ingest_scan", "k_ingest_scatter_f<4>")
KERNELS3 = ("k_ingest_count", "k_ingest_scan", "k_ingest_scatter")


def p50(xs):
    return float(np.median(xs))


def config(B, F):
    cfg = copy.deepcopy(pp.config.kitti_shaped_config(B))
    cfg["model"]["second"]["num_point_features"] = F
    for reader in ("eval_input_reader", "train_input_reader"):
        if reader in cfg:
            cfg[reader]["num_point_features"] = F
    return cfg


def message(frame):
    pts = pp.synth.kitti_cloud(frame, N_REC).astype(np.float64)
    rng = np.random.default_rng(frame)
    bad = rng.random(N_REC) < 0.05
    pts[bad, rng.integers(0, 3, int(bad.sum()))] = np.nan
    return pp.synth.pointcloud2_from_points(pts, N_REC, 1, feature_fields=[("intensity", 7, 16)], point_step=32,
                                            extra_fields=[("ring", 20, 4, 1)], seed=frame)


def kernel_leg(feed, kernels, B, F, reps):
    """feed(eng): one synchronous ingest of B frames.  p50 of each kernel's event time, microseconds."""
    eng = pp.Engine(config(B, F), max_batch=B, max_points_per_frame=NMAX)
    for _ in range(3):
        feed(eng)                                    # allocates the staging; warm-up
    eng.set_profiling(True)
    per = []
    for _ in range(reps):
        feed(eng)
        per.append({k: ms for k, ms in eng.kernel_times() if k in kernels})
    eng.set_profiling(False)
    eng.close()
    return {"batch": B, "us": round(p50([sum(p.values()) for p in per]) * 1e3, 2),
            "kernel_us": {k: round(p50([p[k] for p in per]) * 1e3, 2) for k in kernels}}


def same(a, b):
    return np.array_equal(a[1], b[1]) and a[0][0, :a[1][0]].tobytes() == b[0][0, :b[1][0]].tobytes()


def frame_legs(msg, feats, mount, reps, rounds):
    eng = pp.Engine(config(1, 4), max_batch=1, max_points_per_frame=NMAX)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))

    def host_parse():
        return eng.detect([np.ascontiguousarray(pp.ingest.pointcloud2_to_points(msg, feats), np.float32)])

    legs = {"a_message_features_ms": lambda: eng.detect_pointcloud2([msg], features=feats, mount=mount, first=0, decimate=1),
            "b_host_parse_detect_ms": host_parse}
    want = None
    for name, fn in legs.items():
        for _ in range(3):
            got = fn()
        got = (got[0].copy(), got[1].copy())
        want = got if want is None else want
        assert same(got, want), name
    p50s = {name: [] for name in legs}
    for _ in range(rounds):
        ts = {name: [] for name in legs}
        for _ in range(reps):
            for name, fn in legs.items():            # alternating: every leg sees the same machine state
                t0 = time.perf_counter()
                fn()
                ts[name].append(time.perf_counter() - t0)
        for name in legs:
            p50s[name].append(p50(ts[name]) * 1e3)
    out = {name: {"p50_min": round(min(v), 4), "p50_max": round(max(v), 4)} for name, v in p50s.items()}
    eng.ingest_pointcloud2([msg], first=0, decimate=1, features=feats, mount=mount)
    ts = []
    for i in range(reps + 3):
        eng.timer_start()
        eng.detect_async()
        t = eng.timer_stop()
        if i >= 3:
            ts.append(t)
    out["detect_pass_ms"] = round(p50(ts), 4)
    info = eng.ingest_info()
    out["finite_records"], out["kept_points"] = int(info["finite"][0]), int(info["kept"][0])
    out["detections"] = int(want[1][0])
    eng.sync()
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    reps, rounds = max(args.reps, 50), max(args.rounds, 1)
    feats = [pp.ingest.FeatureField("intensity")]
    mount = pp.ingest.Mount(np.eye(3), np.eye(3), 0.0)
    msg = message(0)
    res = {"reps": reps, "rounds": rounds, "message": f"{N_REC} records x point_step 32, FLOAT32 intensity at 16, 5 % NaN",
           "bytes_copied_per_frame": {"message": msg[2] * msg[4], "host_parsed_array": "kept_points x 16"}}
    res.update(frame_legs(msg, feats, mount, reps, rounds))
    for B in (1, 16):
        msgs = [message(i) for i in range(B)]
        kw = dict(first=0, decimate=1, mount=mount)
        res[f"feature_kernels_b{B}"] = kernel_leg(lambda e: e.ingest_pointcloud2(msgs, features=feats, **kw), KERNELS4, B, 4, reps)
        res[f"xyz_kernels_b{B}"] = kernel_leg(lambda e: e.ingest_pointcloud2(msgs, **kw), KERNELS3, B, 3, reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
