"""Times of tracking on the GPU.  Reads nothing outside the repository.

    python tools/tracking_bench.py [--reps 200] [--off-only]

  kernel   k_track_step from Engine.kernel_times() (a device event pair around the launch) on cfg-A at B = 1 and B = 64,
           standalone (Engine.track_update) with 0, 8 and 64 live tracks per stream and as many rows, every track finding
           its row -- the association then takes as many dependent rounds as there are tracks -- and inside a profiled pass
           on that pass's own detections.  Median, minimum, maximum over --reps.
  pass     wall time of a whole pass on the resident frames (detect_async + sync: one graph replay) with tracking off and
           on, alternating in the same run, median and the 5th / 95th percentiles; the off figures of five blocks of --reps
           give the run-to-run spread.  --off-only runs just those (it touches no tracking call: it also runs on a tree
           without the feature, which is how the figure of the commit before it was taken).
  host     the alternative the kernel replaces: detections() + tracking.Tracker.step on the fetched rows, wall time.
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


def stats(us):
    t = np.asarray(us, np.float64)
    return {"median_us": round(float(np.median(t)), 2), "p05_us": round(float(np.percentile(t, 5)), 2),
            "p95_us": round(float(np.percentile(t, 95)), 2), "min_us": round(float(t.min()), 2), "max_us": round(float(t.max()), 2)}


def engine(B):
    eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=32768)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    frames = [pp.synth.d435i_cloud(i) for i in range(B)]
    rect, trv, _ = pp.synth.default_calib()
    dets, n = eng.detect(frames, np.stack([rect] * B), np.stack([trv] * B))
    return eng, float(np.mean(n))


def replay_us(eng, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.detect_async()
        eng.sync()
        out.append(1e6 * (time.perf_counter() - t0))
    return out


def seeded_rows(B, live, rows, jitter, rng):
    """`live` rows per stream on a 2 m lattice (far outside each other's gates), jittered by a few cm."""
    d = np.zeros((B, rows), pp.Engine.det_dtype())
    for k in range(live):
        d["box3d_lidar"][:, k, 0] = 2.0 * (k % 8) + rng.uniform(-jitter, jitter, B)
        d["box3d_lidar"][:, k, 1] = 2.0 * (k // 8) + rng.uniform(-jitter, jitter, B)
        d["box3d_lidar"][:, k, 3:6] = (0.6, 0.8, 1.7)
        d["score"][:, k] = 0.8
    return d, np.full(B, live, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--off-only", action="store_true")
    a = ap.parse_args()
    for B in (1, 64):
        eng, kept = engine(B)
        for _ in range(20):
            replay_us(eng, 1)
        for block in range(5):
            print(json.dumps({"what": "pass_wall", "batch": B, "tracking": "off", "block": block, "reps": a.reps,
                              "kept_mean": round(kept, 2), **stats(replay_us(eng, a.reps))}), flush=True)
        if a.off_only:
            eng.close()
            continue
        cfg = pp.tracking.TrackConfig(birth_score=0.0)
        rng = np.random.default_rng(1)
        rows = eng.detection_rows
        # ---- the kernel alone ----
        eng.set_tracking(cfg)
        eng.set_tracking(None)
        eng.set_profiling(True)
        for live in (0, 8, 64):
            r = max(rows, live)          # (track_update takes up to 128 rows whatever the engine's own row count)
            eng.track_reset()
            eng.track_update(*seeded_rows(B, live, r, 0.0, rng))
            us = []
            for _ in range(a.reps):
                _, nt, _ = eng.track_update(*seeded_rows(B, live, r, 0.03, rng))
                assert (nt == live).all()
                us.append(1e3 * sum(ms for tag, ms in eng.kernel_times() if tag == "k_track_step"))
            print(json.dumps({"what": "k_track_step", "batch": B, "live": live, "rows": live, "reps": a.reps, **stats(us)}), flush=True)
        # ---- inside a profiled pass ----
        eng.track_reset()
        eng.set_tracking(cfg)
        us, tot = [], []
        for _ in range(min(a.reps, 50)):
            eng.detect_async()
            eng.sync()
            kt = eng.kernel_times()
            us.append(1e3 * sum(ms for tag, ms in kt if tag == "k_track_step"))
            tot.append(1e3 * sum(ms for _, ms in kt))
        _, nt, _ = eng.tracks()
        print(json.dumps({"what": "k_track_step in a pass", "batch": B, "tracks_mean": round(float(nt.mean()), 2),
                          "kernels_sum_median_us": round(float(np.median(tot)), 2), **stats(us)}), flush=True)
        eng.set_profiling(False)
        # ---- the whole pass, off and on alternating ----
        off, on = [], []
        for _ in range(10):
            eng.set_tracking(None)
            replay_us(eng, 5)
            off += replay_us(eng, a.reps // 10)
            eng.set_tracking(cfg)
            replay_us(eng, 5)
            on += replay_us(eng, a.reps // 10)
        print(json.dumps({"what": "pass_wall alternating", "batch": B, "tracking": "off", **stats(off)}), flush=True)
        print(json.dumps({"what": "pass_wall alternating", "batch": B, "tracking": "on", **stats(on)}), flush=True)
        # ---- the host alternative: fetch, then the numpy restatement ----
        eng.set_tracking(None)
        ref = pp.tracking.Tracker(cfg, B)
        host = []
        for _ in range(min(a.reps, 50)):
            eng.detect_async()
            eng.sync()
            t0 = time.perf_counter()
            dets, n = eng.detections()
            ref.step(dets, n)
            host.append(1e6 * (time.perf_counter() - t0))
        print(json.dumps({"what": "host alternative: detections() + Tracker.step", "batch": B,
                          "tracks_mean": round(float(ref.info()["live"][:B].mean()), 2), **stats(host)}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
