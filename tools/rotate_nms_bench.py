"""Times of the rotated NMS on the GPU ("rotated NMS"):

    python tools/rotate_nms_bench.py [--reps 30] [--skip-standalone] [--skip-detector]

  detector    k_postprocess from Engine.kernel_times(), stand-up against rotated rule, at cfg-A B = 64 and cfg-K (two
              classes) B = 32: per mode the median, minimum and maximum over --reps profiled passes on the same frames.
              On a tree without the mode (the parent commit) only the stand-up rows are printed: the comparison the
              default-mode claim "unchanged" is judged by, against that run's own spread.
  standalone  rotate_nms wall time (host call, allocations and copies included) at n = 100, 1 000 and 10 000; the
              kernels' own times come from running this script under `rocprofv3 --kernel-trace --stats --`.
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


def post_times(eng, frames, rect, trv, reps):
    eng.set_profiling(False)
    for _ in range(3):
        eng.detect(frames, rect, trv)
    eng.set_profiling(True)
    out = []
    for _ in range(reps):
        eng.detect(frames, rect, trv)
        out.append(sum(ms for tag, ms in eng.kernel_times() if tag == "k_postprocess"))
    eng.set_profiling(False)
    return np.array(out) * 1e3


def detector(reps):
    cases = (("cfg-A", pp.config.pedestrian_d435i_config(64), 64, 32768, lambda i: pp.synth.d435i_cloud(i)),
             ("cfg-K", pp.config.kitti_shaped_config(32, num_class=2), 32, 24000, lambda i: pp.synth.kitti_cloud(i)))
    for name, cfg, B, nmax, cloud in cases:
        eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=nmax)
        eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
        frames = [cloud(i) for i in range(B)]
        rect, trv, _ = pp.synth.default_calib()
        rect, trv = np.stack([rect] * B), np.stack([trv] * B)
        modes = ("standup", "rotated", "standup") if hasattr(eng, "set_nms_mode") else ("standup", "standup")
        for mode in modes:
            if hasattr(eng, "set_nms_mode"):
                eng.set_nms_mode(mode)
            _, n = eng.detect(frames, rect, trv)
            us = post_times(eng, frames, rect, trv, reps)
            print(json.dumps({"what": "k_postprocess", "config": name, "batch": B, "nms": mode, "reps": reps,
                              "median_us": round(float(np.median(us)), 2), "min_us": round(float(us.min()), 2),
                              "max_us": round(float(us.max()), 2), "kept_mean": round(float(np.mean(n)), 2)}), flush=True)
        eng.close()


def standalone(reps):
    rng = np.random.default_rng(5)
    for n in (100, 1000, 10000):
        side = 1.6 * np.sqrt(n)
        dets = np.concatenate([rng.uniform(0, side, (n, 2)), rng.uniform(0.5, 2.5, (n, 2)), rng.uniform(-3.5, 3.5, (n, 1)),
                               (rng.permutation(n)[:, None] + 0.5) / n], axis=1).astype(np.float32)
        keep = pp.rotate_nms.rotate_nms(dets, 0.5)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            pp.rotate_nms.rotate_nms(dets, 0.5)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = np.array(ts)
        print(json.dumps({"what": "rotate_nms wall", "n": n, "kept": int(len(keep)), "reps": reps,
                          "median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(ts.min()), 3),
                          "max_ms": round(float(ts.max()), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--skip-standalone", action="store_true")
    ap.add_argument("--skip-detector", action="store_true")
    a = ap.parse_args()
    if not a.skip_detector:
        detector(a.reps)
    if not a.skip_standalone and hasattr(pp, "rotate_nms"):
        standalone(a.reps)


if __name__ == "__main__":
    main()
