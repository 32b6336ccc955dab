"""Times of Soft-NMS on the GPU:

    python tools/soft_nms_bench.py [--reps 30] [--skip-standalone] [--skip-detector]

  detector    k_postprocess from Engine.kernel_times() on cfg-A at B = 1 and B = 64, one engine per batch size: the
              stand-up rule and the soft rule with methods hard / linear / gaussian, interleaved (every repetition runs
              the four one after the other on the same frames), median, minimum and maximum over --reps profiled passes.
  standalone  soft_nms wall time (host call, allocations and copies included) per method at n = 100, 1024 and 4096 dense
              boxes; the kernels' own times come from running this script under `rocprofv3 --kernel-trace --stats --`.
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

RULES = (("standup", None), ("soft", "hard"), ("soft", "linear"), ("soft", "gaussian"))


def select(eng, mode, method):
    eng.set_nms_mode(mode)
    if method is not None:
        eng.set_soft_nms(method=method)


def detector(reps):
    for B in (1, 64):
        eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=32768)
        eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
        frames = [pp.synth.d435i_cloud(i) for i in range(B)]
        rect, trv, _ = pp.synth.default_calib()
        rect, trv = np.stack([rect] * B), np.stack([trv] * B)
        kept = {}
        for mode, method in RULES:
            select(eng, mode, method)
            for _ in range(3):
                _, n = eng.detect(frames, rect, trv)
            kept[(mode, method)] = float(np.mean(n))
        us = {r: [] for r in RULES}
        eng.set_profiling(True)
        for _ in range(reps):
            for mode, method in RULES:
                select(eng, mode, method)
                eng.detect(frames, rect, trv)
                us[(mode, method)].append(1e3 * sum(ms for tag, ms in eng.kernel_times() if tag == "k_postprocess"))
        eng.set_profiling(False)
        for mode, method in RULES:
            t = np.array(us[(mode, method)])
            print(json.dumps({"what": "k_postprocess", "config": "cfg-A", "batch": B, "nms": mode, "method": method,
                              "reps": reps, "median_us": round(float(np.median(t)), 2), "min_us": round(float(t.min()), 2),
                              "max_us": round(float(t.max()), 2), "kept_mean": round(kept[(mode, method)], 2)}), flush=True)
        eng.close()


def standalone(reps):
    rng = np.random.default_rng(5)
    for n in (100, 1024, 4096):
        side = 45.0 * np.sqrt(n)
        xy = rng.uniform(0, side, (n, 2))
        dets = np.concatenate([xy, xy + rng.uniform(10.0, 60.0, (n, 2)), rng.uniform(0.02, 1.0, (n, 1))], axis=1).astype(np.float32)
        for method in ("hard", "linear", "gaussian"):
            keep, _ = pp.soft_nms.soft_nms(dets, method)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                pp.soft_nms.soft_nms(dets, method)
                ts.append((time.perf_counter() - t0) * 1e3)
            ts = np.array(ts)
            print(json.dumps({"what": "soft_nms wall", "n": n, "method": method, "kept": int(len(keep)), "reps": reps,
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
    if not a.skip_standalone:
        standalone(a.reps)


if __name__ == "__main__":
    main()
