"""Times of the image-box projection on the GPU:

    python tools/bbox_bench.py [--reps 30] [--skip-standalone] [--skip-detector]

  detector    k_postprocess from Engine.kernel_times(), projection off against on, at cfg-A B = 1 and B = 64: per setting
              the median, minimum and maximum over --reps profiled passes on the same frames (off, on, off again).  On a
              tree without the projection (the parent commit) only the off rows are printed: the comparison the claim
              "off is unchanged" is judged by, against that run's own spread.
  standalone  box3d_to_bbox_gpu wall time (host call, allocations and copies included) at n = 50 and n = 100 000; the
              kernel's own time comes from running this script under `rocprofv3 --kernel-trace --stats --`.
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

P2 = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884], [0, 0, 0, 1]])


def post_times(eng, frames, rect, trv, reps, **kw):
    eng.set_profiling(False)
    for _ in range(3):
        eng.detect(frames, rect, trv, **kw)
    eng.set_profiling(True)
    out = []
    for _ in range(reps):
        eng.detect(frames, rect, trv, **kw)
        out.append(sum(ms for tag, ms in eng.kernel_times() if tag == "k_postprocess"))
    eng.set_profiling(False)
    return np.array(out) * 1e3


def detector(reps):
    for B in (1, 64):
        eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=32768)
        eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
        frames = [pp.synth.d435i_cloud(i) for i in range(B)]
        rect, trv, _ = pp.synth.default_calib()
        rect, trv = np.stack([rect] * B), np.stack([trv] * B)
        has = hasattr(eng, "set_projection")
        for on in ((False, True, False) if has else (False, False)):
            if has:
                eng.set_projection(P2 if on else None)
            kw = dict(p2=P2, bbox=True) if on else {}
            _, n = eng.detect(frames, rect, trv, **kw)
            us = post_times(eng, frames, rect, trv, reps, **kw)
            print(json.dumps({"what": "k_postprocess", "config": "cfg-A", "batch": B, "projection": on, "reps": reps,
                              "median_us": round(float(np.median(us)), 2), "min_us": round(float(us.min()), 2),
                              "max_us": round(float(us.max()), 2), "kept_mean": round(float(np.mean(n)), 2)}), flush=True)
        eng.close()


def standalone(reps):
    rng = np.random.default_rng(5)
    for n in (50, 100000):
        z = rng.uniform(2.0, 40.0, n)
        boxes = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(0.8, 2.2, n), z, rng.uniform(0.4, 4.5, n),
                          rng.uniform(1.3, 1.9, n), rng.uniform(0.4, 2.0, n), rng.uniform(-6.28, 6.28, n)], axis=1)
        pp.projection.box3d_to_bbox_gpu(boxes, [n], P2)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            pp.projection.box3d_to_bbox_gpu(boxes, [n], P2)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = np.array(ts)
        print(json.dumps({"what": "box3d_to_bbox_gpu wall", "n": n, "reps": reps, "median_ms": round(float(np.median(ts)), 3),
                          "min_ms": round(float(ts.min()), 3), "max_ms": round(float(ts.max()), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--skip-standalone", action="store_true")
    ap.add_argument("--skip-detector", action="store_true")
    a = ap.parse_args()
    if not a.skip_detector:
        detector(a.reps)
    if not a.skip_standalone and hasattr(pp, "projection"):
        standalone(a.reps)


if __name__ == "__main__":
    main()
