"""What the AP evaluator's matching statistics cost on the host and on the GPU.

    python tools/eval_stats_bench.py [--frames 3769] [--host-frames 120] [--reps 5]

3 769 seeded synthetic frames (the size of KITTI val; tools/gen_golden_eval.py's make_annos scaled to KITTI-like
counts: 2..11 labelled objects and their jittered detections plus 0..7 false positives per frame), one class,
`get_official_eval_result` with the 2D metric: 3 metrics x 3 difficulties x 6 overlap tiers.

  statistics="gpu"  : the whole evaluation, `reps` times; reported are the medians of the wall time of the
                      statistics part (pack_frames + match_frames_gpu + get_thresholds + pr_frames_gpu) and of the
                      two entry points' kernel times (device events around the launches, summed over the 9 calls each).
  statistics="host" : the same evaluation on the first `host-frames` frames, once; the time inside
                      compute_statistics is scaled by frames / host-frames (the calls are per frame and per
                      threshold, and the number of thresholds saturates at 41 well below the subset's size).
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pp_amd  # noqa: E402

ke = pp_amd.kitti_eval


def make_annos(nframes, seed=11):
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for f in range(nframes):
        n = int(rng.integers(2, 12))
        loc = np.stack([rng.uniform(-20, 20, n), rng.uniform(0.2, 1.4, n), rng.uniform(4.0, 60.0, n)], 1)
        dims = np.stack([rng.uniform(0.5, 0.9, n), rng.uniform(1.5, 1.9, n), rng.uniform(0.5, 0.9, n)], 1)
        rot = rng.uniform(-np.pi, np.pi, n)
        names = np.array(["Pedestrian"] * n, dtype="<U16")
        names[rng.uniform(size=n) < 0.2] = "Cyclist"
        names[rng.uniform(size=n) < 0.1] = "Person_sitting"
        names[rng.uniform(size=n) < 0.1] = "DontCare"
        x1, y1 = rng.uniform(0, 1100, n), rng.uniform(100, 250, n)
        bbox = np.stack([x1, y1, x1 + rng.uniform(20, 90, n), y1 + rng.uniform(20, 120, n)], 1)
        gts.append({"name": names, "truncated": rng.choice([0.0, 0.1, 0.25, 0.4], n), "occluded": rng.integers(0, 3, n),
                    "alpha": -np.arctan2(-loc[:, 0], loc[:, 2]) + rot, "bbox": bbox, "dimensions": dims, "location": loc,
                    "rotation_y": rot})
        keep = rng.uniform(size=n) < 0.8
        nk, nfp = int(keep.sum()), int(rng.integers(0, 8))
        dloc = np.concatenate([loc[keep] + rng.normal(0, 0.05, (nk, 3)),
                               np.stack([rng.uniform(-20, 20, nfp), rng.uniform(0.2, 1.4, nfp), rng.uniform(4, 60, nfp)], 1)], 0)
        ddims = np.concatenate([dims[keep] * rng.uniform(0.95, 1.05, (nk, 3)), np.tile([[0.7, 1.7, 0.7]], (nfp, 1))], 0)
        drot = np.concatenate([rot[keep] + rng.normal(0, 0.1, nk), rng.uniform(-np.pi, np.pi, nfp)], 0)
        fx1, fy1 = rng.uniform(0, 1100, nfp), rng.uniform(100, 250, nfp)
        dbox = np.concatenate([bbox[keep] + rng.normal(0, 3, (nk, 4)),
                               np.stack([fx1, fy1, fx1 + rng.uniform(20, 90, nfp), fy1 + rng.uniform(20, 120, nfp)], 1)], 0)
        nd = nk + nfp
        dnames = np.array(["Pedestrian"] * nd, dtype="<U16")
        dnames[rng.uniform(size=nd) < 0.15] = "Cyclist"
        dts.append({"name": dnames, "truncated": np.zeros(nd), "occluded": np.zeros(nd, dtype=np.int64),
                    "alpha": -np.arctan2(-dloc[:, 0], dloc[:, 2]) + drot, "bbox": dbox, "dimensions": ddims, "location": dloc,
                    "rotation_y": drot, "score": rng.uniform(0.05, 0.99, nd).astype(np.float32)})
    return gts, dts


class Clock:
    """Wraps functions of kitti_eval and adds up the wall time spent inside them."""

    def __init__(self, names, kernel_lists=None):
        self.seconds = 0.0
        self.calls = 0
        self.saved = {n: getattr(ke, n) for n in names}
        self.kernel_lists = kernel_lists or {}

    def __enter__(self):
        for name, fn in self.saved.items():
            setattr(ke, name, self._timed(name, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(ke, name, fn)

    def _timed(self, name, fn):
        def wrapper(*a, **k):
            if name in self.kernel_lists:
                k["kernel_ms"] = self.kernel_lists[name]
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.seconds += time.perf_counter() - t0
                self.calls += 1
        return wrapper


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--host-frames", type=int, default=120)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    pp_amd._lib.build()
    gts, dts = make_annos(a.frames)
    ke.get_official_eval_result(gts[:60], dts[:60], ["Pedestrian"], statistics="gpu")       # warm the device up

    stat_wall, total_wall, k_match, k_pr, text_gpu = [], [], [], [], None
    for _ in range(a.reps):
        lists = {"match_frames_gpu": [], "pr_frames_gpu": []}
        with Clock(["pack_frames", "match_frames_gpu", "get_thresholds", "pr_frames_gpu"], lists) as c:
            t0 = time.perf_counter()
            text_gpu = ke.get_official_eval_result(gts, dts, ["Pedestrian"], statistics="gpu")[0]
            total_wall.append(time.perf_counter() - t0)
        stat_wall.append(c.seconds)
        k_match.append(sum(lists["match_frames_gpu"]))
        k_pr.append(sum(lists["pr_frames_gpu"]))

    sub = min(a.host_frames, a.frames)
    with Clock(["compute_statistics"]) as c:
        t0 = time.perf_counter()
        text_host = ke.get_official_eval_result(gts[:sub], dts[:sub], ["Pedestrian"], statistics="host")[0]
        host_total = time.perf_counter() - t0
    text_gpu_sub = ke.get_official_eval_result(gts[:sub], dts[:sub], ["Pedestrian"], statistics="gpu")[0]
    print(json.dumps({
        "frames": a.frames, "objects": int(sum(len(g["name"]) for g in gts)), "detections": int(sum(len(d["name"]) for d in dts)),
        "gpu_statistics_wall_s": float(np.median(stat_wall)), "gpu_evaluation_wall_s": float(np.median(total_wall)),
        "gpu_match_kernels_ms": float(np.median(k_match)), "gpu_pr_kernels_ms": float(np.median(k_pr)), "reps": a.reps,
        "host_frames": sub, "host_statistics_calls": c.calls, "host_statistics_wall_s": c.seconds,
        "host_evaluation_wall_s": host_total, "host_us_per_call": 1e6 * c.seconds / max(1, c.calls),
        "host_statistics_wall_s_scaled": c.seconds * a.frames / sub,
        "reports_equal_on_subset": text_host == text_gpu_sub, "report_lines": text_gpu.count("\n"),
    }))


if __name__ == "__main__":
    main()
