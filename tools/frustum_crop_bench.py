"""The frustum crop on the host vs on the GPU (csrc/frustum_crop.hip); prints one JSON line.

synth.kitti_cloud-shaped frames widened to a full sweep (x mirrored for half the points, so ~3/4 of a frame lies outside
the image) of ~120 k points x 4 features, cfg-K, max_points_per_frame = 131072, KITTI-like calibration.

  kernels  k_crop_count + k_crop_scan + k_crop_scatter by HIP events (the per-launch events of pp_set_profiling), median
           of 5, at batch 1 and batch 32; achieved byte rate = (2 x cloud bytes + kept bytes) / time, beside
           Engine.device_copy_GBps of the same run (the second read may hit the last-level cache: the rate is what the
           kernels achieve, not an HBM measurement)
  reduce   gt_database.create_reduced_point_cloud over 32 frames, frames/s: engine (max_batch 32) against engine=None
           (frustum.remove_outside_points_np, the parent commit's only option), files written to a temporary directory
  detect   batch 1, host clock, median: Engine.detect on the raw frame; Engine.detect(p2=, image_shape=) (upload + GPU
           crop + pass); host crop + Engine.detect of the cropped frame (the parent commit's only way to a cropped pass)

    python tools/frustum_crop_bench.py [--reps 5]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pp_amd as pp  # noqa: E402

KERNELS = ("k_crop_count", "k_crop_scan", "k_crop_scatter")
NMAX = 131072
N_POINTS = 120000
IMAGE = (375, 1242)


def calib():
    rect = np.eye(4)
    trv2c = np.eye(4)
    trv2c[:3, :3] = [[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]
    trv2c[:3, 3] = [0.0, -0.08, -0.27]
    p2 = np.array([[720.0, 0, 610.0, 45.0], [0, 720.0, 172.0, 0.2], [0, 0, 1.0, 0.003], [0, 0, 0, 1.0]])
    return rect, trv2c, p2


def sweep(frame):
    """A full 360-degree sweep: kitti_cloud's forward fan, every second point mirrored behind the sensor and the fan
    opened to +-pi/2 by swapping x and y for a quarter of them."""
    p = pp.synth.kitti_cloud(frame, N_POINTS).copy()
    p[1::2, 0] = -p[1::2, 0]
    q = p[::4].copy()
    p[::4, 0], p[::4, 1] = q[:, 1], q[:, 0]
    return np.ascontiguousarray(p, np.float32)


def med(xs):
    return float(np.median(xs))


def kernel_leg(frames, planes, reps):
    B = len(frames)
    eng = pp.Engine(pp.config.kitti_shaped_config(B), max_batch=B, max_points_per_frame=NMAX)
    for _ in range(2):
        eng.upload(frames)
        kept = eng.crop_to_image(planes)
    eng.set_profiling(True)
    per = []
    for _ in range(reps):
        eng.upload(frames)
        eng.crop_to_image(planes)
        per.append({k: ms for k, ms in eng.kernel_times() if k in KERNELS})
    eng.set_profiling(False)
    copy = eng.device_copy_GBps()
    eng.close()
    total_us = med([sum(p.values()) for p in per]) * 1e3
    n_in = sum(len(f) for f in frames)
    nbytes = (2 * n_in + int(kept.sum())) * 16
    return {"batch": B, "points": n_in, "kept": int(kept.sum()), "us": round(total_us, 2),
            "kernel_us": {k: round(med([p[k] for p in per]) * 1e3, 2) for k in KERNELS},
            "us_min_max": [round(min(sum(p.values()) for p in per) * 1e3, 2), round(max(sum(p.values()) for p in per) * 1e3, 2)],
            "bytes": nbytes, "GBps": round(nbytes / (total_us * 1e-6) / 1e9, 1), "device_copy_GBps": round(copy, 1)}


def reduce_leg(frames, infos, reps):
    eng = pp.Engine(pp.config.kitti_shaped_config(32), max_batch=32, max_points_per_frame=NMAX)
    gdb = pp.gt_database
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for name, e in (("gpu", eng), ("host", None)):
            ts = []
            for i in range(reps + 1):
                t0 = time.perf_counter()
                kept = gdb.create_reduced_point_cloud(e, infos, frames, os.path.join(td, name))
                if i:
                    ts.append(time.perf_counter() - t0)
            out[f"{name}_frames_per_s"] = round(len(frames) / med(ts), 1)
            out[f"{name}_kept"] = int(kept.sum())
    eng.close()
    assert out["gpu_kept"] == out["host_kept"]
    out["gpu_over_host"] = round(out["gpu_frames_per_s"] / out["host_frames_per_s"], 2)
    return out


def detect_leg(frame, reps):
    rect, trv2c, p2 = calib()
    eng = pp.Engine(pp.config.kitti_shaped_config(1), max_batch=1, max_points_per_frame=NMAX)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    R, T = rect[None], trv2c[None]

    def raw():
        return eng.detect([frame], R, T)

    def gpu_crop():
        return eng.detect([frame], R, T, p2=p2, image_shape=IMAGE)

    def host_crop():
        return eng.detect([pp.frustum.remove_outside_points_np(frame, rect, trv2c, p2, IMAGE)], R, T)

    out = {}
    want = host_crop()
    for name, fn in (("raw_ms", raw), ("gpu_crop_ms", gpu_crop), ("host_crop_ms", host_crop)):
        for _ in range(3):
            got = fn()
        if name != "raw_ms":
            assert np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes(), name
        ts = []
        for _ in range(max(reps, 20)):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        out[name] = round(med(ts) * 1e3, 4)
    out["host_over_gpu"] = round(out["host_crop_ms"] / out["gpu_crop_ms"], 2)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    reps = max(args.reps, 5)
    rect, trv2c, p2 = calib()
    frames = [sweep(i) for i in range(32)]
    plane = pp.frustum.frustum_planes(rect, trv2c, p2, IMAGE)
    infos = [{"velodyne_path": f"velodyne/{i:06d}.bin", "img_shape": np.array(IMAGE), "calib/R0_rect": rect,
              "calib/Tr_velo_to_cam": trv2c, "calib/P2": p2} for i in range(32)]
    res = {"reps": reps, "frame": f"{N_POINTS} points x 4, full sweep", "spread": "min / max over the repetitions of one run",
           "kernels_b1": kernel_leg(frames[:1], plane[None], reps),
           "kernels_b32": kernel_leg(frames, np.stack([plane] * 32), reps),
           "reduce": reduce_leg(frames, infos, reps), "detect_b1": detect_leg(frames[0], reps)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
