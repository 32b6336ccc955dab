"""Feeding the detector the depth image (csrc/ingest.hip: k_depth_*) vs the PointCloud2 message computed from it
(the same file: k_ingest_*); prints one JSON line.

One synthetic 640 x 480 16UC1 image with 30 % invalid pixels and the equivalent ordered messages at point_step 20 and 32
(ingest.depth_to_pointcloud2: invalid pixels NaN), all in one process on one engine; p50 over --reps repetitions of

  a   message:  Engine.detect_pointcloud2, batch 1 (host clock, ends in a synchronise; pageable bytes) -- the parent path,
                once per point_step
  b   depth:    Engine.detect_depth, batch 1 (the same clock)
  b2  depth:    the same from a page-locked DepthStaging: ingest_depth_async + detect_async + detections
  pass          the detection pass alone on the ingested frame (HIP-event stopwatch around pp_detect_async)

The legs alternate within a round, and the p50 is taken --rounds times: the minimum and maximum of the p50s are
reported, so the run-to-run spread is on the page.  Also: the bytes copied per frame by each feed, and the three depth
kernels' times at batch 1 and batch 16 from per-launch events (pp_set_profiling) beside the message kernels' times from
the same run.  The detections of all feeds are checked to be equal before anything is timed.

    python tools/depth_ingest_bench.py [--reps 50] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pp_amd as pp  # noqa: E402

DEPTH_KERNELS = ("k_depth_count", "k_depth_scan", "k_depth_scatter")
MSG_KERNELS = ("k_ingest_count", "k_ingest_scan", "k_ingest_scatter")
NMAX = 76800            # ingest.depth_kept_bound(640, 480, 1, 4)


def p50(xs):
    return float(np.median(xs))


def kernel_leg(feed, kernels, B, reps):
    """feed(eng): one synchronous ingest of B frames.  p50 of each kernel's event time, microseconds."""
    eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=NMAX)
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


def frame_legs(image, intrinsics, msgs, reps, rounds):
    eng = pp.Engine(pp.config.pedestrian_d435i_config(1), max_batch=1, max_points_per_frame=NMAX)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    staging = eng.staging_depth([image])

    def depth_pinned():
        eng.ingest_depth_async(staging, intrinsics)
        eng.detect_async()
        return eng.detections()

    legs = {f"a_message_ps{ps}_ms": (lambda m=m: eng.detect_pointcloud2([m])) for ps, m in msgs.items()}
    legs["b_depth_ms"] = lambda: eng.detect_depth([image], intrinsics)
    legs["b2_depth_pinned_ms"] = depth_pinned
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
    eng.ingest_depth([image], intrinsics)
    ts = []
    for i in range(reps + 3):
        eng.timer_start()
        eng.detect_async()
        t = eng.timer_stop()
        if i >= 3:
            ts.append(t)
    out["detect_pass_ms"] = round(p50(ts), 4)
    info = eng.ingest_info()
    out["valid_pixels"], out["kept_points"] = int(info["finite"][0]), int(info["kept"][0])
    out["detections"] = int(want[1][0])
    eng.sync()
    staging.close()
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    reps, rounds = max(args.reps, 50), max(args.rounds, 1)
    ing = pp.ingest
    image, k = pp.synth.depth_image(0, 640, 480)
    msgs = {ps: ing.depth_to_pointcloud2(image, k, ordered=True, point_step=ps) for ps in (20, 32)}
    res = {"reps": reps, "rounds": rounds, "image": "640x480 16UC1, 30 % invalid pixels",
           "bytes_copied_per_frame": {"depth": image[2] * image[3], **{f"message_ps{ps}": m[2] * m[4] for ps, m in msgs.items()}}}
    res.update(frame_legs(image, k, msgs, reps, rounds))
    for B in (1, 16):
        scenes = [pp.synth.depth_image(i, 640, 480) for i in range(B)]
        images, ks = [s[0] for s in scenes], [s[1] for s in scenes]
        res[f"depth_kernels_b{B}"] = kernel_leg(lambda e: e.ingest_depth(images, ks), DEPTH_KERNELS, B, reps)
        for ps in (20, 32):
            ms = [ing.depth_to_pointcloud2(i, kk, ordered=True, point_step=ps) for i, kk in scenes]
            res[f"message_ps{ps}_kernels_b{B}"] = kernel_leg(lambda e: e.ingest_pointcloud2(ms), MSG_KERNELS, B, reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
