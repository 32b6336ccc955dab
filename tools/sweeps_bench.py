"""The multi-sweep accumulation stage on the GPU (csrc/sweeps.hip); prints one JSON line.

cfg-A (3 point features), synth.d435i_cloud frames of 16384 points, history 4, capacity 16384, no decimation,
max_points_per_frame = 5 x 16384 so that nothing is cut; batch 1 and batch 64, every ring full (the timed calls each
carry 4 stored sweeps per stream).

  kernels  k_sweep_plan + k_sweep_move by HIP events (the per-launch events of pp_set_profiling), median of the
           repetitions, min / max beside it; achieved byte rate = the bytes the rule needs / that time -- per call the
           current rows are read once and written twice (output, ring), the history rows read once and written once:
           (3 + 2 x history) x rows x 12 bytes -- beside Engine.device_copy_GBps of the same process (the second read of
           the current rows, for the ring push, may hit the last-level cache: the rate is what the launches achieve, not
           an HBM measurement)
  call     the synchronous accumulate_sweeps by the host clock (upload excluded), median
  pass_b1  batch 1, host clock, median: Engine.detect on the single sweep -- the pass as the parent commit runs it --
           against Engine.detect(poses=, stamps=) (upload + accumulate + a pass over five sweeps' points); the stage's
           own share is the `call` figure

    python tools/sweeps_bench.py [--reps 20]
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

KERNELS = ("k_sweep_plan", "k_sweep_move")
N, HISTORY = 16384, 4
NMAX = N * (HISTORY + 1)


def med(xs):
    return float(np.median(xs))


def poses_at(i, B):
    return np.stack([pp.sweeps.pose_from_xyyaw(0.05 * i, 0.01 * b, 0.002 * i) for b in range(B)])


def engine(B, weights=False):
    eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=NMAX)
    if weights:
        eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    eng.set_sweeps({"history": HISTORY, "capacity": N, "max_age": 10.0})
    return eng


def kernel_leg(B, reps):
    frames = [pp.synth.d435i_cloud(i % 8) for i in range(B)]
    eng = engine(B)
    step = [0]

    def call():
        i = step[0]
        step[0] += 1
        eng.upload(frames)
        t0 = time.perf_counter()
        counts = eng.accumulate_sweeps(poses_at(i, B), np.full(B, 0.1 * i))
        return counts, time.perf_counter() - t0

    for _ in range(HISTORY + 2):                    # fills every ring and warms the launches up
        counts, _ = call()
    assert counts.tolist() == [NMAX] * B and int(eng.sweeps_info()["truncated"].sum()) == 0
    wall = [call()[1] for _ in range(reps)]
    eng.set_profiling(True)
    per = []
    for _ in range(reps):
        call()
        per.append({k: ms for k, ms in eng.kernel_times() if k in KERNELS})
    eng.set_profiling(False)
    copy = eng.device_copy_GBps()
    eng.close()
    tot = [sum(p.values()) * 1e3 for p in per]
    rows = B * N
    nbytes = (3 + 2 * HISTORY) * rows * 12
    return {"batch": B, "rows_in": rows, "rows_out": B * NMAX, "us": round(med(tot), 2),
            "us_min_max": [round(min(tot), 2), round(max(tot), 2)],
            "kernel_us": {k: round(med([p[k] for p in per]) * 1e3, 2) for k in KERNELS},
            "bytes": nbytes, "GBps": round(nbytes / (med(tot) * 1e-6) / 1e9, 1), "device_copy_GBps": round(copy, 1),
            "call_us_host_clock": round(med(wall) * 1e6, 1)}


def pass_leg(reps):
    frame = [pp.synth.d435i_cloud(3)]
    eng = engine(1, weights=True)
    step = [0]

    def single():
        return eng.detect(frame)

    def accumulated():
        i = step[0]
        step[0] += 1
        return eng.detect(frame, poses=poses_at(i, 1), stamps=[0.1 * i])

    out = {}
    for name, fn in (("single_sweep_pass_ms", single), ("accumulated_pass_ms", accumulated)):
        for _ in range(HISTORY + 2):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        out[name] = round(med(ts) * 1e3, 4)
        out[name + "_min_max"] = [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    reps = max(args.reps, 5)
    res = {"reps": reps, "frame": f"{N} points x 3, history {HISTORY}", "spread": "min / max over the repetitions of one run",
           "b1": kernel_leg(1, reps), "b64": kernel_leg(64, reps), "pass_b1": pass_leg(reps)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
