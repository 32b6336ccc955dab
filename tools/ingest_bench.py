"""Live PointCloud2 ingest on the host vs on the GPU (csrc/ingest.hip); prints one JSON line.

One synthetic 640 x 480 message (30 % of the records carry a NaN) at point_step 20 and 32; p50 over --reps repetitions of

  a  host:    ingest.pointcloud2_to_xyz + ingest.realsense_to_lidar + Engine.detect, batch 1 (host clock; the only way
              to do this without the GPU ingest)
  b  gpu:     Engine.detect_pointcloud2, batch 1 (host clock, ends in a synchronise; the message bytes are pageable)
  b2 gpu:     the same from a page-locked MessageStaging: ingest_pointcloud2_async + detect_async + detections
  c  kernels: k_ingest_count + k_ingest_scan + k_ingest_scatter by HIP events (the per-launch events of pp_set_profiling)
              at batch 1 and batch 16, with bytes read / time against the 8 TB/s HBM peak.  Bytes read = 2 x the message
              bytes: both passes touch every cache line of the message; the second pass may find them in the 256 MB last
              level cache, so the rate is what the kernels achieve, not an HBM measurement.
  pass:       the detection pass alone on the ingested frame (HIP-event stopwatch around pp_detect_async), the figure
              the ingest kernels are compared with

    python tools/ingest_bench.py [--reps 50]
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

ING_KERNELS = ("k_ingest_count", "k_ingest_scan", "k_ingest_scatter")
HBM_PEAK_GBPS = 8000.0
NMAX = 76800            # ingest.kept_bound(640, 480, 1, 4)


def p50(xs):
    return float(np.median(xs))


def kernel_leg(msgs, reps):
    B = len(msgs)
    eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=NMAX)
    for _ in range(3):
        eng.ingest_pointcloud2(msgs)                       # allocates the staging; warm-up
    eng.set_profiling(True)
    per = []
    for _ in range(reps):
        eng.ingest_pointcloud2(msgs)
        per.append({k: ms for k, ms in eng.kernel_times() if k in ING_KERNELS})
    eng.set_profiling(False)
    eng.close()
    med = {k: p50([p[k] for p in per]) * 1e3 for k in ING_KERNELS}
    total_us = p50([sum(p.values()) for p in per]) * 1e3
    nbytes = 2 * sum(m[2] * m[4] for m in msgs)
    gbps = nbytes / (total_us * 1e-6) / 1e9
    return {"batch": B, "us": round(total_us, 2), "kernel_us": {k: round(v, 2) for k, v in med.items()},
            "bytes_read": nbytes, "GBps": round(gbps, 1), "share_of_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4)}


def frame_leg(msg, reps):
    eng = pp.Engine(pp.config.pedestrian_d435i_config(1), max_batch=1, max_points_per_frame=NMAX)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    ing = pp.ingest

    def host():
        return eng.detect([ing.realsense_to_lidar(ing.pointcloud2_to_xyz(*msg))])

    def gpu():
        return eng.detect_pointcloud2([msg])

    staging = eng.staging_pointcloud2([msg])

    def gpu_pinned():
        eng.ingest_pointcloud2_async(staging)
        eng.detect_async()
        return eng.detections()

    out = {}
    want = host()
    for name, fn in (("a_host_ms", host), ("b_gpu_ms", gpu), ("b2_gpu_pinned_ms", gpu_pinned)):
        for _ in range(3):
            got = fn()
        assert np.array_equal(got[1], want[1]) and got[0][0, :got[1][0]].tobytes() == want[0][0, :want[1][0]].tobytes(), name
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        out[name] = round(p50(ts) * 1e3, 4)
    # the detection pass alone, on the ingested frame
    eng.ingest_pointcloud2([msg])
    ts = []
    for i in range(reps + 3):
        eng.timer_start()
        eng.detect_async()
        t = eng.timer_stop()
        if i >= 3:
            ts.append(t)
    out["detect_pass_ms"] = round(p50(ts), 4)
    out["kept_points"] = int(eng.ingest_info()["kept"][0])
    out["finite_records"] = int(eng.ingest_info()["finite"][0])
    eng.sync()
    staging.close()
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    reps = max(args.reps, 50)
    res = {"reps": reps, "message": "640x480, 30 % NaN records"}
    for ps in (20, 32):
        msg = pp.synth.pointcloud2_message(0, 640, 480, point_step=ps)
        r = frame_leg(msg, reps)
        r["message_bytes"] = msg[2] * msg[4]
        r["kernels_b1"] = kernel_leg([msg], reps)
        r["kernels_b16"] = kernel_leg([pp.synth.pointcloud2_message(i, 640, 480, point_step=ps) for i in range(16)], reps)
        r["a_over_b"] = round(r["a_host_ms"] / r["b_gpu_ms"], 1)
        r["ingest_kernels_share_of_b"] = round(r["kernels_b1"]["us"] * 1e-3 / r["b_gpu_ms"], 4)
        r["ingest_kernels_over_detect_pass"] = round(r["kernels_b1"]["us"] * 1e-3 / r["detect_pass_ms"], 3)
        res[f"point_step_{ps}"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
