"""Feeding the detector a camera rig (csrc/ingest.hip) vs ingesting every camera on the host and uploading the
concatenated points, and vs the single-camera depth ingest; prints one JSON line.

Synthetic 640 x 480 16UC1 images with 30 % invalid pixels, 1, 2 and 4 cameras per frame at batch 1 (camera 0 under the
reference mount, the others yawed by 35, -35 and 70 degrees and shifted), all in one process on one engine; p50 over
--reps repetitions of

  rig_cN     Engine.detect_rig_depth, N cameras (host clock, ends in a synchronise; pageable bytes)
  host_cN    ingest.depth_ingest_np per camera on the host, concatenate, Engine.detect: the only route to one frame
             from several cameras without the rig ingest
  single     Engine.detect_depth, one camera (what rig_c1 should sit beside)

The device legs alternate among themselves within a round, then the host legs do (a device leg timed right behind tens
of milliseconds of numpy would pay for the GPU's idling), and the p50 is taken --rounds times: the minimum and maximum
of the p50s are reported, so the run-to-run spread is on the page.  Also: the bytes copied per frame by each feed, and
the three rig kernels' times from per-launch events (pp_set_profiling) beside the single-camera kernels' times from the
same run.  The detections of rig_cN and host_cN, and of rig_c1 and single, are checked to be equal before anything is
timed.

    python tools/rig_ingest_bench.py [--reps 50] [--rounds 5]
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

CAMERAS = (1, 2, 4)
RIG_KERNELS = ("k_rig_count<depth>", "k_rig_scan<depth>", "k_rig_scatter<depth>")
DEPTH_KERNELS = ("k_depth_count", "k_depth_scan", "k_depth_scatter")
NMAX = max(CAMERAS) * 76800            # ingest.depth_kept_bound(640, 480, 1, 4) per camera

# camera axes (x right, y down, z depth) -> lidar axes (x depth, y left, z up), as a column-vector matrix
AXES = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])


def p50(xs):
    return float(np.median(xs))


def mounts():
    out = [pp.ingest.Mount.realsense()]
    for yaw, t in ((35.0, [0.0, 0.15, 1.0]), (-35.0, [0.0, -0.15, 1.0]), (70.0, [-0.05, 0.25, 1.0])):
        a = np.deg2rad(yaw)
        T = np.eye(4)
        T[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ AXES
        T[:3, 3] = t
        out.append(pp.ingest.Mount.from_matrix(T))
    return out


def same(a, b):
    return np.array_equal(a[1], b[1]) and a[0][0, :a[1][0]].tobytes() == b[0][0, :b[1][0]].tobytes()


def kernel_times(eng, feed, kernels, reps):
    for _ in range(3):
        feed()
    eng.set_profiling(True)
    per = []
    for _ in range(reps):
        feed()
        per.append({k: ms for k, ms in eng.kernel_times() if k in kernels})
    eng.set_profiling(False)
    return {"us": round(p50([sum(p.values()) for p in per]) * 1e3, 2),
            "kernel_us": {k: round(p50([p[k] for p in per]) * 1e3, 2) for k in kernels}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    reps, rounds = max(args.reps, 50), max(args.rounds, 1)
    ing = pp.ingest
    scenes = [pp.synth.depth_image(i, 640, 480) for i in range(max(CAMERAS))]
    images, k = [s[0] for s in scenes], scenes[0][1]
    all_mounts = mounts()
    rigs = {n: ing.CameraRig(all_mounts[:n], k) for n in CAMERAS}
    eng = pp.Engine(pp.config.pedestrian_d435i_config(1), max_batch=1, max_points_per_frame=NMAX)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))

    def host(n):
        frame = np.concatenate([ing.depth_ingest_np(images[c], k, **rigs[n].depth_kwargs(c))[0] for c in range(n)])
        return eng.detect([frame])

    legs = {}
    for n in CAMERAS:
        legs[f"rig_c{n}_ms"] = lambda n=n: eng.detect_rig_depth([images[:n]], rigs[n])
        legs[f"host_c{n}_ms"] = lambda n=n: host(n)
    legs["single_depth_ms"] = lambda: eng.detect_depth([images[0]], k)
    first = {}
    for name, fn in legs.items():
        for _ in range(3):
            got = fn()
        first[name] = (got[0].copy(), got[1].copy())
    for n in CAMERAS:
        assert same(first[f"rig_c{n}_ms"], first[f"host_c{n}_ms"]), n
    assert same(first["rig_c1_ms"], first["single_depth_ms"])
    p50s = {name: [] for name in legs}
    # two groups, each alternating within a round so that its legs see the same machine state: the device legs among
    # themselves, then the host legs (tens of milliseconds of numpy each, during which the GPU idles and clocks down: a
    # device leg timed right behind one would pay for that)
    groups = [[n for n in legs if not n.startswith("host")], [n for n in legs if n.startswith("host")]]
    for _ in range(rounds):
        ts = {name: [] for name in legs}
        for group in groups:
            for _ in range(reps):
                for name in group:
                    t0 = time.perf_counter()
                    legs[name]()
                    ts[name].append(time.perf_counter() - t0)
        for name in legs:
            p50s[name].append(p50(ts[name]) * 1e3)
    res = {"reps": reps, "rounds": rounds, "image": "640x480 16UC1, 30 % invalid pixels", "batch": 1}
    res.update({name: {"p50_min": round(min(v), 4), "p50_max": round(max(v), 4)} for name, v in p50s.items()})
    res["bytes_copied_per_frame"] = {}
    for n in CAMERAS:
        eng.ingest_rig_depth([images[:n]], rigs[n])
        kept = int(eng.ingest_info()["kept"][0])
        res["bytes_copied_per_frame"][f"rig_c{n}"] = sum(i[2] * i[3] for i in images[:n])
        res["bytes_copied_per_frame"][f"host_c{n}"] = 12 * kept
        res[f"kept_points_c{n}"] = kept
        res[f"detections_c{n}"] = int(first[f"rig_c{n}_ms"][1][0])
        res[f"rig_kernels_c{n}"] = kernel_times(eng, lambda n=n: eng.ingest_rig_depth([images[:n]], rigs[n]), RIG_KERNELS, reps)
    res["bytes_copied_per_frame"]["single_depth"] = images[0][2] * images[0][3]
    res["depth_kernels_c1"] = kernel_times(eng, lambda: eng.ingest_depth([images[0]], k), DEPTH_KERNELS, reps)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
