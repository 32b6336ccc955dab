"""Building the object database on the host vs on the GPU (csrc/gt_database.hip); prints one JSON line.

  gpu:   frames / s of gt_database.create_groundtruth_database through an Engine, upload included (3 x B frames, B at a
         time); the count and gather kernels alone, us per batch (from the kernel times of pp_gtdb_build)
  host:  frames / s of gt_database.build_objects_np (the float64 restatement) on frames of the same batch
  bound: the copy bound of the two passes -- the clouds' bytes read twice plus the objects' bytes written, over the
         measured device_copy_GBps -- and the gather kernel's distance from its share of it (the cloud read once plus the
         objects written)

cfg-A and cfg-K frame sizes with 8 and 64 boxes per frame, B = 32.

    python tools/gt_database_bench.py [--reps 5]
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

KERNELS = ("k_gdb_planes", "k_gdb_count", "k_gdb_chunks", "k_gdb_offsets", "k_gdb_gather")
B = 32


def frames_for(name):
    if name == "cfg-A":
        return pp.config.pedestrian_d435i_config(B), [pp.synth.d435i_cloud(3000 + i, 16384) for i in range(B)], 16384
    return pp.config.kitti_shaped_config(B), [pp.synth.kitti_cloud(3000 + i, 20000) for i in range(B)], 20000


def boxes_in(rng, cfg, n):
    r = cfg["model"]["second"]["voxel_generator"]["point_cloud_range"]
    xy = rng.uniform([r[0] + 0.5, r[1] + 0.5], [r[3] - 0.5, r[4] - 0.5], (n, 2))
    z = rng.uniform(-1.2, -0.4, (n, 1))
    wlh = np.stack([rng.uniform(0.4, 0.9, n), rng.uniform(0.5, 1.0, n), rng.uniform(1.4, 1.9, n)], 1)
    return np.concatenate([xy, z, wlh, rng.uniform(-np.pi, np.pi, (n, 1))], 1)


def as_infos(boxes):
    """Frame infos whose camera frame IS the lidar frame (identity calibration): the conversion's cost stays in."""
    infos = []
    for k, b in enumerate(boxes):
        n = len(b)
        infos.append({"image_idx": f"{k:06d}", "calib/R0_rect": np.eye(4), "calib/Tr_velo_to_cam": np.eye(4),
                      "annos": {"name": np.array(["Pedestrian"] * n), "location": b[:, :3], "dimensions": b[:, [4, 5, 3]],
                                "rotation_y": b[:, 6], "bbox": np.zeros((n, 4)), "difficulty": np.zeros(n, np.int32),
                                "index": np.arange(n, dtype=np.int32)}})
    return infos


def leg(name, G, reps, copy_gbps):
    cfg, frames, n = frames_for(name)
    F = frames[0].shape[1]
    rng = np.random.default_rng(8)
    boxes = [boxes_in(rng, cfg, G) for _ in frames]
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=n)
    eng.upload(frames)
    counts, _ = eng.build_gt_objects(boxes, return_counts=True)       # allocates the scratch; warm-up
    cut = int(sum(c.sum() for c in counts))
    eng.set_profiling(True)
    per = []
    for _ in range(reps):
        eng.upload(frames)
        eng.build_gt_objects(boxes)
        per.append({k.split(":")[0]: ms for k, ms in eng.kernel_times() if k.split(":")[0] in KERNELS})
    eng.set_profiling(False)
    med = {k: float(np.median([p[k] for p in per])) * 1e3 for k in per[-1]}
    infos = as_infos(boxes * 3)
    pp.gt_database.create_groundtruth_database(eng, infos[:B], frames, used_classes=["Pedestrian"])
    t0 = time.perf_counter()
    pp.gt_database.create_groundtruth_database(eng, infos, frames * 3, used_classes=["Pedestrian"])
    t_gpu = time.perf_counter() - t0
    eng.close()
    t0 = time.perf_counter()
    for f, b in zip(frames[:4], boxes[:4]):
        pp.gt_database.build_objects_np(f, b)
    t_np = time.perf_counter() - t0
    cloud_bytes = sum(f.nbytes for f in frames)
    obj_bytes = cut * F * 4
    bound_us = (2 * cloud_bytes + obj_bytes) / (copy_gbps * 1e9) * 1e6
    gather_bound_us = (cloud_bytes + obj_bytes) / (copy_gbps * 1e9) * 1e6
    return {"gpu_frames_per_s": 3 * B / t_gpu, "host_np_frames_per_s": 4 / t_np, "kernel_us": {k: round(v, 2) for k, v in med.items()},
            "count_plus_gather_us": med.get("k_gdb_count", 0.0) + med.get("k_gdb_gather", 0.0), "points_cut_per_batch": cut,
            "copy_bound_us": bound_us, "gather_bound_us": gather_bound_us,
            "gather_over_bound": med.get("k_gdb_gather", 0.0) / gather_bound_us if gather_bound_us else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    eng = pp.Engine(pp.config.pedestrian_d435i_config(1), max_batch=1, max_points_per_frame=1024)
    copy_gbps = float(eng.device_copy_GBps(1 << 28, 5))
    eng.close()
    res = {"device_copy_GBps": copy_gbps, "B": B}
    for name in ("cfg-A", "cfg-K"):
        for G in (8, 64):
            res[f"{name} G={G}"] = leg(name, G, args.reps, copy_gbps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
