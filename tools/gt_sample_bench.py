"""GT-database sampling on the host vs on the GPU (csrc/gt_sample.hip); prints one JSON line.

  host:  gt_sampler.sample_all_np ms / frame (the float64 restatement of the reference's sample_all) and
         draw_candidates ms / frame at cfg-A and cfg-K
  gpu:   sampling us per batch (k_gts_select + k_gts_count + k_gts_decide + k_gts_paste, from the kernel times of
         pp_gt_sample) at cfg-A B = 2 / 32 and cfg-K B = 32
  train: ms per optimizer step of an augmenting trainer with staged boxes, without and with sampling, in the same run
         (Trainer.step with stage_gt batches taking turns, the next one prefetched), same shapes

One annotated box and up to 8 sampled objects per frame, as the shipped configuration has them.

    python tools/gt_sample_bench.py [--steps 20]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pp_amd as pp  # noqa: E402

GTS_KERNELS = ("k_gts_select", "k_gts_count", "k_gts_decide", "k_gts_paste")
SHAPES = (("cfg-A", 2), ("cfg-A", 32), ("cfg-K", 32))
SPARE = 4096           # room per frame for the pasted points


def frames_for(name, B):
    if name == "cfg-A":
        return pp.config.pedestrian_d435i_config(B), [pp.synth.d435i_cloud(3000 + i, 16384) for i in range(B)], 16384
    return pp.config.kitti_shaped_config(B), [pp.synth.kitti_cloud(3000 + i, 20000) for i in range(B)], 20000


def box_in(rng, cfg, n):
    r = cfg["model"]["second"]["voxel_generator"]["point_cloud_range"]
    xy = rng.uniform([r[0] + 0.5, r[1] + 0.5], [r[3] - 0.5, r[4] - 0.5], (n, 2))
    z = rng.uniform(-1.2, -0.4, (n, 1))
    wlh = np.stack([rng.uniform(0.4, 0.9, n), rng.uniform(0.5, 1.0, n), rng.uniform(1.4, 1.9, n)], 1)
    return np.concatenate([xy, z, wlh, rng.uniform(-np.pi, np.pi, (n, 1))], 1)


def database_for(cfg, n_objects=200, seed=9):
    """Pedestrians spread over the frame's range, 30-200 points each."""
    rng = np.random.default_rng(seed)
    F = pp.config.Derived(cfg).num_point_features
    boxes = box_in(rng, cfg, n_objects)
    infos = {"Pedestrian": [{"box3d_lidar": b, "difficulty": 0, "num_points_in_gt": 50} for b in boxes]}
    points = {"Pedestrian": [rng.uniform(-0.4, 0.4, (int(rng.integers(30, 200)), F)).astype(np.float32) for _ in boxes]}
    sc = pp.gt_sampler.SamplerConfig.from_input_reader(None)
    return pp.gt_sampler.GtDatabase(infos, points, sc, np.random.RandomState(seed), random.Random(seed), F)


def host_leg(name, n_frames=4):
    cfg, frames, _ = frames_for(name, n_frames)
    db = database_for(cfg)
    rng = np.random.default_rng(5)
    gts = [box_in(rng, cfg, 1).astype(np.float32) for _ in frames]
    t0 = time.perf_counter()
    cand = pp.gt_sampler.draw_candidates(db, [np.ones(1, np.int32)] * n_frames, random.Random(0))
    t_draw = time.perf_counter() - t0
    t0 = time.perf_counter()
    for b, f in enumerate(frames):
        pp.gt_sampler.sample_all_np(f, gts[b], None, None, db, cand.cands[b], cand.counts[b])
    t_np = time.perf_counter() - t0
    return {"sample_all_np_ms_per_frame": t_np / n_frames * 1e3, "draw_ms_per_frame": t_draw / n_frames * 1e3}


def gpu_leg(name, B, reps=5):
    cfg, frames, n = frames_for(name, B)
    db = database_for(cfg)
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=n + SPARE)
    eng.load_gt_database(db)
    rng = np.random.default_rng(6)
    gts = [box_in(rng, cfg, 1).astype(np.float32) for _ in frames]
    cand = pp.gt_sampler.draw_candidates(db, [np.ones(1, np.int32)] * B, random.Random(1))
    eng.upload(frames)
    out = eng.gt_sample(gts, candidates=cand)                 # allocates the scratch; warm-up
    pasted = sum(len(o[1]) for o in out) - B
    eng.set_profiling(True)
    per, wall = [], []
    for _ in range(reps):
        eng.upload(frames)
        t0 = time.perf_counter()
        eng.gt_sample(gts, candidates=cand)
        wall.append(time.perf_counter() - t0)
        per.append({k: ms for k, ms in eng.kernel_times() if k.split(":")[0] in GTS_KERNELS})
    eng.set_profiling(False)
    eng.close()
    med = {k: float(np.median([p[k] for p in per])) * 1e3 for k in per[-1]}
    return {"us_per_batch": sum(med.values()), "kernel_us": {k: round(v, 2) for k, v in med.items()},
            "call_ms_median": float(np.median(wall)) * 1e3, "objects_pasted_per_frame": pasted / B}


def train_leg(name, B, steps):
    cfg, frames, n = frames_for(name, B)
    w = pp.weights.init_weights(pp.config.Derived(cfg), seed=7)
    rng = np.random.default_rng(7)
    gts = [box_in(rng, cfg, 1).astype(np.float32) for _ in frames]
    out = {}
    for kind in ("augmented", "sampled+augmented"):
        kw = {}
        if kind != "augmented":
            db = database_for(cfg)
            kw = {"gt_database": db, "sampler": db.config}
        tr = pp.Trainer(cfg, w, max_batch=B, max_points_per_frame=n + SPARE, learning_rate=2e-4, weight_decay=1e-4,
                        augment=True, seed=3, **kw)
        staged = [tr.stage_gt(frames, gts), tr.stage_gt(frames[::-1], gts[::-1])]
        for i in range(4):
            tr.step(staged[i % 2], prefetch=staged[(i + 1) % 2])
        t0 = time.perf_counter()
        for i in range(steps):
            tr.step(staged[i % 2], prefetch=staged[(i + 1) % 2])
        out[f"{kind}_ms_per_step"] = (time.perf_counter() - t0) / steps * 1e3
        tr._prefetched = None
        tr.engine.sync()
        for s in staged:
            s.close()
        tr.close()
    out["ratio"] = out["sampled+augmented_ms_per_step"] / out["augmented_ms_per_step"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    res = {"host": {}, "gpu": {}, "train": {}}
    for name in ("cfg-A", "cfg-K"):
        res["host"][name] = host_leg(name)
    for name, B in SHAPES:
        res["gpu"][f"{name} B={B}"] = gpu_leg(name, B)
    for name, B in SHAPES:
        res["train"][f"{name} B={B}"] = train_leg(name, B, args.steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
