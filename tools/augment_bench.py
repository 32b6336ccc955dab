"""Training-time augmentation on the host vs on the GPU (csrc/augment.hip); prints one JSON line.

  host:  augment.augment_np ms / frame (the float64 restatement of the reference's stages) and augment.draw ms / batch
         at cfg-A and cfg-K with 8 / 64 boxes per frame
  gpu:   augmentation us per batch (k_aug_select + k_aug_points + k_aug_compact, from the kernel times of pp_augment)
         at cfg-A B = 2 / 32 and cfg-K B = 32 with 8 / 64 boxes per frame
  train: ms per optimizer step with staged boxes, without and with augmentation (Trainer.step with stage_gt batches
         taking turns, the next one prefetched: bench.py's train_leg pattern), same shapes

    python tools/augment_bench.py [--steps 20]
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

AUG_KERNELS = ("k_aug_select", "k_aug_points", "k_aug_compact")
SHAPES = (("cfg-A", 2), ("cfg-A", 32), ("cfg-K", 32))


def frames_for(name, B):
    if name == "cfg-A":
        return pp.config.pedestrian_d435i_config(B), [pp.synth.d435i_cloud(3000 + i, 16384) for i in range(B)], 16384
    return pp.config.kitti_shaped_config(B), [pp.synth.kitti_cloud(3000 + i, 20000) for i in range(B)], 20000


def boxes_for(rng, cfg, G):
    """G boxes spread over the frame's range (half of them collide with some other box in a crowded frame)."""
    r = cfg["model"]["second"]["voxel_generator"]["point_cloud_range"]
    xy = rng.uniform([r[0], r[1]], [r[3], r[4]], (G, 2))
    z = rng.uniform(-1.2, -0.4, (G, 1))
    wlh = np.stack([rng.uniform(0.4, 0.9, G), rng.uniform(0.5, 1.0, G), rng.uniform(1.4, 1.9, G)], 1)
    return np.concatenate([xy, z, wlh, rng.uniform(-np.pi, np.pi, (G, 1))], 1).astype(np.float32)


def host_leg(name, G, n_frames=2):
    cfg, frames, _ = frames_for(name, n_frames)
    rng = np.random.default_rng(5)
    gts = [boxes_for(rng, cfg, G) for _ in frames]
    acfg = pp.augment.AugmentConfig.from_input_reader({})
    pc = np.asarray(pp.config.Derived(cfg).pc_range, np.float64)
    t0 = time.perf_counter()
    draws = pp.augment.draw(np.random.RandomState(0), gts, acfg)
    t_draw = time.perf_counter() - t0
    t0 = time.perf_counter()
    for b, f in enumerate(frames):
        pp.augment.augment_np(f, gts[b], None, None, draws.frame(b), acfg, pc)
    t_aug = time.perf_counter() - t0
    return {"augment_np_ms_per_frame": t_aug / n_frames * 1e3, "draw_ms_per_frame": t_draw / n_frames * 1e3}


def gpu_leg(name, B, G, reps=5):
    cfg, frames, n = frames_for(name, B)
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=n)
    rng = np.random.default_rng(6)
    gts = [boxes_for(rng, cfg, G) for _ in frames]
    acfg = pp.augment.AugmentConfig.from_input_reader({})
    draws = pp.augment.draw(np.random.RandomState(1), gts, acfg)
    eng.upload(frames)
    eng.augment(gts, draws=draws, aug_config=acfg)           # allocates the scratch; warm-up
    eng.set_profiling(True)
    per, wall = [], []
    for _ in range(reps):
        eng.upload(frames)
        t0 = time.perf_counter()
        eng.augment(gts, draws=draws, aug_config=acfg)
        wall.append(time.perf_counter() - t0)
        per.append({k: ms for k, ms in eng.kernel_times() if k.split(":")[0] in AUG_KERNELS})
    eng.set_profiling(False)
    eng.close()
    med = {k: float(np.median([p[k] for p in per])) * 1e3 for k in per[-1]}
    return {"us_per_batch": sum(med.values()), "kernel_us": {k: round(v, 2) for k, v in med.items()},
            "call_ms_median": float(np.median(wall)) * 1e3}


def train_leg(name, B, G, steps):
    cfg, frames, n = frames_for(name, B)
    w = pp.weights.init_weights(pp.config.Derived(cfg), seed=7)
    rng = np.random.default_rng(7)
    gts = [boxes_for(rng, cfg, G) for _ in frames]
    out = {}
    for kind, aug in (("plain", None), ("augmented", True)):
        tr = pp.Trainer(cfg, w, max_batch=B, max_points_per_frame=n, learning_rate=2e-4, weight_decay=1e-4,
                        augment=aug, seed=3)
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
    out["ratio"] = out["augmented_ms_per_step"] / out["plain_ms_per_step"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    res = {"host": {}, "gpu": {}, "train": {}}
    for name in ("cfg-A", "cfg-K"):
        for G in (8, 64):
            res["host"][f"{name} G={G}"] = host_leg(name, G)
    for name, B in SHAPES:
        for G in (8, 64):
            res["gpu"][f"{name} B={B} G={G}"] = gpu_leg(name, B, G)
    for name, B in SHAPES:
        for G in (8, 64):
            res["train"][f"{name} B={B} G={G}"] = train_leg(name, B, G, args.steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
