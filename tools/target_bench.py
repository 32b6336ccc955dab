"""Training targets on the host vs on the GPU (csrc/targets.hip); prints one JSON line.

  host:  target_assigner.assign ms / frame, and the whole host pipeline (engine voxeliser -> anchor mask -> assign)
  gpu:   assignment us per batch (anchor mask + reset + the two passes, from the kernel times of pp_assign_targets)
         at cfg-A B = 2 / 32 and cfg-K B = 32 with 4 / 16 / 64 boxes per frame
  train: cfg-A B = 2 / 32 ms per optimizer step, staged dense labels vs staged boxes, with bench.py's train_leg pattern
         (two staged batches taking turns, the next one prefetched)

    python tools/target_bench.py [--steps 20]
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

CFG_TA = {"sample_positive_fraction": "None", "rpn_batch_size": 512}
TGT_KERNELS = ("k_anchor_mask_frame", "k_occ_rowscan", "k_colscan", "k_anchor_lookup", "memset", "k_tgt_top",
               "k_tgt_assign")


def boxes_for(rng, frame, G, sizes=(0.6, 0.8, 1.73)):
    """G boxes, half of them centred on points of the cloud."""
    c = frame[rng.choice(len(frame), G, replace=False), :3].astype(np.float64)
    far = rng.uniform(c.min(0), c.max(0), c.shape)
    c[G // 2:] = far[G // 2:]
    wlh = np.stack([rng.uniform(0.5, 1.1, G) * s for s in sizes], axis=1)
    r = rng.uniform(-np.pi, np.pi, (G, 1))
    return np.concatenate([c, wlh, r], axis=1).astype(np.float32)


def frames_for(name, B):
    if name == "cfg-A":
        return pp.config.pedestrian_d435i_config(B), [pp.synth.d435i_cloud(3000 + i, 16384) for i in range(B)]
    return pp.config.kitti_shaped_config(B), [pp.synth.kitti_cloud(3000 + i, 20000) for i in range(B)]


def host_leg(name, G, n_frames=4):
    cfg, frames = frames_for(name, n_frames)
    eng = pp.Engine(cfg, max_batch=1, max_points_per_frame=20000)
    rng = np.random.default_rng(5)
    gts = [boxes_for(rng, f, G) for f in frames]
    cls = np.ones(G, np.int32)
    masks, t_assign = [], 0.0
    t0 = time.perf_counter()
    for f, g in zip(frames, gts):
        _, coors, _ = eng.points_to_voxel(f)
        coors4 = np.concatenate([np.zeros((len(coors), 1), np.int32), coors], axis=1)
        m = eng.anchor_mask(coors4, 1)[0].astype(bool)
        masks.append(m)
        t1 = time.perf_counter()
        pp.target_assigner.assign(eng.anchors, g, m, cls, 0.5, 0.35, CFG_TA)
        t_assign += time.perf_counter() - t1
    total = time.perf_counter() - t0
    eng.close()
    return {"assign_ms_per_frame": t_assign / n_frames * 1e3, "pipeline_ms_per_frame": total / n_frames * 1e3}


def gpu_leg(name, B, G, reps=5):
    cfg, frames = frames_for(name, B)
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=20000)
    rng = np.random.default_rng(6)
    gts = [boxes_for(rng, f, G) for f in frames]
    eng.upload(frames)
    eng.assign_targets(gts)                   # voxelises the resident frames once; warm-up
    eng.set_profiling(True)
    per, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.assign_targets(gts)
        wall.append(time.perf_counter() - t0)
        kt = eng.kernel_times()
        per.append({n: ms for n, ms in kt if n.split(":")[0] in TGT_KERNELS})
    eng.set_profiling(False)
    eng.close()
    med = {k: float(np.median([p[k] for p in per])) * 1e3 for k in per[-1]}
    return {"us_per_batch": sum(med.values()), "kernel_us": {k: round(v, 2) for k, v in med.items()},
            "call_ms_median": float(np.median(wall)) * 1e3}


def train_leg(B, steps, G=16):
    cfg, frames = frames_for("cfg-A", B)
    d = pp.config.Derived(cfg)
    tr = pp.Trainer(cfg, pp.weights.init_weights(d, seed=7), max_batch=B, max_points_per_frame=16384,
                    learning_rate=2e-4, weight_decay=1e-4)
    rng = np.random.default_rng(7)
    gts = [boxes_for(rng, f, G) for f in frames]
    tr.engine.upload(frames)
    res = tr.engine.assign_targets(gts)
    labels = np.stack([r["labels"] for r in res])
    reg = np.stack([r["bbox_targets"] for r in res])
    out = {}
    for kind in ("labels", "boxes"):
        if kind == "labels":
            staged = [tr.stage(frames, labels, reg), tr.stage(frames[::-1], labels[::-1], reg[::-1])]
        else:
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    res = {"host": {}, "gpu": {}, "train": {}}
    for name in ("cfg-A", "cfg-K"):
        for G in (4, 16):
            res["host"][f"{name} G={G}"] = host_leg(name, G)
    for name, B in (("cfg-A", 2), ("cfg-A", 32), ("cfg-K", 32)):
        for G in (4, 16, 64):
            res["gpu"][f"{name} B={B} G={G}"] = gpu_leg(name, B, G)
    for B in (2, 32):
        res["train"][f"cfg-A B={B}"] = train_leg(B, args.steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
