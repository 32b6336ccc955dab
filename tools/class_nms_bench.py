"""Times of the post-process alone, joint against per-class suppression:

    python tools/class_nms_bench.py [--reps 30]

Fixed head maps (distinct class logits per class, box codes 0.3 * randn, half of the anchors on) go through
Engine.predict with per-kernel profiling on; the times are the kernels' own start / stop events
(Engine.kernel_times()), not the call's wall time.  cfg-A (80 x 64 grid, 10 240 anchors) and cfg-K (KITTI-shaped,
107 136 anchors), two classes each, at B = 1 and 32; per case the modes joint, per_class, joint again.  Per row the
median, minimum and maximum over --reps calls of k_postprocess and, in per-class mode, k_gather_classes.
On a tree without the mode (the parent commit) only the joint rows are printed, twice: the run-to-run spread the claim
"the joint mode is not slower" is judged against.  Prints one JSON line per row.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pp_amd as pp  # noqa: E402


def head_maps(d, B, seed):
    rng = np.random.default_rng(seed)
    A, napl, ncls = d.num_anchors, d.num_anchor_per_loc, d.num_class
    logits = np.stack([np.stack([rng.permutation(np.linspace(-4, 4, A)) + 1e-4 * c for c in range(ncls)], axis=-1)
                       for _ in range(B)]).astype(np.float32)
    box = (0.3 * rng.standard_normal((B, d.head_h, d.head_w, napl * 7))).astype(np.float32)
    dr = rng.standard_normal((B, d.head_h, d.head_w, napl * 2)).astype(np.float32)
    mask = (rng.random((B, A)) < 0.5).astype(np.uint8)
    return box, logits.reshape(B, d.head_h, d.head_w, napl * ncls), dr, mask


def kernel_us(eng, args, reps):
    eng.set_profiling(False)
    for _ in range(3):
        _, n = eng.predict(*args)
    eng.set_profiling(True)
    out = {}
    for _ in range(reps):
        eng.predict(*args)
        seen = {}
        for tag, ms in eng.kernel_times():
            if tag in ("k_postprocess", "k_gather_classes"):
                seen[tag] = seen.get(tag, 0.0) + ms * 1e3
        for tag, us in seen.items():
            out.setdefault(tag, []).append(us)
    eng.set_profiling(False)
    return out, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    cases = (("cfg-A", pp.config.pedestrian_d435i_config), ("cfg-K", pp.config.kitti_shaped_config))
    for name, make in cases:
        for B in (1, 32):
            cfg = make(B)
            cfg["model"]["second"]["num_class"] = 2
            eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=4096)
            rect, trv, _ = pp.synth.default_calib()
            args = head_maps(eng.d, B, 11) + (np.stack([rect] * B), np.stack([trv] * B))
            has = hasattr(eng, "set_class_nms")
            for mode in (("joint", "per_class", "joint") if has else ("joint", "joint")):
                if has:
                    eng.set_class_nms(mode)
                us, n = kernel_us(eng, args, a.reps)
                row = {"config": name, "batch": B, "num_class": 2, "class_nms": mode, "reps": a.reps,
                       "kept_mean": round(float(np.mean(n)), 2)}
                for tag, v in us.items():
                    v = np.array(v)
                    row[tag] = {"median_us": round(float(np.median(v)), 2), "min_us": round(float(v.min()), 2),
                                "max_us": round(float(v.max()), 2)}
                print(json.dumps(row), flush=True)
            eng.close()


if __name__ == "__main__":
    main()
