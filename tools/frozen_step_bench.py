"""Training step with and without the reference's freeze (Trainer(frozen="reference"), the reference's
set_trainable(net, False)) on cfg-A: ms per optimizer step (forward + loss + backward + AdamW, graph replays, host
clock around steps that end in a device synchronisation) and launches per step (one profiled eager step).

    python tools/frozen_step_bench.py [--batches 2,32] [--steps 50] [--warmup 10] [--rounds 2]
The two variants alternate `rounds` times per batch size on the same staged batch; one JSON line per batch size."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pp_amd as pp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="2,32")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=2)
args = ap.parse_args()


def problem(B):
    cfg = pp.config.pedestrian_d435i_config(B)
    d = pp.config.Derived(cfg)
    rng = np.random.default_rng(17)
    frames = [pp.synth.d435i_cloud(700 + i, 16384) for i in range(B)]
    labels = rng.choice([-1, 0, 0, 0, 0], size=(B, d.num_anchors)).astype(np.int32)
    labels[:, rng.choice(d.num_anchors, 40, replace=False)] = 1
    reg = (rng.normal(0, 0.4, (B, d.num_anchors, 7)) * (labels[..., None] > 0)).astype(np.float32)
    return cfg, d, frames, labels, reg


def run(B, frozen, cfg, d, frames, labels, reg):
    tr = pp.Trainer(cfg, pp.weights.init_weights(d, seed=7), max_batch=B, max_points_per_frame=16384,
                    learning_rate=1e-6, weight_decay=1e-4, frozen=frozen)
    st = tr.stage(frames, labels, reg)
    for _ in range(args.warmup):
        tr.step(st)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        tr.step(st)
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    tr.engine.set_profiling(True)
    tr.forward_backward(st)
    launches = len(tr.engine.kernel_times())
    tr.engine.set_profiling(False)
    st.close()
    tr.close()
    return ms, launches


for B in [int(b) for b in args.batches.split(",")]:
    prob = problem(B)
    res = {"unfrozen": [], "reference": []}
    launches = {}
    for _ in range(args.rounds):
        for name, frozen in (("unfrozen", None), ("reference", "reference")):
            ms, n = run(B, frozen, *prob)
            res[name].append(round(ms, 3))
            launches[name] = n
    print(json.dumps({"config": "cfg-A", "batch": B, "ms_per_step": res, "launches_per_step": launches,
                      "best_ms": {k: min(v) for k, v in res.items()}}), flush=True)
