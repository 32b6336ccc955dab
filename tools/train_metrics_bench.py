"""What the training metrics cost (csrc/metrics.hip, pp_set_train_metrics) on cfg-A, one JSON line per batch size:

  step     ms per optimizer step (forward + loss + backward + AdamW, graph replays, host clock around steps that end in
           a device synchronisation) with the switch off and on, alternating on ONE trainer and one staged batch; off
           is the step as it was before the switch existed
  kernel   the two launches alone (each kernel's own start / stop events, pp_head_metrics on the resident head map) against the time
           a copy-rate read of the bytes they touch would take: B * H'W' * 128 B of head map + B * A * 4 B of labels
  host     the alternative without the kernel: the class map out of fetch_intermediates, then numpy (head_metrics_np)

    python tools/train_metrics_bench.py [--batches 2,32,64] [--steps 40] [--warmup 10] [--rounds 3]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pp_amd as pp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="2,32,64")
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--kernel-reps", type=int, default=30)
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


def timed_steps(tr, st, n):
    t0 = time.perf_counter()
    for _ in range(n):
        tr.step(st)
    return (time.perf_counter() - t0) / n * 1e3


for B in [int(b) for b in args.batches.split(",")]:
    cfg, d, frames, labels, reg = problem(B)
    w = pp.weights.init_weights(d, seed=7)
    tr = pp.Trainer(cfg, w, max_batch=B, max_points_per_frame=16384, learning_rate=1e-6, weight_decay=1e-4)
    st = tr.stage(frames, labels, reg)
    eng = tr.engine
    ms = {"off": [], "on": []}
    for on in (False, True):                 # both graphs captured and warm before anything is timed
        eng.set_train_metrics(on)
        timed_steps(tr, st, args.warmup)
    for _ in range(args.rounds):
        for name, on in (("off", False), ("on", True)):
            eng.set_train_metrics(on)
            timed_steps(tr, st, 2)
            ms[name].append(round(timed_steps(tr, st, args.steps), 4))
    counts = eng.train_metrics_counts()
    # the launches alone, on the head map the last step left
    eng.set_profiling(True)
    k_ms = {"k_metrics_pixels": [], "k_metrics_finish": []}
    for _ in range(args.kernel_reps):
        got = eng.head_metrics(labels)["counts"]
        for n, t in eng.kernel_times():
            k_ms[n.split(":")[0]].append(t)
    eng.set_profiling(False)
    assert np.array_equal(got, counts)
    nbytes = B * d.head_h * d.head_w * 128 + B * d.num_anchors * 4
    rate = eng.device_copy_GBps()            # read + written bytes per second of a device copy
    st.close()
    tr.close()
    # the host alternative, on an inference pass's head map
    e2 = pp.Engine(cfg, max_batch=B, max_points_per_frame=16384, weights=w)
    rect, trv, _ = pp.synth.default_calib()
    e2.detect(frames, np.stack([rect] * B), np.stack([trv] * B))
    fetch_ms, np_ms = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        cls = e2.intermediates()["cls_preds"]
        t1 = time.perf_counter()
        pp.metrics.head_metrics_np(labels, cls.reshape(B, d.num_anchors, d.num_class))
        t2 = time.perf_counter()
        fetch_ms.append((t1 - t0) * 1e3)
        np_ms.append((t2 - t1) * 1e3)
    e2.close()
    best = {k: min(v) for k, v in ms.items()}
    print(json.dumps({
        "config": "cfg-A", "batch": B, "ms_per_step": ms, "best_ms": best,
        "added_us_per_step": round((best["on"] - best["off"]) * 1e3, 1),
        "kernel_us": {k: {"median": round(statistics.median(v) * 1e3, 2), "min": round(min(v) * 1e3, 2)} for k, v in k_ms.items()},
        "bytes_read": nbytes, "copy_rate_GBps": round(rate, 1), "copy_rate_read_us": round(nbytes / (rate * 1e9) * 1e6, 2),
        "host_alternative_ms": {"fetch_intermediates": round(min(fetch_ms), 2), "numpy": round(min(np_ms), 2)},
    }), flush=True)
