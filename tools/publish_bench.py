"""Trainer weights into the detector: the host route against the device publish (csrc/weight_publish.hip), one JSON
line per configuration (cfg-A, cfg-K), host clock around calls that end in a device synchronisation:

  host_route   Trainer.weights() (two device-to-host copies + unflatten) + Engine.load_weights() (82 pp_set_weight, fold /
               split / upload in pp_finalize_weights, graphs dropped) + the first detect behind it (re-captures its graph)
  publish      Trainer.publish() wall time (two launches + the read-back of the range flags), the two kernels' own times
               (each launch's start / stop events) and the detect behind it (replays the graph it had)

Both routes run on the trainer's own engine, alternating, after a warm-up of each; min and median over --reps.

    python tools/publish_bench.py [--reps 7] [--batch 1]"""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--batch", type=int, default=1)
args = ap.parse_args()
B = args.batch

CONFIGS = {
    "cfg-A": (pp.config.pedestrian_d435i_config(B), lambda i: pp.synth.d435i_cloud(500 + i, 16384)),
    "cfg-K": (pp.config.kitti_shaped_config(B), lambda i: pp.synth.kitti_cloud(500 + i, 20000)),
}


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3)}


for name, (cfg, cloud) in CONFIGS.items():
    d = pp.config.Derived(cfg)
    frames = [cloud(i) for i in range(B)]
    tr = pp.Trainer(cfg, pp.weights.init_weights(d, seed=7), max_batch=B, max_points_per_frame=32768)
    eng = tr.engine
    t = {k: [] for k in ("weights", "load_weights", "first_detect", "publish", "detect_after_publish")}
    k_us = {}
    want = None
    for rep in range(args.reps + 1):              # rep 0 warms both routes up
        a, w = clock(tr.weights)
        b, _ = clock(lambda: eng.load_weights(w))
        c, host = clock(lambda: eng.detect(frames))
        tr._dirty = True                          # the weights have not moved; publish them anyway
        p, _ = clock(tr.publish)                  # (the publish behind a host load allocates: not timed, see below)
        eng.detect(frames)
        tr._dirty = True
        p, _ = clock(tr.publish)                  # in place
        q, got = clock(lambda: eng.detect(frames))
        assert np.array_equal(host[1], got[1]) and all(
            host[0][i, :n].tobytes() == got[0][i, :n].tobytes() for i, n in enumerate(got[1])), "routes disagree"
        if rep:
            for k, v in zip(t, (a, b, c, p, q)):
                t[k].append(v)
    eng.set_profiling(True)
    for _ in range(args.reps):
        tr._dirty = True
        tr.publish()
        for kn, ms in eng.kernel_times():
            k_us.setdefault(kn.split(":")[0], []).append(ms * 1e3)
    eng.set_profiling(False)
    info = eng.publish_info()
    n_params, n_state = tr.params.numel(), tr.state.numel()
    tr.close()
    host_total = [x + y + z for x, y, z in zip(t["weights"], t["load_weights"], t["first_detect"])]
    pub_total = [x + y for x, y in zip(t["publish"], t["detect_after_publish"])]
    print(json.dumps({
        "config": name, "batch": B, "param_floats": n_params, "state_floats": n_state,
        "host_route_ms": {k: summary(t[k]) for k in ("weights", "load_weights", "first_detect")} | {"total": summary(host_total)},
        "publish_ms": {"publish_wall": summary(t["publish"]), "detect": summary(t["detect_after_publish"]),
                       "total": summary(pub_total)},
        "publish_kernels_us": {k: summary(v) for k, v in k_us.items()},
        "publish_info": info,
    }), flush=True)
