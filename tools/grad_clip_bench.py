"""What gradient clipping costs (csrc/grad_clip.hip, optim.GradClip) on cfg-A, one JSON line per batch size:

  step     ms per optimizer step (forward + loss + backward + AdamW, graph replays, host clock around steps that end in
           a device synchronisation) with clipping off, in monitor mode, and in "global_norm", "norm" and "value",
           alternating on ONE trainer and one staged batch; off is the step as it was before clipping existed (the
           same calls: compare it with this tool's `--modes off` run on the commit before)
  reduce   the reduction alone (pp_grad_norm_device: the partial-sum launch and the finishing launch, back to back on
           one stream, an event pair around `--kernel-reps` calls) for one group and for one group per tensor, against
           the time a copy-rate read of the trainable gradients would take (4 bytes per parameter)

    python tools/grad_clip_bench.py [--batches 2,32,64] [--steps 40] [--warmup 10] [--rounds 3] [--modes off,monitor,...]"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pp_amd as pp  # noqa: E402

MODES = ["off", "monitor", "global_norm", "norm", "value"]
ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="2,32,64")
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--kernel-reps", type=int, default=200)
ap.add_argument("--modes", default=",".join(MODES))
args = ap.parse_args()
modes = args.modes.split(",")
assert all(m in MODES for m in modes), modes


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


def reduce_us(tr, per_tensor, reps):
    """pp_grad_norm_device alone on the trainer's gradient buffer: us per call (two launches), and the norm."""
    import torch
    from pp_amd import optim, trainer
    L = pp._lib.lib()
    n = tr.grads.numel()
    if per_tensor:
        segs, _ = trainer.trainable_tensor_segments(tr.layout, tr.frozen)
        groups = np.arange(len(segs), dtype=np.int32)
    else:
        segs, groups = trainer.trainable_segments(tr.layout, tr.frozen), None
    seg = np.ascontiguousarray(segs, np.int64).reshape(-1, 2)
    G = len(seg) if per_tensor else 1
    nbytes = ctypes.c_int64(0)
    assert L.pp_grad_clip_workspace_bytes(n, len(seg), G, ctypes.byref(nbytes)) == 0
    ws = torch.zeros(nbytes.value // 4, dtype=torch.int32, device=tr.device)

    def call():
        st = L.pp_grad_norm_device(tr.device.index or 0, None, ctypes.c_void_p(tr.grads.data_ptr()), n,
                                   seg.ctypes.data_as(ctypes.c_void_p), len(seg),
                                   groups.ctypes.data_as(ctypes.c_void_p) if per_tensor else None, G,
                                   ctypes.c_void_p(ws.data_ptr()))
        assert st == 0, L.pp_last_error(None)
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    best = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) / reps * 1e3)
    stats = optim.AdamW.decode_stats(ws[:4 + 2 * G].cpu().numpy())
    return {"segments": len(seg), "groups": G, "us_per_call": [round(x, 2) for x in best], "norm": stats["global_norm"]}


for B in [int(b) for b in args.batches.split(",")]:
    cfg, d, frames, labels, reg = problem(B)
    w = pp.weights.init_weights(d, seed=7)
    tr = pp.Trainer(cfg, w, max_batch=B, max_points_per_frame=16384, learning_rate=1e-6, weight_decay=1e-4)
    st = tr.stage(frames, labels, reg)
    clips = {"off": None}
    if modes != ["off"]:
        GradClip = pp.optim.GradClip
        tr.set_grad_clip(GradClip())
        tr.step(st)
        norm = tr.grad_stats()["global_norm"]          # the clipping modes clip: c is half the norm measured here
        clips.update(monitor=GradClip(), global_norm=GradClip("global_norm", 0.5 * norm),
                     norm=GradClip("norm", 0.5 * norm / 9), value=GradClip("value", 1e-4))
    ms = {m: [] for m in modes}

    def switch(m):
        if modes != ["off"]:
            tr.set_grad_clip(clips[m])
    for m in modes:                                      # graphs captured and everything warm before anything is timed
        switch(m)
        timed_steps(tr, st, args.warmup)
    for _ in range(args.rounds):
        for m in modes:
            switch(m)
            timed_steps(tr, st, 2)
            ms[m].append(round(timed_steps(tr, st, args.steps), 4))
    best = {k: min(v) for k, v in ms.items()}
    line = {"config": "cfg-A", "batch": B, "n_params": int(tr.params.numel()), "ms_per_step": ms, "best_ms": best,
            "spread_ms": {k: round(max(v) - min(v), 4) for k, v in ms.items()}}
    if "off" in best:
        line["added_us_per_step"] = {k: round((v - best["off"]) * 1e3, 1) for k, v in best.items() if k != "off"}
    if modes != ["off"]:
        nbytes = 4 * int(tr.params.numel())
        rate = tr.engine.device_copy_GBps()              # read + written bytes per second of a device copy
        line.update(reduce_one_group=reduce_us(tr, False, args.kernel_reps),
                    reduce_per_tensor=reduce_us(tr, True, args.kernel_reps),
                    bytes_read=nbytes, copy_rate_GBps=round(rate, 1),
                    copy_rate_read_us=round(nbytes / (rate * 1e9) * 1e6, 2))
    st.close()
    tr.close()
    print(json.dumps(line), flush=True)
