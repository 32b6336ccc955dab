"""Kernel-tuning aid: per-layer launch time of the RPN GEMM kernels.

    python tools/layer_bench.py [--batch 64] [--layers 5,7] [--config A|K]
The kernel of each layer is the one the pass launches; the runtime switches of INTEGRATION.md section 5 pick another,
e.g. PP_SEP_KERNEL=ws (producer/consumer separable kernel), PP_GEMM_PREC=f32 (float32 MFMA instantiations),
PP_SEP_K4=0 / PP_DECONV_K4=0 (no split-K small-map kernels).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pp_amd as pp  # noqa: E402
from bench import layer_flops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--layers", default="")
ap.add_argument("--config", default="A")
args = ap.parse_args()
B = args.batch
cfg = pp.config.pedestrian_d435i_config(B) if args.config == "A" else pp.config.kitti_shaped_config(B)
eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=20000)
eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
frames = [pp.synth.d435i_cloud(i) if args.config == "A" else pp.synth.kitti_cloud(i) for i in range(B)]
eng.detect(frames)   # fill the activation buffers with real data
tags = eng.layer_tags()
lf = layer_flops(eng.d, B, heads_fused=not any(t.endswith(':heads') for t in tags))
sel = [int(v) for v in args.layers.split(",")] if args.layers else range(len(tags))
tot = 0.0
for i in sel:
    name = tags[i].split(":")[1]
    ms = eng.bench_layer(i, B, reps=20)
    tot += ms
    print(f"{i:2d} {tags[i]:34s}  {ms * 1e3:7.1f} us ({lf[name] / (ms * 1e-3) / 1e12:5.1f} TF)")
print("total", round(tot, 4))
