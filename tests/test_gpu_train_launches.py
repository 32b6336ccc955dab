"""The training step's launch sequence: the ordered Engine.kernel_times() names of one profiled (eager) step, name for
name against tests/golden/train_launches.json, recorded on the MI355X.  Every kernel choice of the host side -- fused
or split forward, fused or product heads, one- or two-pass depthwise backward, paired gradient products, split-K and
deferred reductions, the BatchNorm finalize width -- shows in the names, so a host change that alters any of them
fails here.  The switches are read once per process: their cases run in a child process each."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "train_launches.json")

# case -> (config, batch, targets, switches of its child process)
CASES = {
    "A2": ("A", 2, "dense", None),
    "A32": ("A", 32, "dense", None),
    "A2-gt": ("A", 2, "gt", None),
    "A2-augment": ("A", 2, "augment", None),
    "K32": ("K", 32, "dense", None),
    "A2-fused-min-0": ("A", 2, "dense", {"PP_TRAIN_FUSED_MIN": "0"}),
    "A2-gemm-f32": ("A", 2, "dense", {"PP_TRAIN_GEMM": "f32"}),
    "A2-arena-4096": ("A", 2, "dense", {"PP_TRAIN_ARENA_FLOATS": "4096"}),
}


def launch_names(pp, case):
    """The ordered launch names of one profiled training step of `case` (this process's switches)."""
    kind, B, targets, _ = CASES[case]
    rng = np.random.default_rng(17)
    if kind == "A":
        cfg = pp.config.pedestrian_d435i_config(B)
        frames = [pp.synth.d435i_cloud(700 + i, 6000) for i in range(B)]
    else:
        cfg = pp.config.kitti_shaped_config(B)
        frames = [pp.synth.kitti_cloud(700 + i, 5000) for i in range(B)]
    d = pp.config.Derived(cfg)
    tr = pp.Trainer(cfg, pp.weights.init_weights(d, seed=7), max_batch=B, max_points_per_frame=8192,
                    learning_rate=2e-4, weight_decay=1e-4, augment=(targets == "augment"), seed=11)
    tr.engine.set_profiling(True)
    if targets == "dense":
        A = d.num_anchors
        labels = rng.choice([-1, 0, 0, 0, 0], size=(B, A)).astype(np.int32)
        labels[:, rng.choice(A, 40, replace=False)] = 1
        reg = (rng.normal(0, 0.4, (B, A, 7)) * (labels[..., None] > 0)).astype(np.float32)
        tr.forward_backward(frames, labels, reg)
    else:
        G = 4
        gts = [np.concatenate([rng.uniform(1.0, 5.5, (G, 1)), rng.uniform(-1.5, 1.5, (G, 1)), np.full((G, 1), -0.9),
                               np.full((G, 1), 0.6), np.full((G, 1), 0.8), np.full((G, 1), 1.73),
                               rng.uniform(-np.pi, np.pi, (G, 1))], 1).astype(np.float32) for _ in range(B)]
        tr.forward_backward(frames, gt_boxes=gts)
    names = [n for n, _ in tr.engine.kernel_times()]
    tr.close()
    return names


_CHILD = """
import json, sys
sys.path.insert(0, "tests")
import pp_amd as pp
import test_gpu_train_launches as t
print("RESULT " + json.dumps(t.launch_names(pp, sys.argv[1])))
"""


def case_names(pp, case):
    env = CASES[case][3]
    if env is None:
        return launch_names(pp, case)
    r = subprocess.run([sys.executable, "-c", _CHILD, case], cwd=ROOT, env={**os.environ, **env}, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[len("RESULT "):])


@pytest.mark.parametrize("case", list(CASES))
def test_training_launch_sequence_as_recorded(pp, hip_lib, case):
    with open(GOLDEN) as fh:
        want = json.load(fh)[case]
    got = case_names(pp, case)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (case, i, g, w)
    assert len(got) == len(want), (case, len(got), len(want))
