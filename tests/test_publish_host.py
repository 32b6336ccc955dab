"""Host side of detection during training: kitti_eval.eval_score, the Trainer's dirty flag (what makes publish() a
no-op), the prefetch guard of Trainer.detect, and the C-ABI surface of the publish calls.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_score_is_the_references_formula(pp):
    rng = np.random.default_rng(3)
    m3d, mbev, maos = (rng.uniform(0, 100, (2, 3, 2)) for _ in range(3))      # [class, difficulty, tier]
    want = (m3d[0][0].sum() + maos[0][0].sum() + mbev[0][0].sum()) / 18        # train.py:418, :926, verbatim
    assert pp.kitti_eval.eval_score(m3d, mbev, maos) == want
    assert pp.kitti_eval.eval_score(m3d.tolist(), mbev.tolist(), maos.tolist()) == want
    # the argument order matters (3d, bev, aos): only class 0, difficulty 0 enters
    only = np.zeros((2, 3, 2))
    only[0, 0] = [9.0, 27.0]
    assert pp.kitti_eval.eval_score(only, 0 * only, 0 * only) == 2.0
    only[1] = 50.0
    only[0, 1:] = 50.0
    assert pp.kitti_eval.eval_score(0 * only, only, 0 * only) == 2.0


class _FakeEngine:
    """Records the calls a Trainer makes; nothing touches a device."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append(name)
            return {"loss": 0.0} if name == "train_step_wait" else ("dets", "n") if name == "detect" else None
        return call

    def count(self, name):
        return self.calls.count(name)


def _host_trainer(pp):
    """A Trainer with its buffers on the CPU and a recording engine (the constructor needs a GPU; the methods under test
    do not)."""
    tr = pp.Trainer.__new__(pp.Trainer)
    tr.torch = torch
    tr.engine = _FakeEngine()
    tr.layout = [("a/kernel", 0, 4, 0), ("a/bn/moving_mean", 0, 2, 1)]
    tr.params, tr.state = torch.zeros(4), torch.zeros(2)
    tr.grads = torch.zeros(4)
    tr._prefetched = tr._boxless = tr._metrics = tr.augment = tr.sampler = tr.grad_clip = None
    tr._stats_pending = False
    tr._dirty = True
    tr._enqueue_update = lambda dist: tr.engine.calls.append("update")
    tr._engine_stream = lambda: type("S", (), {"synchronize": staticmethod(lambda: None)})()
    return tr


def test_publish_only_when_the_weights_changed(pp):
    tr = _host_trainer(pp)
    eng = tr.engine
    assert tr.publish() is True and tr.publish() is False and eng.count("publish_weights") == 1
    frames = [np.zeros((3, 3), np.float32)]
    lab, reg = np.zeros((1, 8), np.int32), np.zeros((1, 8, 7), np.float32)
    # every way the buffers move marks them: set_weights, forward_backward (moving statistics), apply_gradients, step
    steps = [lambda: tr.set_weights({"a/kernel": np.ones(4), "a/bn/moving_mean": np.ones(2)}),
             lambda: tr.forward_backward(frames, lab, reg),
             lambda: tr.apply_gradients(),
             lambda: tr.step(frames, lab, reg)]
    for k, change in enumerate(steps):
        change()
        assert tr._dirty
        assert tr.detect(frames) == ("dets", "n")           # publishes, then Engine.detect
        assert eng.count("publish_weights") == 2 + k and not tr._dirty
        tr.detect(frames, None, None, on_numeric="raise")    # unchanged weights: no second publish
        assert eng.count("publish_weights") == 2 + k
    assert eng.calls.index("publish_weights") < eng.calls.index("detect")
    assert torch.equal(tr.params, torch.ones(4))


def test_detect_refuses_a_pending_prefetch(pp):
    tr = _host_trainer(pp)
    tr._prefetched = object()
    with pytest.raises(RuntimeError, match="prefetched"):
        tr.detect([np.zeros((3, 3), np.float32)])
    assert tr.engine.calls == []                             # neither published nor uploaded
    tr._prefetched = None
    tr.detect([np.zeros((3, 3), np.float32)])
    assert tr.engine.calls == ["publish_weights", "detect"]


def test_training_voxelnet_routes_detect_through_the_trainer(pp):
    net = pp.VoxelNet(pp.config.tiny_config(1), training=True)
    with pytest.raises(RuntimeError, match="load_weights"):
        net.detect([np.zeros((3, 3), np.float32)])
    tr = _host_trainer(pp)
    net.trainer, net.engine = tr, tr.engine
    tr.engine.detect = lambda frames, *a, **kw: (np.zeros((len(frames), 1), pp.Engine.det_dtype()),
                                                 np.zeros(len(frames), np.int32))
    out = net.detect([np.zeros((3, 3), np.float32)])
    assert tr.engine.calls == ["publish_weights"] and not tr._dirty
    assert out[0]["scores"] is None and out[0]["batch_idx"] == 0


def test_cabi_declares_and_binds_the_publish_calls(pp, hip_lib):
    with open(os.path.join(ROOT, "include", "pp_hip.h")) as f:
        hdr = f.read()
    assert "#define PP_ABI_VERSION 4" in hdr and hip_lib.pp_abi_version() == 4
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(pp_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    for name in ("pp_publish_train_weights", "pp_publish_info"):
        assert name in declared and name in pp._lib.EXPORTS and hasattr(hip_lib, name)
        assert name in hdr.split("#define PP_ABI_VERSION")[0], "listed among the later additions within 4"
    assert {"api_publish.hip", "weight_publish.hip"} <= set(pp._lib.SOURCES)
    m = re.search(r"typedef struct pp_publish_stats \{(.*?)\} pp_publish_stats;", hdr, flags=re.S)
    fields = re.findall(r"int64_t\s+([a-z0-9_]+);", m.group(1))
    assert fields == [n for n, _ in pp._lib.PPPublishStats._fields_]
    assert fields == ["publishes", "reallocations", "graph_invalidations", "f32_fallback_layers"]
    assert ctypes.sizeof(pp._lib.PPPublishStats) == 32
    assert hip_lib.pp_publish_train_weights(None, None, None) == 1 and hip_lib.pp_publish_info(None, None) == 1   # PP_ERR_ARG
