"""Detection during training (pp_publish_train_weights, csrc/weight_publish.hip; Engine.publish_weights, Trainer.publish /
detect, VoxelNet(training=True).detect).  The yardstick everywhere is the host route on the same machine: engine R is
loaded with load_weights(<the same tensors>), engine P (or the trainer's own engine) gets them by a publish, and head
maps, canvas and detections must be EQUAL (np.array_equal / bytes): both routes have to leave the same weight bytes and
the inference path is deterministic.

Variants of the issue's item 4 that exist:
  * the shipped configuration at B = 1 (64 / 128 / 256 channels, 128-channel head slices: four 32-channel groups in
    the head permutation) -- test_shipped_configuration;
  * the unfused head layer: a configuration whose last transposed convolution reads a 3 x 3 map (9 pixels, not a
    multiple of 4) fails deconv_can_fuse_heads without any environment switch -- test_unfused_head_layer;
  * a layer with cin % 16 != 0 does NOT exist: the backbone launcher refuses every layer with cin % 32 != 0
    (PP_ERR_UNSUPPORTED), so no accepted configuration reaches it.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NPTS = 4096


def _frames(pp, B, F=3, first=300):
    return [pp.synth.d435i_cloud(first + i, NPTS, F) for i in range(B)]


def _tiny(pp, B=2, **second):
    cfg = pp.config.tiny_config(B)
    for k, v in second.items():
        if k == "with_distance":
            cfg["model"]["second"]["voxel_feature_extractor"]["with_distance"] = v
        else:
            cfg["model"]["second"][k] = v
    return cfg


def _engine(pp, cfg, B, precision="split_f16"):
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=NPTS)
    eng.set_gemm_precision(precision)
    return eng


def _flat(eng, w):
    """The tensors of `w` as the flat (params, state) device buffers of eng.train_layout()."""
    layout, n_params, n_state = eng.train_layout()
    p, s = np.zeros(n_params, np.float32), np.zeros(n_state, np.float32)
    for name, off, size, is_state in layout:
        (s if is_state else p)[off:off + size] = np.asarray(w[name], np.float32).reshape(-1)
    out = torch.from_numpy(p).cuda(), torch.from_numpy(s).cuda()
    torch.cuda.synchronize()
    return out


def _publish(eng, w):
    p, s = _flat(eng, w)
    eng.publish_weights(p.data_ptr(), s.data_ptr())      # returns with the weights usable: p, s may go


def _outputs(eng, frames, detect=None):
    dets, n = (detect or eng.detect)(frames, on_numeric="raise")
    return dets.copy(), n.copy(), eng.intermediates(canvas=True)


def _assert_same(got, want):
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert int(want[1].sum()) > 0, "the case detects nothing: it would compare empty lists"
    for b, n in enumerate(want[1]):
        assert got[0][b, :n].tobytes() == want[0][b, :n].tobytes(), f"detections of frame {b}"
    assert sorted(got[2]) == sorted(want[2])
    for k in want[2]:
        assert np.array_equal(got[2][k], want[2][k]), k


def _targets(d, B, seed, npos=40):
    rng = np.random.default_rng(seed)
    A = d.num_anchors
    labels = rng.choice([-1, 0, 0, 0, 0], size=(B, A)).astype(np.int32)
    reg = np.zeros((B, A, 7), np.float32)
    for b in range(B):
        pos = rng.choice(A, npos, replace=False)
        labels[b, pos] = 1
        reg[b, pos] = rng.normal(0, 0.4, (npos, 7)).astype(np.float32)
    return labels, reg


def _check_routes(pp, cfg, B, w, precision="split_f16", F=3):
    """R loaded through the host, P published: equal outputs.  Returns P's info."""
    frames = _frames(pp, B, F)
    R, P = _engine(pp, cfg, B, precision), _engine(pp, cfg, B, precision)
    try:
        R.load_weights(w)
        _publish(P, w)
        assert P.weights_loaded
        info, rinfo = P.publish_info(), R.publish_info()
        print("publish_info", info, "host route", rinfo)
        assert info["publishes"] == 1 and info["reallocations"] == 1
        assert rinfo["publishes"] == 0 and info["f32_fallback_layers"] == rinfo["f32_fallback_layers"]
        _assert_same(_outputs(P, frames), _outputs(R, frames))
        return info
    finally:
        R.close()
        P.close()


@pytest.mark.parametrize("precision", ["split_f16", "f32"])
def test_trainer_detects_with_its_weights_before_and_after_steps(pp, hip_lib, precision):
    """tiny_config, B = 2: after set_weights only, and again after two optimizer steps (parameters AND moving
    statistics have moved), the trainer's detect equals a host-loaded engine's."""
    B = 2
    cfg = _tiny(pp, B)
    frames = _frames(pp, B)
    tr = pp.Trainer(cfg, pp.weights.init_weights(pp.config.Derived(cfg), seed=21), max_batch=B, max_points_per_frame=NPTS)
    R = _engine(pp, cfg, B, precision)
    try:
        tr.engine.set_gemm_precision(precision)
        d = tr.engine.d
        n_fallback = sum(1 for kind, _, _ in pp.weights.layer_table(d) if kind != "head") if precision == "f32" else 0
        w0 = tr.weights()
        R.load_weights(w0)
        _assert_same(_outputs(tr.engine, frames, tr.detect), _outputs(R, frames))
        assert tr.engine.publish_info()["f32_fallback_layers"] == R.publish_info()["f32_fallback_layers"] == n_fallback
        assert tr.publish() is False          # nothing changed since detect published
        labels, reg = _targets(d, B, 11)
        for _ in range(2):
            tr.step(frames, labels, reg)
        w2 = tr.weights()
        moved = [k for k in w0 if not np.array_equal(w0[k], w2[k])]
        assert any(k.endswith("moving_variance") for k in moved) and any(k.endswith("kernel") for k in moved)
        R.load_weights(w2)
        _assert_same(_outputs(tr.engine, frames, tr.detect), _outputs(R, frames))
        assert tr.engine.publish_info()["publishes"] == 2
    finally:
        tr.close()
        R.close()


def test_two_classes_without_direction_head(pp, hip_lib):
    """num_class = 2, no direction classifier: the head matrix is box | cls (2 per anchor) | zero pad."""
    cfg = _tiny(pp, 2, num_class=2, use_direction_classifier=False)
    cfg["eval_input_reader"]["desired_objects"] = ["Pedestrian", "Cyclist"]
    _check_routes(pp, cfg, 2, pp.weights.init_weights(pp.config.Derived(cfg), seed=5))


def test_with_distance_widens_the_pfn(pp, hip_lib):
    cfg = _tiny(pp, 2, with_distance=True)
    d = pp.config.Derived(cfg)
    w = pp.weights.init_weights(d, seed=6)
    assert w["pfn/dense/kernel"].shape[0] == d.num_point_features + 6
    _check_routes(pp, cfg, 2, w)


def test_shipped_configuration(pp, hip_lib):
    """64 / 128 / 256 channels, 128-channel head slices: more than one 32-channel group in the head permutation."""
    cfg = pp.config.pedestrian_d435i_config(1)
    info = _check_routes(pp, cfg, 1, pp.weights.init_weights(pp.config.Derived(cfg), seed=7))
    assert info["f32_fallback_layers"] == 0


def test_unfused_head_layer(pp, hip_lib):
    """A 12 x 12 grid: deconv3 reads a 3 x 3 map, deconv_can_fuse_heads fails, the heads are a layer of their own
    (concat buffer + [PP_HEAD_COLS][CC] matrix)."""
    cfg = _tiny(pp, 2)
    cfg["eval_input_reader"]["feature_map_size"] = [1, 12, 12]
    s = cfg["model"]["second"]
    s["voxel_generator"]["point_cloud_range"] = [0, -0.48, -3.0, 0.96, 0.48, 3.0]
    s["target_assigner"]["anchor_generators"]["anchor_generator_stride"]["offsets"] = [0.08, -0.48, -1.465]
    probe = pp.Engine(cfg, max_batch=2, max_points_per_frame=NPTS)
    try:
        probe.load_weights(pp.weights.init_weights(probe.d, seed=8))
        tags = probe.layer_tags()
    finally:
        probe.close()
    # six separable layers + three transposed convolutions + the head layer: the configuration reaches the unfused path
    assert len(tags) == 10 and tags[-1].endswith("heads"), tags
    _check_routes(pp, cfg, 2, pp.weights.init_weights(pp.config.Derived(cfg), seed=8))


def _out_of_range(w, S=1.0e6):
    """`w` with the folded weights of rpn/block1/1 scaled by S (beyond 32768: the layer leaves the float16 pieces) and
    its input scaled by 1 / S, so that the network computes what it computed (ReLU and the depthwise taps commute with
    a positive factor) and the outputs stay finite."""
    w = copy.deepcopy(w)
    for k in ("gamma", "beta"):
        w["rpn/block1/0/bn/" + k] = (w["rpn/block1/0/bn/" + k] / np.float32(S)).astype(np.float32)
    w["rpn/block1/1/bn/gamma"] = (w["rpn/block1/1/bn/gamma"] * np.float32(S)).astype(np.float32)
    w["rpn/block1/1/bn/moving_mean"] = (w["rpn/block1/1/bn/moving_mean"] / np.float32(S)).astype(np.float32)
    return w


def test_range_fallback_in_and_out(pp, hip_lib):
    B = 2
    cfg = _tiny(pp, B)
    frames = _frames(pp, B)
    w = pp.weights.init_weights(pp.config.Derived(cfg), seed=9)
    big = _out_of_range(w)
    R, P = _engine(pp, cfg, B), _engine(pp, cfg, B)
    try:
        _publish(P, w)
        ref = _outputs(P, frames)                        # captures P's graphs for the in-range pattern
        i0 = P.publish_info()
        assert i0["f32_fallback_layers"] == 0
        _publish(P, big)
        R.load_weights(big)
        i1 = P.publish_info()
        print("fallback layers: published", i1["f32_fallback_layers"], "host", R.publish_info()["f32_fallback_layers"])
        assert i1["f32_fallback_layers"] == R.publish_info()["f32_fallback_layers"] == 1
        assert i1["graph_invalidations"] == i0["graph_invalidations"] + 1 and i1["reallocations"] == 1
        _assert_same(_outputs(P, frames), _outputs(R, frames))
        _publish(P, w)                                   # back: same allocations, the other instantiation again
        i2 = P.publish_info()
        assert i2["f32_fallback_layers"] == 0 and i2["reallocations"] == 1
        assert i2["graph_invalidations"] == i1["graph_invalidations"] + 1
        R.load_weights(w)
        got = _outputs(P, frames)
        _assert_same(got, _outputs(R, frames))
        _assert_same(got, ref)
    finally:
        R.close()
        P.close()


def test_second_publish_is_in_place(pp, hip_lib):
    B = 2
    cfg = _tiny(pp, B)
    frames = _frames(pp, B)
    d = pp.config.Derived(cfg)
    w1, w2 = pp.weights.init_weights(d, seed=12), pp.weights.init_weights(d, seed=13)
    R, P = _engine(pp, cfg, B), _engine(pp, cfg, B)
    try:
        _publish(P, w1)
        first = _outputs(P, frames)
        i1 = P.publish_info()
        _publish(P, w2)
        i2 = P.publish_info()
        assert i2["publishes"] == i1["publishes"] + 1
        assert i2["reallocations"] == i1["reallocations"] and i2["graph_invalidations"] == i1["graph_invalidations"]
        second = _outputs(P, frames)                     # replays the graphs captured for w1
        R.load_weights(w2)
        _assert_same(second, _outputs(R, frames))
        assert not np.array_equal(first[2]["box_preds"], second[2]["box_preds"])
    finally:
        R.close()
        P.close()


def test_published_weights_win_and_host_weights_win_back(pp, hip_lib):
    B = 2
    cfg = _tiny(pp, B)
    frames = _frames(pp, B)
    d = pp.config.Derived(cfg)
    wa, wb = pp.weights.init_weights(d, seed=14), pp.weights.init_weights(d, seed=15)
    R, P = _engine(pp, cfg, B, "f32"), _engine(pp, cfg, B)
    try:
        P.load_weights(wa)
        _publish(P, wb)
        P.set_gemm_precision("f32")                      # must re-derive from the published B, not from A's leftovers
        R.load_weights(wb)
        _assert_same(_outputs(P, frames), _outputs(R, frames))
        assert P.publish_info()["f32_fallback_layers"] == R.publish_info()["f32_fallback_layers"] > 0
        P.load_weights(wa)
        R.load_weights(wa)
        _assert_same(_outputs(P, frames), _outputs(R, frames))
        _publish(P, wb)                                  # and a publish after a host load allocates again
        assert P.publish_info()["reallocations"] == 2
        R.load_weights(wb)
        _assert_same(_outputs(P, frames), _outputs(R, frames))
    finally:
        R.close()
        P.close()


def test_training_voxelnet_detects(pp, hip_lib):
    """VoxelNet(training=True): load_weights, train_step, detect == an inference VoxelNet loaded with get_weights().
    Without the feature this ends in "pp_detect_async: weights not finalised"."""
    B = 2
    cfg = _tiny(pp, B)
    frames = _frames(pp, B)
    net = pp.VoxelNet(cfg, training=True, max_batch=B, max_points_per_frame=NPTS)
    ref = pp.VoxelNet(cfg, training=False, max_batch=B, max_points_per_frame=NPTS)
    try:
        net.load_weights(pp.weights.init_weights(net.d, seed=16))
        labels, reg = _targets(net.d, B, 17)
        net.train_step(frames, labels, reg)
        got = net.detect(frames)
        ref.load_weights(net.get_weights())
        want = ref.detect(frames)
        assert len(got) == len(want) == B and any(x["scores"] is not None for x in want)
        for g, x in zip(got, want):
            assert sorted(g) == sorted(x)
            for k in x:
                if x[k] is None:
                    assert g[k] is None, k
                else:
                    assert np.array_equal(g[k], x[k]), k
    finally:
        net.trainer.close()
        ref.engine.close()


def test_detect_between_steps_does_not_disturb_training(pp, hip_lib):
    """step, step against step, detect, step: parameters, moving statistics and AdamW moments bit-identical; detect
    with a prefetched batch pending raises."""
    B = 2
    cfg = _tiny(pp, B)
    frames, other = _frames(pp, B), _frames(pp, B, first=340)
    d = pp.config.Derived(cfg)
    w = pp.weights.init_weights(d, seed=18)
    labels, reg = _targets(d, B, 19)
    a = pp.Trainer(cfg, w, max_batch=B, max_points_per_frame=NPTS)
    b = pp.Trainer(cfg, w, max_batch=B, max_points_per_frame=NPTS)
    try:
        a.step(frames, labels, reg)
        a.step(frames, labels, reg)
        b.step(frames, labels, reg)
        _, n = b.detect(other)
        assert int(n.sum()) > 0
        b.step(frames, labels, reg)
        for name in ("params", "state"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert torch.equal(a.optimizer.m, b.optimizer.m) and torch.equal(a.optimizer.v, b.optimizer.v)
        assert a.optimizer.iterations == b.optimizer.iterations == 2
        tb1, tb2 = b.stage(frames, labels, reg), b.stage(other, labels, reg)
        b.forward_backward(tb1, prefetch=tb2)
        with pytest.raises(RuntimeError, match="prefetched"):
            b.detect(other)
        b.forward_backward(tb2)                          # the prefetched batch trains; detect works again
        b.detect(other)
        tb1.close()
        tb2.close()
    finally:
        a.close()
        b.close()
