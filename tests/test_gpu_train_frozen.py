"""Frozen-layer fine-tuning on the GPU (Trainer(frozen=...), set_trainable; pp_train_set_frozen): the step with frozen
units against torch autograd (tests/frozen_ref.py), the state and optimizer after a step, bit-identity with nothing
frozen and across freeze changes on a live trainer, the launch structure of a frozen step, and the reference's
load -> set_trainable(False) -> train -> export workflow."""
import os

import numpy as np
import pytest
import torch

import frozen_ref
import util_ref
from oracle import train_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _small_cfg(pp, name, B=2):
    cfg = pp.config.tiny_config(B)
    s = cfg["model"]["second"]
    if name in ("deep", "deep-wide"):
        s["rpn"].update(layer_nums=[3, 5, 5])
    if name == "deep-wide":
        s["rpn"].update(num_filters=[64, 128, 256], num_upsample_filters=[128, 128, 128])
        s["voxel_feature_extractor"]["num_filters"] = 128
    return cfg


def _frames(seed, ns=(900, 400)):
    rng = np.random.default_rng(seed)
    return [rng.uniform([0, -0.64, -3], [1.6, 0.64, 3], (n, 3)).astype(np.float32) for n in ns]


def _targets(d, B, seed, npos=40):
    rng = np.random.default_rng(seed)
    A = d.num_anchors
    labels = rng.choice([-1, 0, 0, 0, 0], size=(B, A)).astype(np.int32)
    reg = np.zeros((B, A, 7), np.float32)
    for b in range(B):
        pos = rng.choice(A, npos if b == 0 else npos // 3, replace=False)
        labels[b, pos] = 1
        reg[b, pos] = rng.normal(0, 0.4, (len(pos), 7)).astype(np.float32)
    return labels, reg


def _moving_stats_near_the_batch(d, w, ex, labels, reg, seed):
    """Random moving statistics of the scale the network's batch statistics have (so that the inference-mode layers
    neither vanish nor explode): mean + 0.2 std N(0, 1), variance x U(0.6, 1.6)."""
    _, _, stats, _ = train_ref.training_step(d, w, ex, labels, reg, ex[6][0])
    rng = np.random.default_rng(seed)
    w = dict(w)
    for pre, (mean, var) in stats.items():
        w[pre + "/moving_mean"] = (mean + 0.2 * np.sqrt(var) * rng.normal(size=mean.shape)).astype(np.float32)
        w[pre + "/moving_variance"] = (var * rng.uniform(0.6, 1.6, var.shape)).astype(np.float32)
    return w


def _frozen_mask(tr):
    from pp_amd import trainer
    mask = np.zeros(tr.params.numel(), bool)
    for name, off, size, st in tr.layout:
        if not st and trainer.unit_of(name) in set(tr.frozen):
            mask[off:off + size] = True
    return mask


CASES = {
    "deep-reference": ("deep", "reference"),
    "deep-wide-reference": ("deep-wide", "reference"),
    "tiny-pfn": ("tiny", ["pfn"]),
    "deep-block2-deconv2": ("deep", [f"rpn/block2/{j}" for j in range(6)] + ["rpn/deconv2"]),
    "tiny-heads-and-deconv3": ("tiny", ["rpn/deconv3", "rpn/conv_cls", "rpn/block1/1"]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_frozen_gradients_match_autograd_small_grids(pp, hip_lib, case):
    """Losses to 1e-5, every trainable tensor's gradient to 1e-4 of its largest entry (the bar of the unfrozen
    test_gpu_train.py) against the float64 restatement, frozen entries of the gradient buffer exactly 0, and a second
    pass bit-identical."""
    from pp_amd import trainer
    name, frozen = CASES[case]
    B = 2
    cfg = _small_cfg(pp, name, B)
    d = pp.config.Derived(cfg)
    frames = _frames(4)
    labels, reg = _targets(d, B, 11)
    rect, trv, p2 = pp.synth.default_calib()
    ex, _ = util_ref.oracle_example(d, frames, rect, trv, p2)
    w = _moving_stats_near_the_batch(d, pp.weights.init_weights(d, seed=21), ex, labels, reg, 5)
    units = trainer.resolve_frozen(d, frozen)
    tr = pp.Trainer(cfg, w, max_batch=B, max_points_per_frame=4096, frozen=frozen)
    assert tr.frozen == units
    tr.grads.fill_(7.0)                         # stale values the step must overwrite
    out = tr.forward_backward(frames, labels, reg)
    g1 = tr.grads.cpu().numpy().copy()
    vals, want = frozen_ref.training_step(d, w, ex, labels, reg, ex[6][0], frozen=units, dtype=torch.float64)
    for k in ("loss", "loc_loss_reduced", "cls_loss_reduced", "dir_loss_reduced", "cls_pos_loss", "cls_neg_loss"):
        assert abs(out[k] - vals[k]) <= 1e-5 * max(1.0, abs(vals[k])), (k, out[k], vals[k])
    got = tr.gradients()
    assert sorted(got) == sorted(want)
    assert not any(trainer.unit_of(k) in set(units) for k in got)
    worst = ("", 0.0)
    for k, g in want.items():
        err = float(np.abs(got[k] - g).max()) / max(float(np.abs(g).max()), 1e-12)
        if err > worst[1]:
            worst = (k, err)
    print(f"{case}: worst relative gradient error {worst[1]:.2e} ({worst[0]})")
    assert worst[1] <= 1e-4, worst
    mask = _frozen_mask(tr)
    assert mask.any() and np.all(g1[mask] == 0.0)
    # BatchNorm of the frozen units: moving statistics untouched; trainable ones updated
    after = tr.weights()
    for k in w:
        if k.endswith(("moving_mean", "moving_variance")):
            if trainer.unit_of(k) in set(units):
                assert np.array_equal(after[k], w[k]), k
            else:
                assert not np.array_equal(after[k], w[k]), k
    out2 = tr.forward_backward(frames, labels, reg)
    assert out2["loss"] == out["loss"] and np.array_equal(tr.grads.cpu().numpy(), g1)
    tr.close()


def test_frozen_state_and_optimizer_shipped_config(pp, hip_lib):
    """cfg-A at B=2 with the reference freeze: after Trainer.step the frozen parameters, moving statistics and AdamW
    moments are bit-identical to before, the trainable moving statistics moved, and trainable parameters / m / v equal
    to the bit what a full-buffer k_adamw launch makes of the same inputs."""
    import ctypes
    B = 2
    cfg = pp.config.pedestrian_d435i_config(B)
    d = pp.config.Derived(cfg)
    frames = [pp.synth.d435i_cloud(30 + i, 16384) for i in range(B)]
    labels, reg = _targets(d, B, 11)
    w = pp.weights.init_weights(d, seed=21)
    tr = pp.Trainer(cfg, w, max_batch=B, max_points_per_frame=16384, frozen="reference")
    g = torch.Generator(device="cpu").manual_seed(3)
    tr.optimizer.m.copy_(torch.randn(tr.params.numel(), generator=g) * 1e-3)
    tr.optimizer.v.copy_(torch.rand(tr.params.numel(), generator=g) * 1e-6)
    tr.optimizer.iterations = 5
    p0, s0 = tr.params.clone(), tr.state.clone()
    m0, v0 = tr.optimizer.m.clone(), tr.optimizer.v.clone()
    lr_t = tr.optimizer.lr_t()
    tr.step(frames, labels, reg)
    torch.cuda.synchronize()
    mask = torch.from_numpy(_frozen_mask(tr)).to(tr.device)
    grads = tr.grads.clone()
    assert bool((grads[mask] == 0).all())
    # the reference: k_adamw over the whole buffer from the same parameters, gradients and moments
    pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
    opt = tr.optimizer
    st = hip_lib.pp_adamw_step_device(tr.device.index or 0, None, ctypes.c_void_p(pr.data_ptr()),
                                      ctypes.c_void_p(grads.data_ptr()), ctypes.c_void_p(mr.data_ptr()),
                                      ctypes.c_void_p(vr.data_ptr()), pr.numel(), lr_t, opt.beta_1, opt.beta_2,
                                      opt.epsilon, opt.weight_decay)
    assert st == 0
    torch.cuda.synchronize()
    train = ~mask
    assert torch.equal(tr.params[train], pr[train])
    assert torch.equal(opt.m[train], mr[train]) and torch.equal(opt.v[train], vr[train])
    assert torch.equal(tr.params[mask], p0[mask])
    assert torch.equal(opt.m[mask], m0[mask]) and torch.equal(opt.v[mask], v0[mask])
    assert not torch.equal(tr.params[train], p0[train])
    from pp_amd import trainer
    after = tr.weights()
    for name, off, size, is_state in tr.layout:
        if not is_state:
            continue
        if trainer.unit_of(name) in set(tr.frozen):
            assert np.array_equal(after[name], w[name]), name
        else:
            assert not np.array_equal(after[name], w[name]), name
    tr.close()


def _snapshot(tr):
    return [t.detach().cpu().numpy().copy() for t in (tr.params, tr.grads, tr.state, tr.optimizer.m, tr.optimizer.v)]


def test_nothing_frozen_is_bit_identical_to_the_unfrozen_trainer(pp, hip_lib):
    B = 2
    cfg = _small_cfg(pp, "deep", B)
    d = pp.config.Derived(cfg)
    frames = _frames(6)
    labels, reg = _targets(d, B, 12)
    w = pp.weights.init_weights(d, seed=8)
    runs = []
    for kind in ("absent", "None", "()", "set_trainable(True)"):
        kw = {} if kind == "absent" else {"frozen": None if kind == "None" else ("reference" if "set" in kind else ())}
        tr = pp.Trainer(cfg, w, max_batch=B, max_points_per_frame=4096, **kw)
        if kind == "set_trainable(True)":
            assert tr.frozen != ()
            tr.set_trainable(True)
            assert tr.frozen == ()
        losses = [tr.step(frames, labels, reg)["loss"] for _ in range(3)]
        runs.append((kind, losses, _snapshot(tr)))
        tr.close()
    for kind, losses, snap in runs[1:]:
        assert losses == runs[0][1], kind
        for a, b in zip(snap, runs[0][2]):
            assert np.array_equal(a, b), kind


def test_changing_the_freeze_on_a_live_trainer(pp, hip_lib):
    """unfrozen -> reference-frozen -> unfrozen on one trainer: every step matches, to the bit, a fresh trainer built
    with that step's freeze from the same weights, state and optimizer moments; each change re-captures the step's
    graphs once and every other step replays them."""
    B = 2
    cfg = _small_cfg(pp, "deep", B)
    d = pp.config.Derived(cfg)
    frames = _frames(7)
    labels, reg = _targets(d, B, 13)
    w = pp.weights.init_weights(d, seed=9)
    live = pp.Trainer(cfg, w, max_batch=B, max_points_per_frame=4096)
    per_phase = None
    for phase, frozen in enumerate((None, "reference", None)):
        live.set_frozen(frozen)
        c_before, r_before = live.engine.train_graph_stats()
        for k in range(3):
            fresh = pp.Trainer(cfg, live.weights(), max_batch=B, max_points_per_frame=4096, frozen=frozen)
            fresh.optimizer.m.copy_(live.optimizer.m)
            fresh.optimizer.v.copy_(live.optimizer.v)
            fresh.optimizer.iterations = live.optimizer.iterations
            a = live.step(frames, labels, reg)
            b = fresh.step(frames, labels, reg)
            assert a == b, (phase, k)
            for x, y in zip(_snapshot(live), _snapshot(fresh)):
                assert np.array_equal(x, y), (phase, k)
            fresh.close()
            if k == 1:
                c_mid = live.engine.train_graph_stats()[0]
        c_after, r_after = live.engine.train_graph_stats()
        assert r_after - r_before == 3
        assert c_after == c_mid            # the third step of a phase replays
        if per_phase is None:
            per_phase = c_after - c_before
            assert per_phase >= 1
        assert c_after - c_before == per_phase, (phase, c_after - c_before, per_phase)
    live.close()


def _names(pp, frozen):
    B = 2
    cfg = pp.config.pedestrian_d435i_config(B)
    d = pp.config.Derived(cfg)
    frames = [pp.synth.d435i_cloud(700 + i, 6000) for i in range(B)]
    labels, reg = _targets(d, B, 17)
    tr = pp.Trainer(cfg, pp.weights.init_weights(d, seed=7), max_batch=B, max_points_per_frame=8192, frozen=frozen)
    tr.engine.set_profiling(True)
    tr.forward_backward(frames, labels, reg)
    names = [n for n, _ in tr.engine.kernel_times()]
    tr.close()
    return d, names


def test_frozen_step_launch_structure(pp, hip_lib):
    from pp_amd import trainer
    d, full = _names(pp, None)
    _, fz = _names(pp, "reference")
    units = set(trainer.reference_frozen_units(d))
    seps = [u for u in trainer.train_units(d) if u.startswith("rpn/block")]
    bn_layers = [u for u in trainer.train_units(d) if u.startswith(("rpn/block", "rpn/deconv"))]

    def tag(u):
        return u[len("rpn/"):].replace("/", ".")
    assert not any(n.startswith("k_tr_pfn_bwd") for n in fz)
    for u in units - {"pfn"}:
        t = tag(u)
        assert not any(n.endswith((":pair." + t, ":wgrad." + t)) for n in fz), u
    # block1/0..2 have nothing trainable in front of them: no backward at all; block2/3's frozen layers pass the gradient
    for u in ("rpn/block1/0", "rpn/block1/1", "rpn/block1/2"):
        assert not any(n.endswith("." + tag(u)) and ":fwd." not in n for n in fz if n.startswith("k_tr_gemm")), u
    for u in ("rpn/block2/0", "rpn/block3/2"):
        assert "k_tr_gemm2:dgrad." + tag(u) in fz, u
    # depthwise-kernel gradients and BatchNorm finalizes: one per trainable layer
    n_dw = sum(n in ("k_tr_dw_bwd_w", "k_tr_dw_bwd") for n in fz)
    assert n_dw == len([u for u in seps if u not in units]), n_dw
    n_fin = sum(n.startswith("k_tr_bn_finalize") for n in fz)
    assert n_fin == len([u for u in bn_layers if u not in units]), n_fin
    assert sum(n.startswith("k_tr_bn_finalize") for n in full) == len(bn_layers) + 1
    assert fz.count("k_tr_bn_frozen") == 1
    assert len(fz) < len(full), (len(fz), len(full))
    print(f"launches: unfrozen {len(full)}, reference-frozen {len(fz)}")


def _gt(B, seed, x=(1.0, 5.5), y=(-1.5, 1.5)):
    rng = np.random.default_rng(seed)
    G = 4
    return [np.concatenate([rng.uniform(*x, (G, 1)), rng.uniform(*y, (G, 1)), np.full((G, 1), -0.9),
                            np.full((G, 1), 0.6), np.full((G, 1), 0.8), np.full((G, 1), 1.73),
                            rng.uniform(-np.pi, np.pi, (G, 1))], 1).astype(np.float32) for _ in range(B)]


def _finetune(pp, cfg, src, freeze, frames, gts, steps=3):
    from pp_amd import trainer
    d = pp.config.Derived(cfg)
    saved = pp.weights.load_any(src, d)
    net = pp.VoxelNet(cfg, training=True, max_batch=len(frames), max_points_per_frame=8192)
    net.load_weights(src)
    freeze(net)
    units = set(net.trainer.frozen)
    assert units
    for _ in range(steps):
        out = net.train_step(frames, gt_boxes=gts)
        assert np.isfinite(out["loss"])
    w = net.get_weights()
    changed = 0
    for k, v in saved.items():
        if trainer.unit_of(k) in units:
            assert np.array_equal(w[k], v), k
        else:
            changed += not np.array_equal(w[k], v)
    assert changed > 0
    net.trainer.close()
    eng = pp.Engine(cfg, max_batch=len(frames), max_points_per_frame=8192)
    eng.load_weights(w)
    dets, n = eng.detect(frames)
    assert n.shape == (len(frames),)
    eng.close()


def test_finetune_workflow_from_saved_weights(pp, hip_lib, tmp_path):
    """weights.save_npz -> VoxelNet(training=True).load_weights -> set_trainable(False) -> train_step(gt_boxes=...) ->
    weights(): the frozen tensors are the saved ones, and the export runs through inference."""
    B = 2
    cfg = pp.config.pedestrian_d435i_config(B)
    d = pp.config.Derived(cfg)
    path = str(tmp_path / "w.npz")
    pp.weights.save_npz(path, pp.weights.init_weights(d, seed=31))
    frames = [pp.synth.d435i_cloud(800 + i, 6000) for i in range(B)]
    _finetune(pp, cfg, path, lambda net: net.set_trainable(False), frames, _gt(B, 3))


def test_finetune_keras_checkpoint_with_explicit_units(pp, hip_lib):
    """The Keras .h5 checkpoint (tiny config, layer_nums [1, 1, 1]): the reference selection is refused, an explicit
    unit list fine-tunes."""
    B = 2
    cfg = pp.config.tiny_config(B)
    ckpt = os.path.join(GOLD, "keras_ckpt_tiny.h5")
    net = pp.VoxelNet(cfg, training=True, max_batch=B, max_points_per_frame=8192)
    net.load_weights(ckpt)
    with pytest.raises(ValueError):
        net.set_trainable(False)
    assert net.trainer.frozen == ()
    net.trainer.close()
    frames = _frames(9)
    _finetune(pp, cfg, ckpt, lambda net: net.trainer.set_frozen(["pfn", "rpn/block1/0"]), frames,
              _gt(B, 4, x=(0.3, 1.3), y=(-0.4, 0.4)))
