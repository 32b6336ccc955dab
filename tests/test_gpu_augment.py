"""Training-time augmentation on the GPU (csrc/augment.hip): pp_augment against the reference fixture and the host
float64 restatement (augment.augment_np), the three feeds, the fused augmented step against pp_augment +
pp_train_step_gt, seeding, and argument refusal."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _within_ulp(got, want, nulp=1):
    got = np.asarray(got, np.float32)
    want32 = np.asarray(want, np.float64).astype(np.float32)
    assert got.shape == want32.shape, (got.shape, want32.shape)
    sp = np.spacing(np.maximum(np.abs(got), np.abs(want32))).astype(np.float64)
    bad = np.abs(got.astype(np.float64) - want32.astype(np.float64)) > nulp * sp
    assert not bad.any(), (bad.sum(), got[bad][:4], want32[bad][:4])


def _close(got, want):
    """The issue's bar against the reference, which rounds to float32 after every stage: 2e-6 * max(1, |x|)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.abs(got - want) > 2e-6 * np.maximum(1.0, np.abs(want))
    assert not bad.any(), (bad.sum(), got[bad][:4], want[bad][:4])


def _engine(pp, cfg, B, n=8192):
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=n)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    return eng


def _near_face(pp, pts, boxes):
    if len(boxes) == 0 or len(pts) == 0:
        return 0
    n, d = pp.augment.box_planes(np.asarray(boxes, np.float64))
    sg = pp.augment.face_sign(np.asarray(pts, np.float64)[:, :3], n, d)
    dist = np.abs(sg) / np.linalg.norm(n, axis=-1)[None]
    return int((dist.min(axis=(1, 2)) < 1e-9).sum())


def _check_batch(pp, eng, frames, gts, valids, cfg, classes=None):
    pc = np.asarray(eng.d.pc_range, np.float64)
    draws = pp.augment.draw(np.random.RandomState(1), gts, cfg)
    eng.upload(frames)
    got = eng.augment(gts, classes, valids, draws, cfg)
    near = 0
    for b in range(len(frames)):
        pts, bx, cl = pp.augment.augment_np(frames[b], np.asarray(gts[b], np.float32), None if classes is None else classes[b],
                                            None if valids is None else valids[b], draws.frame(b), cfg, pc)
        near += _near_face(pp, frames[b], gts[b])
        gp, gb, gc = got[b]
        _within_ulp(gp, pts)
        assert len(gb) == len(bx), (b, len(gb), len(bx))
        _within_ulp(gb, bx)
        np.testing.assert_array_equal(gc, cl)
    print(f"points within 1e-9 m of a face (excluded from nothing, expected 0): {near}")
    assert near == 0
    return got


def test_fixture_cases_in_one_batch(pp, hip_lib):
    G = load_golden("ref_augment.npz")
    names = [str(n) for n in G["names"]]
    cfgs = []
    for c in names:
        v = G[c + "__cfg"]
        cfgs.append(pp.augment.AugmentConfig(v[0:2], v[2:5], v[5:7], v[7:9], v[9:11], v[11:14], int(v[14])))
    frames = [G[c + "__in_points"].astype(np.float32) for c in names]
    gts = [G[c + "__in_boxes"].reshape(-1, 7).astype(np.float32) for c in names]
    valids = [G[c + "__in_valid"].astype(bool) for c in names]
    # the v1 cases together, the v2 case on its own (the rule is per batch); each frame with its own seeded draws
    for group in ([i for i, c in enumerate(cfgs) if not c.global_rot_per_object],
                  [i for i, c in enumerate(cfgs) if c.global_rot_per_object]):
        d_all = [pp.augment.draw(np.random.RandomState(int(G[names[i] + "__seed"])), [gts[i]], cfgs[i]) for i in group]
        T = cfgs[group[0]].num_try
        draws = pp.augment.Draws([d.flip[0] for d in d_all], [d.theta[0] for d in d_all], [d.scale[0] for d in d_all],
                                 [d.t[0] for d in d_all], [d.seed[0] for d in d_all],
                                 np.concatenate([d.boxes for d in d_all]).reshape(-1, T, 5),
                                 [d.counts[0] for d in d_all])
        eng2 = _engine(pp, pp.config.pedestrian_d435i_config(len(group)), len(group))
        eng2.upload([frames[i] for i in group])
        got = eng2.augment([gts[i] for i in group], None, [valids[i] for i in group], draws, cfgs[group[0]])
        sel = eng2.augment_selected()
        g0 = 0
        for k, i in enumerate(group):
            c = names[i]
            gp, gb, gc = got[k]
            np.testing.assert_array_equal(sel[g0:g0 + len(gts[i])], G[c + "__selected"], err_msg=c)
            g0 += len(gts[i])
            want_b = G[c + "__out_boxes"]
            assert len(gb) == len(want_b), c
            _close(gb, want_b)
            pre = np.empty_like(gp)
            pre[pp.augment.shuffle_perm(int(draws.seed[k]), len(gp))] = gp
            _close(pre[:, :3], G[c + "__s6_points"][:, :3])
        eng2.close()


@pytest.mark.parametrize("v2", [False, True])
def test_random_batches_cfg_a(pp, hip_lib, v2):
    rng = np.random.default_rng(5 + v2)
    B = 32
    cfg = pp.config.pedestrian_d435i_config(B)
    eng = _engine(pp, cfg, B)
    frames = [pp.synth.d435i_cloud(300 + i, 6000) for i in range(B)]
    gts, valids = [], []
    for b in range(B):
        G = int(rng.integers(0, 17))
        g = np.concatenate([rng.uniform(0.3, 6.2, (G, 1)), rng.uniform(-2.4, 2.4, (G, 1)), rng.uniform(-1.2, -0.4, (G, 1)),
                            rng.uniform(0.4, 0.9, (G, 1)), rng.uniform(0.5, 1.0, (G, 1)), rng.uniform(1.4, 1.9, (G, 1)),
                            rng.uniform(-np.pi, np.pi, (G, 1))], 1).astype(np.float32)
        gts.append(g)
        valids.append(rng.uniform(size=G) < 0.8)
    acfg = pp.augment.AugmentConfig.from_input_reader(
        {"global_random_rotation_range_per_object": [-0.3, 0.3]} if v2 else {})
    _check_batch(pp, eng, frames, gts, valids, acfg)
    eng.close()


def test_random_batch_cfg_k(pp, hip_lib):
    rng = np.random.default_rng(9)
    B = 8
    cfg = pp.config.kitti_shaped_config(B)
    eng = _engine(pp, cfg, B, n=20000)
    frames = [pp.synth.kitti_cloud(40 + i, 16000) for i in range(B)]
    gts, cls = [], []
    for b in range(B):
        G = int(rng.integers(0, 17))
        g = np.concatenate([rng.uniform(2, 60, (G, 1)), rng.uniform(-30, 30, (G, 1)), rng.uniform(-1.5, -0.5, (G, 1)),
                            rng.uniform(0.5, 2.0, (G, 1)), rng.uniform(0.5, 4.5, (G, 1)), rng.uniform(1.4, 1.9, (G, 1)),
                            rng.uniform(-np.pi, np.pi, (G, 1))], 1).astype(np.float32)
        gts.append(g)
        cls.append(np.ones(G, np.int32))
    got = _check_batch(pp, eng, frames, gts, None, pp.augment.AugmentConfig.from_input_reader({}), cls)
    for b in range(B):          # the reflectance travels with its point
        np.testing.assert_array_equal(np.sort(got[b][0][:, 3]), np.sort(frames[b][:, 3]))
    eng.close()


def test_feeds_give_identical_bits(pp, hip_lib):
    B = 2
    cfg = pp.config.pedestrian_d435i_config(B)
    frames = [pp.synth.d435i_cloud(70 + i, 5000) for i in range(B)]
    gts = [np.array([[2.0, 0.3, -0.6, 0.6, 0.8, 1.7, 0.2], [4.0, -1.0, -0.6, 0.6, 0.8, 1.7, 1.2]], np.float32)] * B
    acfg = pp.augment.AugmentConfig.from_input_reader({})
    draws = pp.augment.draw(np.random.RandomState(3), gts, acfg)
    eng = _engine(pp, cfg, B)
    eng.upload(frames)
    a = eng.augment(gts, draws=draws, aug_config=acfg)
    st = eng.staging(frames)                        # B <= 4: the zero-copy feed
    eng.upload_async(st)
    b = eng.augment(gts, draws=draws, aug_config=acfg)
    eng.sync()
    eng2 = _engine(pp, pp.config.pedestrian_d435i_config(6), 6)
    st2 = eng2.staging(frames * 3)                  # B > 4: the copy feed (the first two frames draw the same numbers)
    eng2.upload_async(st2)
    c = eng2.augment(gts * 3, draws=pp.augment.draw(np.random.RandomState(3), gts * 3, acfg), aug_config=acfg)[:2]
    for x, y in ((a, b), (a, c)):
        for fa, fb in zip(x, y):
            for ka, kb in zip(fa, fb):
                assert np.array_equal(ka, kb)
    eng.close()
    eng2.close()


def _problem(pp, B, seed=3, two_class=False):
    """cfg-A frames with 4 pedestrian boxes each, or (two_class) a KITTI-shaped 2-class config with 6 boxes of
    mixed classes per frame; returns (config, classes per frame or None, frames, boxes per frame)."""
    rng = np.random.default_rng(seed)
    if two_class:
        cfg = pp.config.kitti_shaped_config(B, num_class=2)
        frames = [pp.synth.kitti_cloud(600 + seed * 10 + i, 8000) for i in range(B)]
        lo, hi, G = (4.0, -20.0), (40.0, 20.0), 6
    else:
        cfg = pp.config.pedestrian_d435i_config(B)
        frames = [pp.synth.d435i_cloud(500 + seed * 10 + i, 6000) for i in range(B)]
        lo, hi, G = (1.0, -1.5), (5.5, 1.5), 4
    gts, cls = [], []
    for b in range(B):
        g = np.concatenate([rng.uniform(lo[0], hi[0], (G, 1)), rng.uniform(lo[1], hi[1], (G, 1)), np.full((G, 1), -0.9),
                            np.full((G, 1), 0.6), np.full((G, 1), 0.8), np.full((G, 1), 1.73),
                            rng.uniform(-np.pi, np.pi, (G, 1))], 1).astype(np.float32)
        gts.append(g)
        cls.append(np.arange(G, dtype=np.int32) % 2 + 1)
    return cfg, (cls if two_class else None), frames, gts


def _trainer(pp, cfg, B, **kw):
    return pp.Trainer(cfg, pp.weights.init_weights(pp.config.Derived(cfg), seed=7), max_batch=B, max_points_per_frame=8192,
                      learning_rate=2e-4, weight_decay=1e-4, **kw)


@pytest.mark.parametrize("staged,two_class", [(False, False), (True, False), (False, True), (True, True)])
def test_fused_step_equals_augment_then_gt_step(pp, hip_lib, staged, two_class):
    """The fused augmented step and pp_augment + pp_train_step_gt on its outputs: the same losses and the same bits in
    every gradient and statistic.  two_class: a 2-class config with mixed classes (the classes must follow their
    boxes through the compaction into the targets)."""
    B = 2
    cfg, cls, frames, gts = _problem(pp, B, two_class=two_class)
    acfg = pp.augment.AugmentConfig.from_input_reader({})
    ta = _trainer(pp, cfg, B, augment=acfg, seed=11)
    tb = _trainer(pp, cfg, B)
    rs = np.random.RandomState(11)
    rev = (lambda x: None if x is None else x[::-1])  # noqa: E731
    batches = [ta.stage_gt(frames, gts, cls), ta.stage_gt(frames[::-1], gts[::-1], rev(cls))] if staged else None
    for i in range(4):
        fr, gt, gc = (frames, gts, cls) if i % 2 == 0 else (frames[::-1], gts[::-1], rev(cls))
        if staged:
            a = ta.forward_backward(batches[i % 2], prefetch=batches[(i + 1) % 2])
        else:
            a = ta.forward_backward(fr, gt_boxes=gt, gt_classes=gc)
        draws = batches[i % 2].aug[1] if staged else pp.augment.draw(rs, gt, acfg)
        tb.engine.upload(fr)
        out = tb.engine.augment(gt, gc, draws=draws, aug_config=acfg)
        if two_class:
            kept = np.concatenate([o[2] for o in out])
            assert (kept == 1).any() and (kept == 2).any(), kept
        kb, kc, kn = tb.engine.pack_gt([o[1] for o in out], [o[2] for o in out])
        tb.engine.train_step_gt_async(tb.params.data_ptr(), tb.grads.data_ptr(), tb.state.data_ptr(), kb, kc, kn)
        b = tb.engine.train_step_wait()
        assert a == b, (i, a, b)
        assert np.array_equal(ta.grads.cpu().numpy(), tb.grads.cpu().numpy()), i
        assert np.array_equal(ta.state.cpu().numpy(), tb.state.cpu().numpy()), i
        if i == 1:      # a graph per input buffer: both captured by now
            c0, r0 = ta.engine.train_graph_stats()
    c1, r1 = ta.engine.train_graph_stats()
    assert c1 == c0 and r1 == r0 + 2, (c0, r0, c1, r1)
    if batches:
        for s in batches:
            s.close()
    ta.close()
    tb.close()


def test_seeded_trainers_agree(pp, hip_lib):
    B = 2
    cfg, _, frames, gts = _problem(pp, B, seed=5)
    ws = []
    for seed in (21, 21, 22):
        t = _trainer(pp, cfg, B, augment=True, seed=seed)
        for _ in range(3):
            t.step(frames, gt_boxes=gts)
        ws.append(t.params.cpu().numpy().copy())
        t.close()
    assert np.array_equal(ws[0], ws[1])
    assert not np.array_equal(ws[0], ws[2])


def test_dense_labels_refused_when_augmenting(pp, hip_lib):
    B = 1
    cfg, _, frames, gts = _problem(pp, B)
    t = _trainer(pp, cfg, B, augment=True, seed=0)
    A = t.engine.d.num_anchors
    with pytest.raises(ValueError):
        t.step(frames[:1], np.zeros((1, A), np.int32), np.zeros((1, A, 7), np.float32))
    t.close()


def test_refused_arguments_leave_handle_usable(pp, hip_lib):
    B = 2
    cfg, _, frames, gts = _problem(pp, B)
    t = _trainer(pp, cfg, B)
    eng, L = t.engine, t.engine._lib
    eng.upload(frames)
    acfg = pp.augment.AugmentConfig.from_input_reader({})
    draws = pp.augment.draw(np.random.RandomState(0), gts, acfg)
    boxes, cls, counts = eng.pack_gt(gts)
    fr = draws.frames_struct()
    bd = np.ascontiguousarray(draws.boxes)
    pts = np.empty((sum(len(f) for f in frames), 3), np.float32)
    bo = np.empty((len(boxes), 7), np.float32)
    co = np.empty((len(boxes),), np.int32)
    cn = np.empty((B,), np.int32)

    def call(boxes=boxes, counts=counts, batch=B, num_try=100, fr=fr, bd=bd):
        ac = pp._lib.PPAugmentConfig()
        ac.num_try, ac.global_rot_per_object = num_try, 0
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        return L.pp_augment(eng._h, p(boxes), None, None, p(counts), batch, ctypes.byref(ac), fr.ctypes.data,
                            bd.ctypes.data, p(pts), p(bo), p(co), p(cn))

    bad_box = boxes.copy()
    bad_box[0, 3] = -1
    nan_box = boxes.copy()
    nan_box[1, 0] = np.nan
    bad_cnt = counts.copy()
    bad_cnt[0] = 300
    fr_scale = fr.copy()
    fr_scale["scale"][0] = 0.0
    fr_nan = fr.copy()
    fr_nan["theta"][1] = np.inf
    bd_nan = bd.copy()
    bd_nan[0, 5, 3] = np.nan
    for kw in ({"boxes": bad_box}, {"boxes": nan_box}, {"counts": bad_cnt}, {"batch": 1}, {"num_try": 0},
               {"num_try": 129}, {"fr": fr_scale}, {"fr": fr_nan}, {"bd": bd_nan}):
        assert call(**kw) == 1, kw        # PP_ERR_ARG
        assert L.pp_last_error(eng._h)
    assert call() == 0
    lc, tc = eng.loss_config(), eng.target_config()
    ptrs = [ctypes.c_void_p(t.params.data_ptr()), ctypes.c_void_p(t.grads.data_ptr()), ctypes.c_void_p(t.state.data_ptr())]
    losses = np.zeros(8, np.float32)

    def step(boxes=boxes, counts=counts, batch=B, num_try=100, fr=fr, bd=bd):
        ac = pp._lib.PPAugmentConfig()
        ac.num_try, ac.global_rot_per_object = num_try, 0
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        return L.pp_train_step_aug(eng._h, *ptrs, p(boxes), None, p(counts), batch, ctypes.byref(lc), ctypes.byref(tc),
                                   None, ctypes.byref(ac), fr.ctypes.data, bd.ctypes.data, p(losses))

    eng.upload(frames)
    for kw in ({"boxes": bad_box}, {"counts": bad_cnt}, {"batch": 1}, {"num_try": 129}, {"fr": fr_scale},
               {"fr": fr_nan}, {"bd": bd_nan}):
        assert step(**kw) == 1, kw
    assert step() == 0 and np.isfinite(losses[0])
    t.step(frames, gt_boxes=gts)
    t.close()


def test_voxelnet_passes_augmentation_through(pp, hip_lib):
    B = 2
    cfg, _, frames, gts = _problem(pp, B, seed=7)
    w = pp.weights.init_weights(pp.config.Derived(cfg), seed=7)
    net = pp.VoxelNet(cfg, training=True, max_batch=B, max_points_per_frame=8192, augment=True, seed=4)
    net.load_weights(w)
    t = pp.Trainer(cfg, w, max_batch=B, max_points_per_frame=8192, augment=True, seed=4)
    valid = [np.array([True, False, True, True])] * B
    for _ in range(2):
        a = net.train_step(frames, gt_boxes=gts, gt_valid=valid, apply=False)
        b = t.forward_backward(frames, gt_boxes=gts, gt_valid=valid)
        assert a == b
        assert np.array_equal(net.trainer.grads.cpu().numpy(), t.grads.cpu().numpy())
    plain = pp.VoxelNet(cfg, training=True, max_batch=B, max_points_per_frame=8192)
    plain.load_weights(w)
    assert plain.train_step(frames, gt_boxes=gts, apply=False) != a
    for x in (net.trainer, t, plain.trainer):
        x.close()
