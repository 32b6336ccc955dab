"""GT-database sampling on the GPU (csrc/gt_sample.hip): pp_gt_sample against the reference fixture and the host
float64 restatement (gt_sampler.sample_all_np) -- decisions equal, clouds bit-identical --, frames without boxes, the
three feeds, run-to-run identity, what follows on the grown frames, and argument refusal."""
import random

import numpy as np
import pytest

from conftest import load_golden
from test_gt_sampler_host import DB_CLASSES, case_cfg, fixture_db

pytestmark = pytest.mark.gpu


def _cfg(pp, B, num_class=1):
    cfg = pp.config.pedestrian_d435i_config(B)
    cfg["model"]["second"]["num_class"] = num_class
    return cfg


def _ped_db(pp, F=3, max_num=8):
    """The fixture's Pedestrian objects as a one-class database."""
    gts = pp.gt_sampler
    full = fixture_db(pp, F)
    n = int((full.classes == 1).sum())
    infos = {"Pedestrian": [{"box3d_lidar": full.boxes[i], "difficulty": 0, "num_points_in_gt": 9} for i in range(n)]}
    points = {"Pedestrian": [full.object_points(i) for i in range(n)]}
    cfg = gts.SamplerConfig.from_input_reader({"sample_classes": ["Pedestrian"], "sample_max_nums": [max_num],
                                               "sampler_noise_x_closer": [0, 0], "sampler_noise_x_farther": [0, 0],
                                               "sampler_noise_y": [0, 0]})
    return gts.GtDatabase(infos, points, cfg, np.random.RandomState(5), random.Random(5), F)


def _near_face(pp, pts, boxes):
    if len(boxes) == 0 or len(pts) == 0:
        return 0
    n, d = pp.augment.box_planes(np.asarray(boxes, np.float64))
    sg = pp.augment.face_sign(np.asarray(pts, np.float64)[:, :3], n, d)
    dist = np.abs(sg) / np.linalg.norm(n, axis=-1)[None]
    return int((dist.min(axis=(1, 2)) < 1e-9).sum())


def _near_touching(pp, frame_boxes, cand_boxes):
    """Box pairs whose collision decision changes when a candidate moves by 1e-9 m."""
    aug = pp.augment
    if len(cand_boxes) == 0:
        return 0
    fb = np.asarray(frame_boxes, np.float64).reshape(-1, 7)
    every = np.concatenate([fb, cand_boxes], 0)
    ec = aug.box_corners_2d(*(every[:, k] for k in (0, 1, 3, 4, 6)))
    cc = ec[len(fb):]
    base = aug.collide(cc[:, None], ec[None])
    flips = np.zeros_like(base)
    for dx, dy in ((1e-9, 0), (-1e-9, 0), (0, 1e-9), (0, -1e-9)):
        flips |= aug.collide((cc + np.array([dx, dy]))[:, None], ec[None]) != base
    flips[np.arange(len(cc)), len(fb) + np.arange(len(cc))] = False
    return int(flips.sum())


def _compare(pp, eng, db, frames, gt, classes, valids, cand, cfg):
    """Uploads, samples on the GPU, and compares every frame with sample_all_np.  Returns the GPU's outputs."""
    gts = pp.gt_sampler
    eng.upload(frames)
    got = eng.gt_sample(gt, classes, valids, cand, cfg)
    tap = eng.gt_sample_info()
    near = touching = 0
    for b in range(len(frames)):
        pts, bx, cl, va, info = gts.sample_all_np(frames[b], np.asarray(gt[b], np.float32), None if classes is None else classes[b],
                                                  None if valids is None else valids[b], db, cand.cands[b], cand.counts[b],
                                                  cfg, return_info=True)
        n = int(cand.counts[b].sum())
        cb = db.boxes[cand.cands["object"][b, :n]]
        near += _near_face(pp, frames[b], cb)
        s0 = 0
        for r in range(gts.PP_GTS_MAX_ROUNDS):
            s1 = s0 + int(cand.counts[b, r])
            touching += _near_touching(pp, gt[b], cb[s0:s1])
            s0 = s1
        gp, gb, gc, gv = got[b]
        np.testing.assert_array_equal(tap["status"][b], info["status"], err_msg=f"frame {b}")
        np.testing.assert_array_equal(tap["point_counts"][b], info["point_counts"], err_msg=f"frame {b}")
        assert tap["round_used"][b] == info["round_used"], b
        assert gp.dtype == np.float32 and gp.shape == pts.shape, (b, gp.shape, pts.shape)
        assert gp.tobytes() == pts.tobytes(), f"frame {b}: cloud not bit-identical"
        np.testing.assert_array_equal(gb, bx.astype(np.float32))
        np.testing.assert_array_equal(gc, cl)
        np.testing.assert_array_equal(gv, va)
    print(f"points within 1e-9 m of a candidate face: {near}; box pairs within 1e-9 m of touching: {touching} "
          "(nothing is excluded from comparison; both expected 0)")
    assert near == 0 and touching == 0
    return got, tap


def test_fixture_cases_in_one_batch(pp, hip_lib):
    G = load_golden("ref_gt_sample.npz")
    gts = pp.gt_sampler
    names = [str(n) for n in G["names"]]
    db = fixture_db(pp)
    eng = pp.Engine(_cfg(pp, len(names), num_class=2), max_batch=len(names), max_points_per_frame=8192)
    eng.load_gt_database(db)
    # one batch per (max, min) point-collision setting: the thresholds are per call
    groups = {}
    for c in names:
        groups.setdefault(tuple(int(v) for v in G[f"case__{c}__cfg"]), []).append(c)
    assert len(groups) == 2
    for cs in groups.values():
        frames = [G["frame__" + str(G[f"case__{c}__frame"])] for c in cs]
        gt = [G[f"case__{c}__gt_boxes"].astype(np.float32) for c in cs]
        for c, g in zip(cs, gt):
            assert np.array_equal(g.astype(np.float64), G[f"case__{c}__gt_boxes"])      # float32-representable
        classes = [G[f"case__{c}__gt_classes"] for c in cs]
        cand = gts.Candidates(np.stack([G[f"case__{c}__cands"] for c in cs]), np.stack([G[f"case__{c}__cand_counts"] for c in cs]))
        got, tap = _compare(pp, eng, db, frames, gt, classes, None, cand, case_cfg(pp, cs[0]))
        for b, c in enumerate(cs):                                                        # and against the reference itself
            pre = f"case__{c}__"
            want = np.concatenate([G[pre + "pasted"], frames[b]], 0)
            assert got[b][0].tobytes() == want.tobytes(), c
            np.testing.assert_array_equal(got[b][1], np.concatenate([G[pre + "gt_boxes"], G[pre + "ret_boxes"]], 0).astype(np.float32))
            np.testing.assert_array_equal(got[b][2], np.concatenate([G[pre + "gt_classes"], G[pre + "ret_classes"]]))
            np.testing.assert_array_equal(tap["status"][b], G[pre + "status"])
            np.testing.assert_array_equal(tap["point_counts"][b], G[pre + "point_counts"])
    eng.close()


def _random_batch(pp, rng, db, B, F, n_pts, span):
    """Frames of n_pts points over `span` (x0, x1, y0, y1), 0-6 boxes each with random valid flags."""
    frames, gt, classes, valids = [], [], [], []
    for b in range(B):
        n = int(rng.integers(n_pts // 2, n_pts))
        p = np.stack([rng.uniform(span[0], span[1], n), rng.uniform(span[2], span[3], n), rng.uniform(-1.4, 1.4, n)] +
                     [rng.uniform(0, 1, n)] * (F - 3), 1).astype(np.float32)
        frames.append(p)
        g = int(rng.integers(0, 7))
        bx = np.stack([rng.uniform(0.4, 6.0, g), rng.uniform(-2.2, 2.2, g), rng.uniform(-0.9, -0.5, g), rng.uniform(0.5, 0.7, g),
                       rng.uniform(0.7, 0.9, g), rng.uniform(1.5, 1.8, g), rng.uniform(-3.1, 3.1, g)], 1).astype(np.float32)
        gt.append(bx)
        classes.append(np.ones(g, np.int32))
        valids.append(rng.uniform(size=g) < 0.7)
    return frames, gt, classes, valids


@pytest.mark.parametrize("seed", [11, 12])
def test_random_batches_cfg_a(pp, hip_lib, seed):
    gts = pp.gt_sampler
    B = 32
    db = _ped_db(pp)
    eng = pp.Engine(_cfg(pp, B), max_batch=B, max_points_per_frame=8192)
    eng.load_gt_database(db)
    rng = np.random.default_rng(seed)
    frames, gt, classes, valids = _random_batch(pp, rng, db, B, 3, 6000, (0.05, 6.35, -2.5, 2.5))
    cand = gts.draw_candidates(db, classes, random.Random(seed))
    got, tap = _compare(pp, eng, db, frames, gt, classes, valids, cand, db.config)
    st = tap["status"]
    assert (st == gts.ACCEPTED).any() and (st == gts.BOX_COLLISION).any()
    eng.close()


def test_cfg_k_shaped_four_features(pp, hip_lib):
    gts = pp.gt_sampler
    B = 8
    cfg = pp.config.kitti_shaped_config(B)
    F = pp.config.Derived(cfg).num_point_features
    assert F == 4
    db = _ped_db(pp, F=4)
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=32768)
    eng.load_gt_database(db)
    rng = np.random.default_rng(21)
    frames, gt, classes, valids = _random_batch(pp, rng, db, B, 4, 20000, (0.05, 12.0, -5.0, 5.0))
    cand = gts.draw_candidates(db, classes, random.Random(21))
    got, _ = _compare(pp, eng, db, frames, gt, classes, valids, cand, db.config)
    pasted = [len(g[0]) - len(f) for g, f in zip(got, frames)]
    assert max(pasted) > 0
    b = int(np.argmax(pasted))
    assert np.any(got[b][0][:pasted[b], 3] != 0)            # the fourth feature rides along
    eng.close()


def test_frames_without_boxes(pp, hip_lib):
    gts = pp.gt_sampler
    db = fixture_db(pp)
    G = load_golden("ref_gt_sample.npz")
    frame = G["frame__full"]
    empty = [i for i in range(len(db)) if db.offsets[i + 1] == db.offsets[i]]
    full = [i for i in range(len(db)) if db.offsets[i + 1] > db.offsets[i] and db.classes[i] == 1]
    cands = np.zeros((3, gts.PP_GTS_MAX_CAND), gts.CAND_DTYPE)
    cands["object"][0, :3] = [empty[0], empty[0], full[0]]         # succeeds in its third round
    cands["object"][1, :2] = [empty[0], empty[1]]                  # every round fails
    cands["object"][2, :3] = [full[1], full[2], full[3]]           # has a box: the first round only
    counts = np.array([[1, 1, 1, 0], [1, 1, 0, 0], [1, 1, 1, 0]], np.int32)
    cand = gts.Candidates(cands, counts)
    gt = [np.zeros((0, 7), np.float32), np.zeros((0, 7), np.float32), G["case__shipped__gt_boxes"][:1].astype(np.float32)]
    eng = pp.Engine(_cfg(pp, 3, num_class=2), max_batch=3, max_points_per_frame=8192)
    eng.load_gt_database(db)
    got, tap = _compare(pp, eng, db, [frame] * 3, gt, None, None, cand, db.config)
    assert tap["round_used"].tolist()[:2] == [2, -1]
    assert tap["status"][0, :3].tolist() == [gts.EMPTY_OBJECT, gts.EMPTY_OBJECT, gts.ACCEPTED]
    assert got[1][0].tobytes() == frame.tobytes() and len(got[1][1]) == 0     # unchanged
    failed = int(sum(len(g) == 0 and r < 0 for g, r in zip(gt, tap["round_used"])))
    assert failed == 1
    assert tap["status"][2, 1:3].tolist() == [gts.ROUND_NOT_USED] * 2
    eng.close()


def test_runs_and_feeds_identical(pp, hip_lib):
    gts = pp.gt_sampler
    B = 4
    db = _ped_db(pp)
    eng = pp.Engine(_cfg(pp, B), max_batch=B, max_points_per_frame=8192)
    eng.load_gt_database(db)
    rng = np.random.default_rng(31)
    frames, gt, classes, valids = _random_batch(pp, rng, db, B, 3, 5000, (0.05, 6.35, -2.5, 2.5))
    cand = gts.draw_candidates(db, classes, random.Random(31))

    def flat(out, tap):
        return [a.tobytes() for o in out for a in o] + [tap[k].tobytes() for k in ("status", "point_counts", "round_used")]

    eng.upload(frames)
    first = flat(eng.gt_sample(gt, classes, valids, cand), eng.gt_sample_info())
    eng.upload(frames)
    assert flat(eng.gt_sample(gt, classes, valids, cand), eng.gt_sample_info()) == first          # integer atomics
    st = eng.staging(frames)                                                                      # zero-copy (<= 4 frames)
    eng.upload_async(st)
    assert flat(eng.gt_sample(gt, classes, valids, cand), eng.gt_sample_info()) == first
    import torch
    pts, offs = eng._pack(frames, 3)
    dev = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()
    eng.upload_device(dev.data_ptr(), offs)
    assert flat(eng.gt_sample(gt, classes, valids, cand), eng.gt_sample_info()) == first
    eng.close()


def test_augmentation_and_detection_follow_the_grown_frames(pp, hip_lib):
    """What runs after the sampling sizes itself from the grown frames: pp_augment on them equals the host's
    augmentation of the host's sampled frames, and a detection pass voxelises every pasted point."""
    gts = pp.gt_sampler
    B = 4
    db = _ped_db(pp)
    eng = pp.Engine(_cfg(pp, B), max_batch=B, max_points_per_frame=8192)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    eng.load_gt_database(db)
    rng = np.random.default_rng(41)
    frames, gt, classes, valids = _random_batch(pp, rng, db, B, 3, 3000, (0.05, 6.35, -2.5, 2.5))
    frames[1] = frames[1][:500]                       # the largest frame after pasting is not the largest before
    cand = gts.draw_candidates(db, classes, random.Random(41))
    eng.upload(frames)
    got = eng.gt_sample(gt, classes, valids, cand)
    assert any(len(g[0]) > len(f) for g, f in zip(got, frames))
    acfg = pp.augment.AugmentConfig.from_input_reader(None)
    boxes2, cls2, val2 = [g[1] for g in got], [g[2] for g in got], [g[3] for g in got]
    draws = pp.augment.draw(np.random.RandomState(2), boxes2, acfg)
    out = eng.augment(boxes2, cls2, val2, draws, acfg)
    pc = np.asarray(eng.d.pc_range, np.float64)
    for b in range(B):
        pts, bx, cl = pp.augment.augment_np(got[b][0], boxes2[b], cls2[b], val2[b], draws.frame(b), acfg, pc)
        assert out[b][0].shape == pts.shape
        want = pts.astype(np.float32)
        sp = np.spacing(np.maximum(np.abs(out[b][0]), np.abs(want)))
        assert (np.abs(out[b][0].astype(np.float64) - want) <= sp).all()
        assert len(out[b][1]) == len(bx)
        np.testing.assert_array_equal(out[b][2], cl)
    # a pass over sampled frames sees the pasted points: the pillar counts equal those of the same clouds uploaded whole
    eng.upload(frames)
    got = eng.gt_sample(gt, classes, valids, cand)
    rect, trv, _ = pp.synth.default_calib()
    eng.set_calib(np.stack([rect] * B), np.stack([trv] * B), B)
    eng.detect_async()
    eng.sync()
    n1 = eng.intermediates()["n_pillars"].copy()
    eng.upload([g[0] for g in got], np.stack([rect] * B), np.stack([trv] * B))
    eng.detect_async()
    eng.sync()
    np.testing.assert_array_equal(n1, eng.intermediates()["n_pillars"])
    eng.close()


def test_refusals_leave_the_handle_usable(pp, hip_lib):
    gts = pp.gt_sampler
    B = 2
    eng = pp.Engine(_cfg(pp, B), max_batch=B, max_points_per_frame=2048)
    rng = np.random.default_rng(51)
    db = _ped_db(pp)
    frames, gt, classes, valids = _random_batch(pp, rng, db, B, 3, 1500, (0.05, 6.35, -2.5, 2.5))
    gt = [g[:1] for g in gt]
    classes = [np.ones(len(g), np.int32) for g in gt]
    cand = gts.draw_candidates(db, classes, random.Random(51))
    eng.upload(frames)
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*no database"):
        eng.gt_sample(gt, classes, None, cand, db.config)
    with pytest.raises(ValueError, match="point features"):
        eng.load_gt_database(_ped_db(pp, F=4))
    two = fixture_db(pp)
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*class 2"):
        eng.load_gt_database(two)                                        # a one-class engine
    eng.load_gt_database(db)
    bad = gts.Candidates(cand.cands.copy(), cand.counts.copy())
    bad.cands["object"][0, 0] = len(db)
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*outside the database"):
        eng.gt_sample(gt, classes, None, bad)
    bad = gts.Candidates(cand.cands.copy(), cand.counts.copy())
    bad.counts[0] = [20, 20, 0, 0]
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*more than 32 candidates"):
        eng.gt_sample(gt, classes, None, bad)
    bad = gts.Candidates(cand.cands.copy(), cand.counts.copy())
    bad.cands["group"][0, 0] = 3
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*groups out of order"):
        eng.gt_sample(gt, classes, None, bad)
    # the bound on the pasted cloud: 32 of the largest object on a frame of ~2 000 points
    big = int(np.argmax(np.diff(db.offsets)))
    bad = gts.Candidates(np.zeros_like(cand.cands), np.zeros_like(cand.counts))
    bad.cands["object"][:] = big
    bad.counts[:, 0] = 32
    frames2 = [np.concatenate([f, f])[:2048 - 40] for f in frames]
    eng.upload(frames2)
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*max_points_per_frame"):
        eng.gt_sample(gt, classes, None, bad)
    many = [np.repeat(g[:1], 250, 0) for g in gt]
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*candidates > 256"):
        eng.gt_sample(many, None, None, cand)
    with pytest.raises(RuntimeError, match="PP_ERR_ARG.*frames are resident"):
        eng.gt_sample(gt[:1], classes[:1], None, gts.Candidates(cand.cands[:1], cand.counts[:1]))
    # usable afterwards
    eng.upload(frames)
    _compare(pp, eng, db, frames, gt, classes, None, cand, db.config)
    eng.close()


# ---- the sampled training step ----

def _trainer(pp, cfg, B, **kw):
    return pp.Trainer(cfg, pp.weights.init_weights(pp.config.Derived(cfg), seed=7), max_batch=B, max_points_per_frame=16384,
                      learning_rate=2e-4, weight_decay=1e-4, **kw)


def _problem(pp, B, two_class, seed=3):
    rng = np.random.default_rng(seed)
    if two_class:
        cfg = pp.config.kitti_shaped_config(B, num_class=2)
        frames = [pp.synth.kitti_cloud(600 + seed * 10 + i, 8000) for i in range(B)]
        lo, hi, G = (4.0, -20.0), (40.0, 20.0), 3
    else:
        cfg = pp.config.pedestrian_d435i_config(B)
        frames = [pp.synth.d435i_cloud(500 + seed * 10 + i, 6000) for i in range(B)]
        lo, hi, G = (1.0, -1.5), (5.5, 1.5), 2
    gt, cls = [], []
    for b in range(B):
        g = np.concatenate([rng.uniform(lo[0], hi[0], (G, 1)), rng.uniform(lo[1], hi[1], (G, 1)), np.full((G, 1), -0.9),
                            np.full((G, 1), 0.6), np.full((G, 1), 0.8), np.full((G, 1), 1.73),
                            rng.uniform(-np.pi, np.pi, (G, 1))], 1).astype(np.float32)
        gt.append(g)
        cls.append(np.arange(G, dtype=np.int32) % 2 + 1 if two_class else np.ones(G, np.int32))
    return cfg, cls, frames, gt


@pytest.mark.parametrize("augment,two_class,staged,flags", [
    (True, False, True, False), (True, False, False, False), (False, False, True, False), (True, True, True, False),
    (False, True, False, False),
    (True, False, True, True), (True, False, False, True), (False, False, True, True), (False, False, False, True),
    (True, True, False, True)])
def test_fused_step_equals_sample_augment_gt_step(pp, hip_lib, augment, two_class, staged, flags):
    """pp_train_step_sample against pp_gt_sample -> pp_augment -> pp_train_step_gt on each other's outputs: the same
    losses and the same bits in every gradient and statistic, over 4 steps; graph captures constant once both input
    buffers' graphs exist.  flags: some frame boxes are invalid (gt_valid), the same flags on both sides."""
    B = 2
    cfg, cls, frames, gt = _problem(pp, B, two_class)
    val = [np.arange(len(g)) % 2 == b % 2 for b, g in enumerate(gt)] if flags else None
    assert val is None or any((~v).any() for v in val)
    F = pp.config.Derived(cfg).num_point_features
    dbs = [fixture_db(pp, F) if two_class else _ped_db(pp, F) for _ in range(2)]      # two cursors in the same state
    acfg = pp.augment.AugmentConfig.from_input_reader({}) if augment else None
    ta = _trainer(pp, cfg, B, augment=acfg, seed=11, gt_database=dbs[0], sampler=dbs[0].config)
    tb = _trainer(pp, cfg, B, augment=acfg, seed=11, gt_database=dbs[1], sampler=dbs[1].config)   # driven by hand
    rev = (lambda x: None if x is None else x[::-1])  # noqa: E731
    batches = [ta.stage_gt(frames, gt, cls, gt_valid=val), ta.stage_gt(rev(frames), rev(gt), rev(cls), gt_valid=rev(val))] \
        if staged else None
    accepted, pasted_cls = 0, set()
    for i in range(4):
        fr, g, gc, gv = (frames, gt, cls, val) if i % 2 == 0 else (rev(frames), rev(gt), rev(cls), rev(val))
        if staged:
            a = ta.forward_backward(batches[i % 2], prefetch=batches[(i + 1) % 2])
            cand = batches[i % 2].cand
            draws = batches[i % 2].aug[1] if augment else None
        else:
            a = ta.forward_backward(fr, gt_boxes=g, gt_classes=gc, gt_valid=gv)
            cand = tb._draw_candidates(g, gc)
            draws = tb._draw_augment(g, cand) if augment else None
        eng = tb.engine
        eng.upload(fr)
        out = eng.gt_sample(g, gc, gv, cand)
        accepted += sum(len(o[1]) for o in out) - sum(len(x) for x in g)
        for o, x in zip(out, g):
            pasted_cls |= set(o[2][len(x):].tolist())
            if flags:
                assert not o[3][:len(x)].all() and o[3][len(x):].all()     # the flags came through; pasted objects are valid
        boxes, classes = [o[1] for o in out], [o[2] for o in out]
        if augment:
            rows = np.array([len(x) for x in g]) + cand.counts.max(axis=1)
            start = np.concatenate([[0], np.cumsum(rows)])
            used = np.concatenate([draws.boxes[start[b]:start[b] + len(boxes[b])] for b in range(B)], 0)
            d2 = pp.augment.Draws(draws.flip, draws.theta, draws.scale, draws.t, draws.seed, used, [len(x) for x in boxes])
            n_in = sum(len(x) for x in boxes)
            out = eng.augment(boxes, classes, [o[3] for o in out], d2, acfg)
            boxes, classes = [o[1] for o in out], [o[2] for o in out]
            if flags:
                assert sum(len(x) for x in boxes) < n_in                   # the augmentation drops the invalid boxes
        kb, kc, kn = eng.pack_gt(boxes, classes)
        eng.train_step_gt_async(tb.params.data_ptr(), tb.grads.data_ptr(), tb.state.data_ptr(), kb, kc, kn)
        b = eng.train_step_wait()
        assert a == b, (i, a, b)
        assert np.array_equal(ta.grads.cpu().numpy(), tb.grads.cpu().numpy()), i
        assert np.array_equal(ta.state.cpu().numpy(), tb.state.cpu().numpy()), i
        if i == 1:      # a graph per input buffer: both captured by now
            c0, r0 = ta.engine.train_graph_stats()
    c1, r1 = ta.engine.train_graph_stats()
    assert c1 == c0 and r1 == r0 + 2, (c0, r0, c1, r1)
    print(f"objects pasted over 4 steps: {accepted}, classes {sorted(pasted_cls)}")
    assert accepted > 0
    assert pasted_cls == ({1, 2} if two_class else {1})
    # the handle knows the sampled frames' sizes on the device only: the synchronous calls say so until the next upload
    if not staged:                               # (a staged run has prefetched -- uploaded -- the next batch already)
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*sampled inside a training step"):
            ta.engine.gt_sample(g, gc, None, cand)
        if augment:
            with pytest.raises(RuntimeError, match="PP_ERR_STATE.*sampled training step"):
                ta.engine.augment_selected()
    for s_ in batches or []:
        s_.close()
    ta.close()
    tb.close()


def _empty_db(pp, n=24):
    """Objects without points: every candidate fails the point test, so a frame without boxes fails all its rounds."""
    gts = pp.gt_sampler
    full = fixture_db(pp)
    infos = {"Pedestrian": [{"box3d_lidar": full.boxes[i], "difficulty": 0, "num_points_in_gt": 0} for i in range(n)]}
    points = {"Pedestrian": [np.zeros((0, 3), np.float32) for _ in range(n)]}
    cfg = gts.SamplerConfig.from_input_reader({"sample_classes": ["Pedestrian"], "sample_max_nums": [8]})
    return gts.GtDatabase(infos, points, cfg, np.random.RandomState(5), random.Random(5), 3)


@pytest.mark.parametrize("staged", [False, True])
def test_trainer_counts_frames_left_without_boxes(pp, hip_lib, staged):
    """Exact count, per step: with a database of empty objects every frame that comes without boxes stays without.
    The staged route alternates a 2-frame and a 1-frame batch, the next one prefetched while the step runs."""
    cfg, cls, frames, gt = _problem(pp, 2, False)
    none = np.zeros((0, 7), np.float32)
    batches = [(frames, [none, gt[1]]), (frames[:1], [none]), (frames, [gt[0], gt[1]]), (frames, [none, none])]
    boxless = [1, 1, 0, 2]
    t = _trainer(pp, cfg, 2, gt_database=_empty_db(pp), sampler=True, seed=3)
    st = [t.stage_gt(f, g) for f, g in batches] if staged else None
    want = 0
    for rnd in range(2):
        for k, (f, g) in enumerate(batches):
            if staged:
                losses = t.step(st[k], prefetch=st[(k + 1) % len(st)])
            else:
                losses = t.step(f, gt_boxes=g)
            assert np.isfinite(losses["loss"])
            want += boxless[k]
            assert t.frames_left_without_boxes == want, (rnd, k, t.frames_left_without_boxes, want)
            info = t.engine.gt_sample_info()
            assert info["round_used"].shape == (len(f),) and (info["round_used"] < 0).all()
    assert want == 8
    for s_ in st or []:
        s_.close()
    t.close()
    # and a database whose objects have points leaves none behind on these clouds
    db = _ped_db(pp)
    t = _trainer(pp, cfg, 2, gt_database=db, sampler=db.config, seed=3)
    t.step(frames, gt_boxes=[none, none])
    used = t.engine.gt_sample_info()["round_used"]
    assert t.frames_left_without_boxes == int((used < 0).sum())
    assert (used >= 0).any()
    t.close()


def test_per_object_global_rotation_is_refused_with_sampling(pp, hip_lib):
    cfg, cls, frames, gt = _problem(pp, 2, False)
    db = _ped_db(pp)
    grot = pp.augment.AugmentConfig.from_input_reader({"global_random_rotation_range_per_object": [-0.4, 0.4]})
    assert grot.global_rot_per_object
    with pytest.raises(ValueError, match="global_random_rotation_range_per_object"):
        _trainer(pp, cfg, 2, augment=grot, gt_database=db, sampler=db.config)
    # the C-ABI says the same, and the handle trains on afterwards
    acfg = pp.augment.AugmentConfig.from_input_reader({})
    t = _trainer(pp, cfg, 2, augment=acfg, seed=1, gt_database=db, sampler=db.config)
    cand = t._draw_candidates(gt, cls)
    draws = t._draw_augment(gt, cand)
    kb, kc, kn = t.engine.pack_gt(gt, cls)
    t.engine.upload(frames)
    with pytest.raises(RuntimeError, match="PP_ERR_UNSUPPORTED.*global_random_rotation_range_per_object"):
        t.engine.train_step_sample_async(t.params.data_ptr(), t.grads.data_ptr(), t.state.data_ptr(), kb, kc, kn, None,
                                         cand, db.config, draws, grot)
    # gt_valid is checked against the boxes, the draws against their rows
    with pytest.raises(ValueError, match="gt_valid: 1 flags for 4 boxes"):
        t.engine.train_step_sample_async(t.params.data_ptr(), t.grads.data_ptr(), t.state.data_ptr(), kb, kc, kn,
                                         np.ones(1, np.uint8), cand, db.config, draws, acfg)
    assert np.isfinite(t.step(frames, gt_boxes=gt, gt_valid=[np.array([True, False])] * 2)["loss"])
    t.close()


def test_trainer_refusals(pp, hip_lib):
    cfg = pp.config.pedestrian_d435i_config(1)
    w = pp.weights.init_weights(pp.config.Derived(cfg), seed=7)
    db = _ped_db(pp)
    with pytest.raises(ValueError, match="go together"):
        pp.Trainer(cfg, w, max_batch=1, sampler=True)
    with pytest.raises(ValueError, match="go together"):
        pp.Trainer(cfg, w, max_batch=1, gt_database=db)
    with pytest.raises(ValueError, match="SamplerConfig"):
        pp.Trainer(cfg, w, max_batch=1, gt_database=db, sampler={"sample_classes": ["Pedestrian"]})
    t = pp.Trainer(cfg, w, max_batch=1, max_points_per_frame=8192, gt_database=db, sampler=True)
    A = t.engine.d.num_anchors
    with pytest.raises(ValueError, match="gt_boxes"):
        t.step([pp.synth.d435i_cloud(1, 2000)], np.zeros((1, A), np.int32), np.zeros((1, A, 7), np.float32))
    t.close()
