"""Training targets assigned on the GPU from ground-truth boxes (csrc/targets.hip: pp_assign_targets,
pp_train_step_gt*) against the reference's own create_target_np (ref_targets.npz) and the host pipeline
(engine voxeliser -> anchor mask -> target_assigner.assign), and the training step fed that way."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_TA = {"sample_positive_fraction": "None", "rpn_batch_size": 512}
CASES = [(n, m) for n in ("three", "offgrid", "empty", "tie") for m in (False, True)]


def _golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "ref_targets.npz")) as z:
        return {k: z[k] for k in z.files}


def _same_targets(got, want, what, log_ulp=1):
    """Bit-identical, except the three log columns of the regression targets: within `log_ulp` float32 ulp (the GPU
    rounds log once from float64; numpy's float32 log is not correctly rounded)."""
    for k in ("labels", "positive_gt_id", "assigned_anchors_inds", "bbox_outside_weights"):
        assert got[k].dtype == want[k].dtype, (what, k, got[k].dtype, want[k].dtype)
        assert np.array_equal(got[k], want[k]), (what, k)
    if want["assigned_anchors_overlap"] is None:
        assert got["assigned_anchors_overlap"] is None, what
    else:
        assert got["assigned_anchors_overlap"] is not None, what
        assert got["assigned_anchors_overlap"].dtype == want["assigned_anchors_overlap"].dtype, what
        assert np.array_equal(got["assigned_anchors_overlap"], want["assigned_anchors_overlap"]), what
    g, w = got["bbox_targets"], want["bbox_targets"]
    assert g.dtype == w.dtype == np.float32 and g.shape == w.shape, what
    exact = [0, 1, 2, 6]
    assert np.array_equal(g[:, exact], w[:, exact]), what
    np.testing.assert_array_max_ulp(g[:, 3:6], w[:, 3:6], maxulp=log_ulp)


def test_reference_fixture_bit_exact(pp, hip_lib):
    """All 8 cases of the reference's create_target_np outputs in one batch of 8 frames on a cfg-A engine."""
    G = _golden()
    eng = pp.Engine(pp.config.pedestrian_d435i_config(8), max_batch=8, max_points_per_frame=4096)
    assert np.array_equal(eng.anchors, G["anchors"]), "the fixture's anchors are the engine's own grid"
    A = eng.anchors.shape[0]
    gts = [G[f"{n}_{'mask' if m else 'all'}_gt"] for n, m in CASES]
    masks = np.stack([G[f"{n}_mask_anchors_mask"] if m else np.ones(A, bool) for n, m in CASES])
    got = eng.assign_targets(gts, anchors_mask=masks)
    assert len(got) == 8
    for (n, m), r in zip(CASES, got):
        tag = f"{n}_{'mask' if m else 'all'}"
        want = {k: G[f"{tag}_{k}"] for k in ("labels", "bbox_targets", "bbox_outside_weights", "positive_gt_id",
                                             "assigned_anchors_inds", "assigned_anchors_overlap")}
        if bool(G[tag + "_overlap_is_none"]):
            want["assigned_anchors_overlap"] = None
        _same_targets(r, want, tag)
    assert (got[0]["labels"] > 0).sum() == 103
    eng.close()


def _boxes(rng, d, G, num_class, sizes):
    """G random boxes over (and a little beyond) the point-cloud range, rotations at and one ulp beside +-pi/4,
    duplicated boxes (ties), classes 1..num_class."""
    lo, hi = np.array(d.pc_range[:3]), np.array(d.pc_range[3:])
    span = hi - lo
    xy = rng.uniform(lo[:2] - 0.05 * span[:2], hi[:2] + 0.05 * span[:2], (G, 2))
    z = rng.uniform(-1.5, -0.5, (G, 1))
    wlh = np.stack([rng.uniform(0.3, 1.0, G) * sizes[0], rng.uniform(0.5, 1.2, G) * sizes[1],
                    rng.uniform(0.8, 1.2, G) * sizes[2]], axis=1)
    r = rng.uniform(-np.pi, np.pi, (G, 1))
    b = np.concatenate([xy, z, wlh, r], axis=1).astype(np.float32)
    q = np.float32(np.pi / 4)
    special = np.array([q, -q, np.nextafter(q, np.float32(1)), np.nextafter(q, np.float32(0)),
                        np.nextafter(-q, np.float32(-1)), np.nextafter(-q, np.float32(0)),
                        np.float32(3 * np.pi / 4), np.float32(np.pi / 2)], np.float32)
    k = min(G, len(special))
    b[:k, 6] = special[:k]
    if G >= 4:
        b[G - 1] = b[G - 2]          # a duplicated box: two boxes tie for every anchor
        b[1, :2] = b[0, :2]          # same centre, different rotation / size
    cls = rng.integers(1, num_class + 1, G).astype(np.int32)
    return b, cls


def _blob_boxes(rng, frame, G, sizes):
    """Boxes centred on points of the cloud (positives guaranteed)."""
    idx = rng.choice(len(frame), G, replace=False)
    c = frame[idx, :3].astype(np.float64)
    wlh = np.stack([rng.uniform(0.5, 1.1, G) * sizes[0], rng.uniform(0.5, 1.1, G) * sizes[1],
                    rng.uniform(0.9, 1.1, G) * sizes[2]], axis=1)
    r = rng.uniform(-np.pi, np.pi, (G, 1))
    return np.concatenate([c, wlh, r], axis=1).astype(np.float32)


def _host_targets(pp, eng, frame, gt, cls):
    """The host pipeline: engine voxeliser -> anchor mask -> target_assigner.assign."""
    _, coors, _ = eng.points_to_voxel(frame)
    coors4 = np.concatenate([np.zeros((len(coors), 1), np.int32), coors], axis=1)
    mask = eng.anchor_mask(coors4, 1)[0].astype(bool)
    return pp.target_assigner.assign(eng.anchors, gt, mask, cls, 0.5, 0.35, CFG_TA), mask


@pytest.mark.parametrize("which", ["cfg-A", "cfg-K"])
def test_resident_frames_match_host_pipeline(pp, hip_lib, which):
    B = 8
    rng = np.random.default_rng(21 if which == "cfg-A" else 22)
    if which == "cfg-A":
        cfg, ncls = pp.config.pedestrian_d435i_config(B), 1
        frames = [pp.synth.d435i_cloud(700 + i, 8192) for i in range(B)]
        counts = [0, 256, 1, 5, 16, 3, 40, 8]
        sizes = (0.6, 0.8, 1.73)
    else:
        cfg, ncls = pp.config.kitti_shaped_config(B, num_class=2), 2
        frames = [pp.synth.kitti_cloud(800 + i, 16384) for i in range(B)]
        counts = [4, 0, 64, 16, 1, 8, 32, 12]
        sizes = (1.6, 3.9, 1.56)
    d = pp.config.Derived(cfg)
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=20000)
    gts, classes = [], []
    for b, G in enumerate(counts):
        g, c = _boxes(rng, d, G, ncls, sizes)
        if G >= 8:               # a share of the boxes on the cloud itself, so that anchors are matched
            g[G // 2:G // 2 + G // 4] = _blob_boxes(rng, frames[b], G // 4, sizes)
        gts.append(g)
        classes.append(c)
    host = [_host_targets(pp, eng, frames[b], gts[b], classes[b]) for b in range(B)]
    eng.upload(frames)
    got = eng.assign_targets(gts, classes)
    npos = 0
    for b in range(B):
        want, mask = host[b]
        # numpy's SIMD float32 log is up to 3 ulp from the correctly rounded value (measured on 2 M ratios): the log
        # columns are checked exactly against float64 log rounded once, and loosely against the host's own
        _same_targets(got[b], want, f"{which} frame {b}", log_ulp=4)
        pos = want["assigned_anchors_inds"]
        ratio = gts[b][want["positive_gt_id"], 3:6] / eng.anchors[pos, 3:6]
        exact = np.log(ratio.astype(np.float64)).astype(np.float32)
        assert np.array_equal(got[b]["bbox_targets"][pos, 3:6], exact), (which, b)
        assert (got[b]["labels"][~mask] == -1).all()
        npos += int((want["labels"] > 0).sum())
    assert npos > 20, npos
    assert {int(c) for b in range(B) for c in got[b]["labels"][got[b]["labels"] > 0]} <= set(range(1, ncls + 1))
    # the same frames with the masks passed in: the same targets
    again = eng.assign_targets(gts, classes, anchors_mask=np.stack([h[1] for h in host]))
    for b in range(B):
        _same_targets(again[b], got[b], f"{which} frame {b}, mask passed")
    eng.close()


def _step_problem(pp, B=2, seed=31):
    cfg = pp.config.pedestrian_d435i_config(B)
    d = pp.config.Derived(cfg)
    rng = np.random.default_rng(seed)
    frames = [pp.synth.d435i_cloud(900 + seed + i, 8192) for i in range(B)]
    gts = []
    for b in range(B):
        g, _ = _boxes(rng, d, 6, 1, (0.6, 0.8, 1.73))
        g[:3] = _blob_boxes(rng, frames[b], 3, (0.6, 0.8, 1.73))
        gts.append(g)
    return cfg, d, frames, gts


def _trainer(pp, cfg, d, B):
    return pp.Trainer(cfg, pp.weights.init_weights(d, seed=7), max_batch=B, max_points_per_frame=8192,
                      learning_rate=2e-4, weight_decay=1e-4)


@pytest.mark.parametrize("profiled", [False, True])
def test_gt_step_equals_dense_step(pp, hip_lib, profiled):
    """Trainer.step(gt_boxes=...) and Trainer.step(labels, reg_targets) with the targets Engine.assign_targets returned
    for the same frames: the same bits for 3 optimizer steps (graph replays; profiled: the eager path)."""
    B = 2
    cfg, d, frames, gts = _step_problem(pp, B)
    ta, tb = _trainer(pp, cfg, d, B), _trainer(pp, cfg, d, B)
    tb.engine.upload(frames)
    res = tb.engine.assign_targets(gts)
    labels = np.stack([r["labels"] for r in res])
    reg = np.stack([r["bbox_targets"] for r in res])
    assert (labels > 0).sum() > 0
    if profiled:
        ta.engine.set_profiling(True)
        tb.engine.set_profiling(True)
    for i in range(3):
        a = ta.step(frames, gt_boxes=gts)
        b = tb.step(frames, labels, reg)
        assert a == b, (i, a, b)
        assert a["num_positives"] == int((labels > 0).sum())
        assert np.array_equal(ta.grads.cpu().numpy(), tb.grads.cpu().numpy()), i
        assert np.array_equal(ta.params.cpu().numpy(), tb.params.cpu().numpy()), i
        assert np.array_equal(ta.state.cpu().numpy(), tb.state.cpu().numpy()), i
    if profiled:
        names = {n.split(":")[0] for n, _ in ta.engine.kernel_times()}
        assert {"k_tgt_top", "k_tgt_assign"} <= names, names
    else:
        ca, ra = ta.engine.train_graph_stats()
        assert ca <= 2 and ra == 3, (ca, ra)
    ta.close()
    tb.close()


def test_staged_prefetched_gt_batches(pp, hip_lib):
    """Two stage_gt batches taking turns with prefetch= for 4 steps: the parameters of 4 unstaged gt steps, replays."""
    B = 2
    cfg, d, frames, gts = _step_problem(pp, B, seed=41)
    frames2, gts2 = frames[::-1], gts[::-1]
    cls = [np.ones(len(g), np.int32) for g in gts]
    ta, tb = _trainer(pp, cfg, d, B), _trainer(pp, cfg, d, B)
    staged = [ta.stage_gt(frames, gts, cls), ta.stage_gt(frames2, gts2)]
    for i in range(4):
        ta.step(staged[i % 2], prefetch=staged[(i + 1) % 2])
    for i in range(4):
        tb.step(frames if i % 2 == 0 else frames2, gt_boxes=gts if i % 2 == 0 else gts2)
    assert np.array_equal(ta.params.cpu().numpy(), tb.params.cpu().numpy())
    assert np.array_equal(ta.state.cpu().numpy(), tb.state.cpu().numpy())
    captures, replays = ta.engine.train_graph_stats()
    assert captures <= 2 and replays == 4, (captures, replays)
    for s in staged:
        s.close()
    ta.close()
    tb.close()


def test_bad_boxes_are_refused_and_the_handle_stays_usable(pp, hip_lib):
    B = 2
    cfg, d, frames, gts = _step_problem(pp, B, seed=51)
    tr = _trainer(pp, cfg, d, B)
    eng = tr.engine
    eng.upload(frames)
    ref = eng.assign_targets(gts)
    many = [np.tile(gts[0][:1], (257, 1)), gts[1]]
    zero_w = [gts[0].copy(), gts[1]]
    zero_w[0][2, 3] = 0.0
    nan = [gts[0].copy(), gts[1]]
    nan[0][1, 0] = np.nan
    bad = [(many, None, "PP_ERR_ARG"), (zero_w, None, "PP_ERR_ARG"), (nan, None, "PP_ERR_ARG"),
           (gts, [np.full(len(g), 3, np.int32) for g in gts], "PP_ERR_ARG"), (gts[:1], None, "PP_ERR_STATE")]
    for boxes, cls, status in bad:
        with pytest.raises(RuntimeError, match=status):
            eng.assign_targets(boxes, cls)
        if len(boxes) == B:
            with pytest.raises(RuntimeError, match=status):
                tr.step(frames, gt_boxes=boxes, gt_classes=cls)
        for r, w in zip(eng.assign_targets(gts), ref):      # (tr.step uploaded the same frames)
            assert np.array_equal(r["labels"], w["labels"])
    # a batch that differs from the resident frames, in the step
    with pytest.raises(RuntimeError, match="PP_ERR_STATE"):
        eng.train_step_gt_async(tr.params.data_ptr(), tr.grads.data_ptr(), tr.state.data_ptr(),
                                *eng.pack_gt(gts[:1]))
    # numeric sample_positive_fraction: refused before anything reaches the GPU
    cfg2 = pp.config.pedestrian_d435i_config(B)
    cfg2["model"]["second"]["target_assigner"]["sample_positive_fraction"] = 0.25
    tr2 = _trainer(pp, cfg2, d, B)
    with pytest.raises(ValueError, match="global generator"):
        tr2.step(frames, gt_boxes=gts)
    with pytest.raises(ValueError, match="global generator"):
        tr2.engine.assign_targets(gts)
    assert tr2.step(frames, gt_boxes=None, labels=np.stack([r["labels"] for r in ref]),
                    reg_targets=np.stack([r["bbox_targets"] for r in ref]))["num_positives"] > 0
    tr2.close()
    # the handle still trains from boxes, and still assigns the same targets
    out = tr.step(frames, gt_boxes=gts)
    assert out["num_positives"] == sum(int((r["labels"] > 0).sum()) for r in ref)
    eng.upload(frames)
    for r, w in zip(eng.assign_targets(gts), ref):
        assert np.array_equal(r["labels"], w["labels"]) and np.array_equal(r["bbox_targets"], w["bbox_targets"])
    tr.close()
