"""Anchors per location other than the shipped two (tests/anchor_layouts.py: 1 and 3 per location, two sizes, a rotation
that is neither 0 nor pi/2, two classes, no direction head, an odd 9 x 7 grid with A % 16 = 13 / 15 and A % 4 = 1 / 3)
through everything that indexes by num_anchor_per_loc: the fused head row [box napl*7 | cls napl*ncls | dir napl*2 | pad] of
the deconv / head epilogues, the compact class-logit plane, the candidate scan (16-anchor fast path, strided fallback),
k_loss_pixels<NAPL, NCLS> and k_loss_count's scalar path, the metrics kernel, targets.hip, the head fold of the weight
publish, upload_heads / fetch_heads and the anchor-cell table -- against the oracles the two-per-location tests use.

The 20 x 16 layouts run the uniform deconv kernels with fused heads (and the class plane they leave); the 9 x 7 ones the
generic GEMM with a separate head layer.  Every test asserts what makes it meaningful: a mixed anchor mask, at least one
detection per frame, the layer tags of the kernel family, A % 16 / A % 4 as tabulated.
"""
import numpy as np
import pytest
import torch

import anchor_layouts as L
from oracle import loss_ref, ref_numpy as rn, train_ref
import util_ref

pytestmark = pytest.mark.gpu

TOL = 1e-4
B = 2
CFG_TA = {"sample_positive_fraction": "None", "rpn_batch_size": 512}
STEP_LAYOUTS = ["one", "three", "three-2cls-nodir", "three-odd"]
HEAD_KEYS = ("box_preds", "cls_preds", "dir_cls_preds")


class Problem:
    """One layout: config, weights, two frames (and a third for the three-frame engine), the oracle's run on them, boxes
    and the host assigner's targets.  Built once per layout and left unchanged."""

    def __init__(self, pp, name):
        self.name = name
        self.cfg = L.layout_config(pp, name, B)
        d = self.d = pp.config.Derived(self.cfg)
        self.napl, self.A = L.LAYOUTS[name][5], L.LAYOUTS[name][6]
        assert d.num_anchor_per_loc == self.napl and d.num_anchors == self.A
        self.odd = L.LAYOUTS[name][4]
        assert (self.A % 16, self.A % 4) == {"three-odd": (13, 1), "one-odd": (15, 3)}.get(name, (0, 0))
        self.w = pp.weights.init_weights(d, seed=3)
        self.frames3 = L.layout_frames(d, 13, counts=(700, 90, 300))
        self.frames = self.frames3[:B]
        self.calib = pp.synth.default_calib()
        rect, trv, p2 = self.calib
        self.ref3 = util_ref.oracle_detect(d, self.w, self.frames3, rect, trv, p2)
        self.ref = util_ref.oracle_detect(d, self.w, self.frames, rect, trv, p2)
        for fr, det in zip(self.ref3["frames"], self.ref3["dets"]):
            m = fr["anchors_mask"]
            assert m.any() and not m.all(), "the oracle's anchor mask must be mixed"
            assert det["scores"] is not None and len(det["scores"]) >= 1, "the oracle must detect something in every frame"
        self.masks = np.stack([f["anchors_mask"] for f in self.ref["frames"]])
        self.keys = [k for k in HEAD_KEYS if k in self.ref["preds"]]
        assert ("dir_cls_preds" in self.keys) == d.use_direction_classifier
        self.anchors = self.ref["frames"][0]["anchors"]
        # 3-4 boxes per frame around the occupied corner: near an anchor's size, one at 0.785, one across, one far off
        size = np.asarray(d.anchor_cfg["sizes"], np.float32).reshape(-1, 3)
        lo, hi = np.array(d.pc_range[:3]), np.array(d.pc_range[3:])
        self.gts, self.classes = [], []
        for b, rows in enumerate(([(0.15, 0.12, 0, 0.785), (0.30, 0.22, -1, 0.1), (0.22, 0.10, 0, 1.5), (0.9, 0.9, 0, -2.9)],
                                  [(0.12, 0.15, -1, 0.785), (0.28, 0.10, 0, -1.62), (0.33, 0.24, 0, 3.0)])):
            g = []
            for fx, fy, si, rot in rows:
                xy = lo[:2] + (hi[:2] - lo[:2]) * np.array([fx, fy])
                g.append([xy[0], xy[1], -1.0, *(size[si] * np.array([1.05, 0.95, 1.0])), rot])
            self.gts.append(np.array(g, np.float32))
            self.classes.append(((np.arange(len(g)) + b) % d.num_class + 1).astype(np.int32))
        self.host = [pp.target_assigner.assign(self.anchors, self.gts[b], self.masks[b], self.classes[b], 0.5, 0.35, CFG_TA)
                     for b in range(B)]
        self.labels = np.stack([h["labels"] for h in self.host]).astype(np.int32)
        self.reg = np.stack([h["bbox_targets"] for h in self.host]).astype(np.float32)
        assert all((h["labels"] > 0).sum() >= 2 for h in self.host), "every frame must have positives"
        assert (self.labels == -1).any() and (self.labels == 0).any()
        if d.num_class > 1:
            assert set(np.unique(self.labels[self.labels > 0])) == set(range(1, d.num_class + 1)), "every class among the positives"

    def check_tags(self, tags):
        """The layer tags that say which kernel family ran (so that the test cannot silently stop covering it)."""
        deconvs = [t for t in tags if ":deconv" in t]
        assert len(deconvs) == 3, tags
        if self.odd:      # generic GEMM for the separable layers (odd width), the heads as a layer of their own
            assert tags[-1].startswith("k_gemm_layer<") and tags[-1].endswith(":heads"), tags
            assert all(t.startswith("k_gemm_layer<") for t in tags if ":block" in t), tags
        else:             # uniform deconv kernels, heads fused into them (the last one leaves the class plane)
            assert not any(t.endswith(":heads") for t in tags), tags
            assert all(t.startswith(("k_deconv_k4<", "k_deconv_u<", "k_deconv_r<")) for t in deconvs), tags


@pytest.fixture(scope="module")
def problems(pp, hip_lib):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Problem(pp, name)
        return cache[name]

    return get


def _engine(pp, p, max_batch=B, weights=None):
    eng = pp.Engine(L.layout_config(pp, p.name, max_batch), max_batch=max_batch, max_points_per_frame=4096)
    eng.load_weights(p.w if weights is None else weights)
    return eng


def _detect(pp, p, eng, frames, ref):
    """detect + intermediates against the oracle's run: pillars, mask exact; head maps within TOL; detections."""
    from test_gpu_parity import _assert_dets
    n_f = len(frames)
    rect, trv, _ = p.calib
    dets, n = eng.detect(frames, np.stack([rect] * n_f), np.stack([trv] * n_f))
    im = eng.intermediates()
    for b in range(n_f):
        fr = ref["frames"][b]
        P = fr["coordinates"].shape[0]
        assert im["n_pillars"][b] == P and np.array_equal(im["coors"][b, :P], fr["coordinates"])
        assert np.array_equal(im["num_points"][b, :P], fr["num_points"])
        assert np.array_equal(im["anchors_mask"][b].astype(bool), fr["anchors_mask"])
    assert [k for k in HEAD_KEYS if k in im] == p.keys
    for k in p.keys:
        assert im[k].shape == ref["preds"][k].shape, k
        print(f"{p.name} B={n_f} {k}: max |diff| {np.abs(im[k] - ref['preds'][k]).max():.2e}")
        np.testing.assert_allclose(im[k], ref["preds"][k], rtol=0, atol=TOL, err_msg=k)
    _assert_dets([pp.VoxelNet._to_dict(dets[b], int(n[b]), b) for b in range(n_f)], ref["dets"])
    return im, dets, n


# ------------------------------------------------------------------ 1. end to end
@pytest.mark.parametrize("name", L.NAMES)
def test_end_to_end(pp, problems, name):
    p = problems(name)
    eng = _engine(pp, p)
    im2, _, _ = _detect(pp, p, eng, p.frames, p.ref)
    tags2 = eng.layer_tags()
    print(name, "B=2", tags2)
    p.check_tags(tags2)
    again, _, _ = _detect(pp, p, eng, p.frames, p.ref)
    assert all(again[k].tobytes() == im2[k].tobytes() for k in p.keys), "a second pass gives the same bits"
    eng.close()
    eng3 = _engine(pp, p, max_batch=3)
    im3, _, _ = _detect(pp, p, eng3, p.frames3, p.ref3)
    tags3 = eng3.layer_tags()
    print(name, "B=3", tags3)
    p.check_tags(tags3)
    if tags3 == tags2:      # the same kernels: a frame's head map does not depend on its batch
        for k in p.keys:
            assert im3[k][:B].tobytes() == im2[k].tobytes(), (k, "shared frames, same kernels: same bits")
    eng3.close()


# ------------------------------------------------------------------ 2. hand-built head maps through predict
@pytest.mark.parametrize("name", L.NAMES)
def test_predict_every_class_column_wins(pp, problems, name):
    """Engine.predict on the oracle's head maps (upload_heads; no class plane: the strided scan over the head rows).  Frame
    j is oracle frame j % 2 with one class logit per (anchor-in-location r, class k) overwritten by a distinct large value on
    a masked-in anchor, the j-th column position getting the largest: that anchor is frame j's first detection, with the
    label, box and direction flip the oracle gives.  A shifted column cannot pass."""
    from test_gpu_parity import _assert_dets
    p = problems(name)
    d, napl, ncls = p.d, p.napl, p.d.num_class
    combos = [(r, k) for r in range(napl) for k in range(ncls)]
    nf = len(combos)
    eng = pp.Engine(L.layout_config(pp, name, nf), max_batch=nf, max_points_per_frame=4096)
    preds = {k: np.stack([p.ref["preds"][k][j % B] for j in range(nf)]).copy() for k in p.keys}
    mask = np.stack([p.masks[j % B] for j in range(nf)]).astype(np.uint8)
    cls = preds["cls_preds"].reshape(nf, p.A, ncls)
    assert cls.max() < 4.0, "the planted logits must stand above the network's own"
    rng = np.random.default_rng(17)
    planted = []
    for j in range(nf):
        on = np.flatnonzero(mask[j])
        where = {}
        for i, (r, k) in enumerate(combos):
            cand = [a for a in on if a % napl == r and a // napl not in {v // napl for v in where.values()}]
            where[r, k] = int(rng.choice(cand))
            cls[j, where[r, k], k] = 6.0 + 0.25 * i + (4.0 if i == j else 0.0)      # distinct; combo j on top
        planted.append(where)
    rect, trv, _ = p.calib
    rects, trvs = np.stack([rect] * nf), np.stack([trv] * nf)
    dets, n = eng.predict(preds["box_preds"], preds["cls_preds"], preds.get("dir_cls_preds"), mask, rects, trvs)
    ex = (None, None, None, rects, trvs, None, np.stack([p.anchors] * nf), mask, np.arange(nf), None)
    ref = rn.predict(ex, preds, d.nms_dict())
    _assert_dets([pp.VoxelNet._to_dict(dets[j], int(n[j]), j) for j in range(nf)], ref)
    winners = set()
    for j, (r, k) in enumerate(combos):
        a = planted[j][r, k]
        assert n[j] >= 1 and dets[j]["anchor_index"][0] == a, (j, r, k, a, dets[j]["anchor_index"][:n[j]])
        assert dets[j]["label"][0] == k and ref[j]["label_preds"][0] == k
        assert abs(dets[j]["score"][0] - 1 / (1 + np.exp(-(10.0 + 0.25 * j)))) < 1e-6
        if d.use_direction_classifier:
            want_dir = int(np.argmax(preds["dir_cls_preds"].reshape(nf, p.A, 2)[j, a]))
            assert dets[j]["dir_label"][0] == want_dir
        winners.add((int(dets[j]["anchor_index"][0]) % napl, int(dets[j]["label"][0])))
    assert winners == set(combos), "every (r, k) column position is the winner of some detection"
    eng.close()


def test_no_direction_head_row_ends_at_its_last_class_column(pp, problems):
    """27 columns in use and no direction head: what would be the direction pair of the third anchor of a pixel lies at
    columns 31 and 32 -- padding and the NEXT pixel's first box value.  A NaN there (an anchor nobody selects: masked out)
    must change nothing; the post-process used to read it into its non-finite check and refuse the frame."""
    from test_gpu_parity import _assert_dets
    p = problems("three-2cls-nodir")
    d = p.d
    eng = pp.Engine(L.layout_config(pp, p.name, 1), max_batch=1, max_points_per_frame=4096)
    preds = {k: p.ref["preds"][k][:1].copy() for k in p.keys}
    mask = p.masks[:1].astype(np.uint8).copy()
    # a masked-in third anchor (r = 2) whose right-hand neighbour pixel is in the same map row
    on = [a for a in np.flatnonzero(mask[0]) if a % 3 == 2 and (a // 3) % d.head_w < d.head_w - 1]
    a = int(on[len(on) // 2])
    px = a // 3
    mask[0, 3 * (px + 1):3 * (px + 2)] = 0
    preds["cls_preds"].reshape(1, p.A, 2)[0, a, 1] = 11.0
    preds["box_preds"].reshape(1, d.head_h * d.head_w, 21)[0, px + 1, 0] = np.nan
    rect, trv, _ = p.calib
    dets, n = eng.predict(preds["box_preds"], preds["cls_preds"], None, mask, rect[None], trv[None])
    ex = (None, None, None, rect[None], trv[None], None, p.anchors[None], mask, np.arange(1), None)
    ref = rn.predict(ex, preds, d.nms_dict())
    _assert_dets([pp.VoxelNet._to_dict(dets[0], int(n[0]), 0)], ref)
    assert dets[0]["anchor_index"][0] == a and dets[0]["label"][0] == 1 and dets[0]["dir_label"][0] == 0
    eng.close()


# ------------------------------------------------------------------ 3. targets, 4. loss
@pytest.mark.parametrize("name", L.NAMES)
def test_targets_and_head_loss(pp, problems, name):
    from test_gpu_targets import _same_targets
    p = problems(name)
    d = p.d
    eng = _engine(pp, p)
    im, _, _ = _detect(pp, p, eng, p.frames, p.ref)
    assert np.array_equal(eng.anchors, p.anchors)
    # ---- Engine.assign_targets against the host assigner: the resident frames' masks, and the masks passed in ----
    for how, got in (("resident", eng.assign_targets(p.gts, p.classes)),
                     ("masks passed", eng.assign_targets(p.gts, p.classes, anchors_mask=p.masks))):
        for b in range(B):
            _same_targets(got[b], p.host[b], f"{name} frame {b} ({how})", log_ulp=4)
            pos = p.host[b]["assigned_anchors_inds"]
            ratio = p.gts[b][p.host[b]["positive_gt_id"], 3:6] / eng.anchors[pos, 3:6]
            assert np.array_equal(got[b]["bbox_targets"][pos, 3:6], np.log(ratio.astype(np.float64)).astype(np.float32))
            assert (got[b]["labels"][~p.masks[b]] == -1).all()
    if 0.785 in d.anchor_cfg["rotations"]:      # the box at 0.785 matched the 0.785 anchor: angle target exactly 0
        for b in range(B):
            pos = np.flatnonzero(got[b]["labels"] > 0)
            at = pos[(eng.anchors[pos, 6] == np.float32(0.785)) & (got[b]["bbox_targets"][pos, 6] == 0.0)]
            assert len(at) >= 1, (name, b)
    # ---- head_loss on the resident head maps with those targets ----
    s = d.config["model"]["second"]
    res = eng.head_loss(p.labels, p.reg)
    vals, grads = loss_ref.training_loss(s, im["box_preds"], im["cls_preds"], im.get("dir_cls_preds"), p.labels, p.reg, p.anchors)
    keys = ["loss", "loc_loss_reduced", "cls_loss_reduced", "cls_pos_loss", "cls_neg_loss"]
    gkeys = ["box_preds_grad", "cls_preds_grad"]
    if d.use_direction_classifier:
        keys.append("dir_loss_reduced")
        gkeys.append("dir_cls_preds_grad")
    else:
        assert res["dir_loss_reduced"] == 0.0 and "dir_cls_preds_grad" not in res
    for k in keys:
        print(f"{name} {k}: kernel {res[k]:.8g}, restatement {vals[k]:.8g}")
        assert abs(res[k] - vals[k]) <= 2e-5 * max(1e-3, abs(vals[k])), (k, res[k], vals[k])
    assert res["num_positives"] == vals["num_positives"] == int((p.labels > 0).sum())
    for k in gkeys:
        assert res[k].shape == grads[k].shape
        np.testing.assert_allclose(res[k], grads[k], rtol=2e-4, atol=1e-8, err_msg=k)
        assert res[k].any(), k
    used = p.napl * (7 + d.num_class + (2 if d.use_direction_classifier else 0))
    assert used == {"one": 10, "three": 30, "two-sizes": 22, "three-2cls-nodir": 27, "three-odd": 30, "one-odd": 10}[name]
    assert not res["head_grad"][:, :, used:].any(), "columns past the heads get no gradient"
    again = eng.head_loss(p.labels, p.reg)
    assert again["loss"] == res["loss"] and again["head_grad"].tobytes() == res["head_grad"].tobytes()
    eng.close()


# ------------------------------------------------------------------ 5. training step, 6. round trip
def _step_targets(p, seed=11):
    """Random targets as test_gradients_match_autograd_small_grids draws them (positives on any anchor, every class)."""
    rng = np.random.default_rng(seed)
    labels = rng.choice([-1, 0, 0, 0, 0], size=(B, p.A)).astype(np.int32)
    reg = np.zeros((B, p.A, 7), np.float32)
    for b in range(B):
        pos = rng.choice(p.A, 40 if b == 0 else 13, replace=False)
        labels[b, pos] = rng.integers(1, p.d.num_class + 1, len(pos))
        reg[b, pos] = rng.normal(0, 0.4, (len(pos), 7)).astype(np.float32)
    return labels, reg


@pytest.mark.parametrize("name", STEP_LAYOUTS)
def test_training_step_matches_autograd(pp, problems, name):
    from test_gpu_train import _rel_errors
    from test_gpu_train_metrics import _interval_check
    p = problems(name)
    d = p.d
    labels, reg = _step_targets(p)
    # Weights under which no pre-ReLU value (and no PFN max) of the restated step lies within 5e-6 of its kink: ReLU is not
    # differentiable there, and an implementation whose round-off (~1e-6 on a normalised activation) puts such an element on
    # the other side differs by that element's whole contribution (oracle/train_ref.py, `margins`).  The clouds fill one
    # corner of the map, so whole regions share a value; seed 3 leaves one of them 2e-7 from zero in deconv3.
    w = pp.weights.init_weights(d, seed=21 if p.odd else 22)
    ex = p.ref["example"]
    margins = {}
    vals, grads, _, preds = train_ref.training_step(d, w, ex, labels, reg, p.anchors, margins=margins)
    margin = min(v for k, v in margins.items() if not k.startswith("#"))
    print(f"{name}: smallest distance of a pre-ReLU value to its kink {margin:.2e}")
    assert margin >= 5e-6, margins
    tr = pp.Trainer(p.cfg, w, max_batch=B, max_points_per_frame=4096, metrics=True)
    out = tr.forward_backward(p.frames, labels, reg)
    g1 = tr.grads.cpu().numpy().copy()
    counts = tr.engine.train_metrics_counts()
    keys = ["loss", "loc_loss_reduced", "cls_loss_reduced", "cls_pos_loss", "cls_neg_loss"] + \
        (["dir_loss_reduced"] if d.use_direction_classifier else [])
    for k in keys:
        assert abs(out[k] - vals[k]) <= 1e-5 * max(1.0, abs(vals[k])), (k, out[k], vals[k])
    if not d.use_direction_classifier:
        assert out["dir_loss_reduced"] == 0.0 and "rpn/conv_dir_cls/kernel" not in tr.gradients()
    assert out["num_positives"] == vals["num_positives"] == 53
    assert tr.gradients()["rpn/conv_box/kernel"].shape[-1] == 7 * p.napl
    assert tr.gradients()["rpn/conv_cls/kernel"].shape[-1] == d.num_class * p.napl
    (wn, wmax), _ = _rel_errors(tr.gradients(), grads)
    print(f"{name}: {tr.params.numel()} trainable parameters, worst relative gradient error {wmax:.2e} ({wn})")
    assert wmax <= 1e-4, (wn, wmax)
    _, g64f, _, _ = train_ref.training_step(d, w, ex, labels, reg, p.anchors, dtype=torch.float64,
                                            forced=util_ref.forced_decisions(tr, ex))
    (fn_, fmax), _ = _rel_errors(tr.gradients(), g64f)
    print(f"{name}: against float64 with the step's decisions {fmax:.2e} ({fn_})")
    assert fmax <= 1e-4, (fn_, fmax)
    # the step's metric counts against the host restatement on the restated network's training-mode class logits
    _interval_check(pp, counts, labels, preds["cls_preds"].reshape(B, p.A, d.num_class))
    assert counts[1] == 53
    out2 = tr.forward_backward(p.frames, labels, reg)
    assert out2["loss"] == out["loss"] and np.array_equal(tr.grads.cpu().numpy(), g1), "bit-identical second pass"
    tr.close()


@pytest.mark.parametrize("name", STEP_LAYOUTS)
def test_trained_weights_round_trip(pp, problems, name):
    """Two optimizer steps, then Trainer.weights() into a fresh Engine, and Trainer.detect (the weight publish folds the
    heads on the GPU): both give the head maps of the oracle on those weights."""
    p = problems(name)
    labels, reg = _step_targets(p, seed=12)
    tr = pp.Trainer(p.cfg, p.w, max_batch=B, max_points_per_frame=4096, learning_rate=2e-3, weight_decay=1e-4)
    for _ in range(2):
        tr.step(p.frames, labels, reg)
    w2 = tr.weights()
    pp.weights.check_weights(p.d, w2)
    assert np.abs(w2["rpn/conv_cls/kernel"] - p.w["rpn/conv_cls/kernel"]).max() > 1e-4, "the steps moved the heads"
    rect, trv, p2 = p.calib
    ref2 = util_ref.oracle_detect(p.d, w2, p.frames, rect, trv, p2)
    assert all(r["scores"] is not None for r in ref2["dets"])
    tr.detect(p.frames, np.stack([rect] * B), np.stack([trv] * B))
    im_pub = tr.engine.intermediates()
    for k in p.keys:
        print(f"{name} published {k}: max |diff| {np.abs(im_pub[k] - ref2['preds'][k]).max():.2e}")
        np.testing.assert_allclose(im_pub[k], ref2["preds"][k], rtol=0, atol=TOL, err_msg=k)
    tr.close()
    eng = _engine(pp, p, weights=w2)
    _detect(pp, p, eng, p.frames, ref2)
    eng.close()
