"""Training metrics on the GPU (csrc/metrics.hip; pp_head_metrics, pp_set_train_metrics): the counts on injected
logits against the host restatement (exact), on the resident head map (exact up to anchors on a threshold), inside
the training step, and the switch left off.  tiny_config: 16 x 20 = 320 head pixels, one full 256-thread workgroup
and a 64-pixel tail, 640 anchors."""

import numpy as np
import pytest

import util_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return load_golden("ref_train_metrics.npz")


def _engine(pp, ncls, B):
    cfg = pp.config.tiny_config(B)
    cfg["model"]["second"]["num_class"] = ncls
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=4096)
    assert eng.d.num_anchors == 640 and eng.d.head_h * eng.d.head_w == 320 and eng.d.num_anchor_per_loc == 2
    return eng


def _same(pp, eng, labels, logits, what):
    got = eng.head_metrics(labels, cls_preds=logits)
    want = pp.metrics.head_metrics_np(labels, logits)
    print(what, "counts", got["counts"][:17].tolist())
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], want), (what, got["counts"], want)
    assert np.array_equal(got["fn"], got["n_pos"] - got["tp"]) and np.array_equal(got["tn"], got["n_neg"] - got["fp"])
    return got


# ---- a. injected logits: exact ----
@pytest.mark.parametrize("case", ["b2c1", "b3c2", "b1c3"])
def test_injected_logits_equal_the_host_restatement(pp, hip_lib, gold, case):
    """The committed seeded logits (clear of every threshold: tests/test_train_metrics_host.py) with mixed labels, with
    all labels -1 and with all labels 0; batch 2 / 3 / 1, num_class 1 / 2 / 3."""
    logits, labels = gold[f"{case}/logits"], gold[f"{case}/labels"]
    B, A, ncls = logits.shape[1:]
    eng = _engine(pp, ncls, B)
    for s in (0, 2):                                            # (step 2: no positives)
        got = _same(pp, eng, labels[s], logits[s], f"{case} step {s}")
        assert got["n_pos"] + got["n_neg"] == (labels[s] != -1).sum()
    # the 4-D head-map shape is taken as well
    assert np.array_equal(eng.head_metrics(labels[0], logits[0].reshape(B, 16, 20, 2 * ncls))["counts"],
                          pp.metrics.head_metrics_np(labels[0], logits[0]))
    ign = _same(pp, eng, np.full((B, A), -1, np.int32), logits[1], f"{case} all ignored")
    assert not ign["counts"].any()
    bg = _same(pp, eng, np.zeros((B, A), np.int32), logits[1], f"{case} all background")
    assert bg["n_neg"] == B * A and bg["n_pos"] == 0 and not bg["tp"].any() and bg["fp"][0] > bg["fp"][6] > 0
    # a smaller batch than the engine's, and the same bytes on a second run
    if B > 1:
        _same(pp, eng, labels[3][:1], logits[3][:1], f"{case} batch 1 of {B}")
    again = eng.head_metrics(labels[0], cls_preds=logits[0])["counts"]
    assert np.array_equal(again, pp.metrics.head_metrics_np(labels[0], logits[0]))
    eng.close()


def test_hand_placed_logits(pp, hip_lib):
    """Values both implementations decide exactly: 0 (score 0.5, not above it), +-80, NaN, a two-class tie -- in the first
    workgroup, across the 256-pixel boundary and in the last pixel of the tail."""
    nan = np.float32("nan")
    pat = np.array([[0.0, -3.0], [80.0, -80.0], [-80.0, -80.0], [nan, 5.0], [5.0, nan], [2.0, 2.0], [-80.0, 80.0], [nan, nan],
                    [0.0, 0.0], [-0.0, 80.0]], np.float32)
    eng = _engine(pp, 2, 3)
    B, A = 3, 640
    logits = np.full((B, A, 2), -80.0, np.float32)
    labels = np.zeros((B, A), np.int32)
    for b, start in enumerate((0, 2 * 256 - 5, A - len(pat))):
        logits[b, start:start + len(pat)] = pat
        labels[b, start:start + len(pat)] = [0, 1, 0, 2, 1, 1, 2, -1, 1, 2]
    got = _same(pp, eng, labels, logits, "hand-placed")
    # per frame: rows 0, 1, 2, 4, 5, 6, 9 of the pattern hit, every filler anchor is a background hit
    assert got["acc_hit"] == B * (A - len(pat) + 7)
    assert got["tp"].tolist() == [B * 5, B * 5, B * 4, B * 4, B * 4, B * 3, B * 3] and got["fp"].tolist() == [B, B, 0, 0, 0, 0, 0]
    # labels rotated: every class against every pattern row
    for k in (1, 2):
        _same(pp, eng, np.where(labels >= 0, (labels + k) % 3, labels).astype(np.int32), logits, f"hand-placed + {k}")
    eng.close()


def test_argument_errors(pp, hip_lib):
    eng = _engine(pp, 1, 2)
    L, h = eng._lib, eng._h
    lab = np.zeros((2, 640), np.int32)
    counts = np.full(32, -5, np.int64)
    ARG, STATE = 1, 2
    assert L.pp_head_metrics(h, None, 2, None, counts.ctypes.data) == ARG
    assert L.pp_head_metrics(h, lab.ctypes.data, 2, None, None) == ARG
    assert L.pp_head_metrics(h, lab.ctypes.data, 0, None, counts.ctypes.data) == ARG
    assert L.pp_head_metrics(h, lab.ctypes.data, 3, None, counts.ctypes.data) == ARG
    assert L.pp_set_train_metrics(h, 2) == ARG and L.pp_set_train_metrics(h, -1) == ARG
    assert L.pp_get_train_metrics_enabled(h, None) == ARG
    assert L.pp_get_train_metrics(h, None) == ARG
    assert L.pp_get_train_metrics(h, counts.ctypes.data) == STATE          # no step has run
    assert (counts == -5).all()
    assert eng.train_metrics is False
    eng.set_train_metrics(True)
    assert eng.train_metrics is True
    assert L.pp_get_train_metrics(h, counts.ctypes.data) == STATE          # still no step
    with pytest.raises(ValueError):
        eng.head_metrics(lab[:, :10])
    with pytest.raises(ValueError):
        eng.head_metrics(lab, cls_preds=np.zeros((2, 640, 2), np.float32))
    eng.close()


# ---- b. the resident head map ----
def _detect_problem(pp, B=2, seed=7):
    cfg = pp.config.tiny_config(B)
    d = pp.config.Derived(cfg)
    w = pp.weights.init_weights(d, seed=seed)
    w["rpn/conv_cls/bias"] = np.array(w["rpn/conv_cls/bias"], np.float32) + np.float32(0.37)      # a non-zero class bias
    rng = np.random.default_rng(seed)
    frames = [rng.uniform([0, -0.64, -3], [1.6, 0.64, 3], (n, 3)).astype(np.float32) for n in (900, 400)[:B]]
    labels = rng.choice([-1, 0, 0, 1], size=(B, d.num_anchors)).astype(np.int32)
    return cfg, d, w, frames, labels


# (tests/test_train_metrics_host.py checks on the CPU oracle's forward pass that this problem stays under the cap)
def _interval_check(pp, counts, labels, cls):
    """Every counter within what the anchors on a threshold leave open (at most 0.1 % of the anchors may be)."""
    M = pp.metrics
    near = M.near_threshold(cls)
    assert near.sum() <= 1e-3 * near.size, f"{int(near.sum())} of {near.size} anchors within 4 * 2**-24 of a threshold"
    want = M.unpack_counts(M.head_metrics_np(labels, cls))
    got = M.unpack_counts(counts)
    print("resident head map: counts", np.asarray(counts)[:17].tolist(), "anchors on a threshold:", int(near.sum()))
    slack_pos, slack_neg = int((near & (labels > 0)).sum()), int((near & (labels == 0)).sum())
    assert got["n_pos"] == want["n_pos"] and got["n_neg"] == want["n_neg"]
    assert abs(got["acc_hit"] - want["acc_hit"]) <= int(near.sum())
    assert (np.abs(got["tp"] - want["tp"]) <= slack_pos).all() and (np.abs(got["fp"] - want["fp"]) <= slack_neg).all()


def test_resident_head_map_after_detect(pp, hip_lib):
    cfg, d, w, frames, labels = _detect_problem(pp)
    eng = pp.Engine(cfg, max_batch=2, max_points_per_frame=4096)
    eng.load_weights(w)
    rect, trv, _ = pp.synth.default_calib()
    eng.detect(frames, np.stack([rect] * 2), np.stack([trv] * 2))
    got = eng.head_metrics(labels)
    cls = eng.intermediates()["cls_preds"].reshape(2, d.num_anchors, 1)
    _interval_check(pp, got["counts"], labels, cls)
    assert got["tp"][0] > 0 and got["fp"][0] > 0
    # the same logits handed in as an array: the same bytes (one kernel, two strides)
    assert np.array_equal(eng.head_metrics(labels, cls_preds=cls)["counts"], got["counts"])
    eng.close()


# ---- c. inside the step ----
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


def _trainer(pp, metrics, seed=21):
    cfg, d, w, frames, _ = _detect_problem(pp, seed=seed)
    tr = pp.Trainer(cfg, w, max_batch=2, max_points_per_frame=4096, learning_rate=2e-4, weight_decay=1e-4, metrics=metrics)
    return tr, d, frames


def test_counts_inside_the_step(pp, hip_lib):
    M = pp.metrics
    tr, d, frames = _trainer(pp, True)
    assert tr.engine.train_metrics is True and tr.metrics_steps == 500
    by_hand = M.TrainMetrics()
    for i in range(2):
        labels, reg = _targets(d, 2, 11 + i)
        out = tr.step(frames, labels, reg)
        counts = tr.engine.train_metrics_counts()
        print("step", i, "counts", counts[:17].tolist())
        # the step leaves its head map on the device: the standalone call right behind it reads the same logits
        assert np.array_equal(tr.engine.head_metrics(labels)["counts"], counts), i
        assert np.array_equal(tr.engine.train_metrics_counts(), counts)          # (the standalone call left them alone)
        c = M.unpack_counts(counts)
        assert c["n_pos"] == out["num_positives"] == (labels > 0).sum() and c["n_neg"] == (labels == 0).sum()
        assert (c["tp"] + c["fn"] == c["n_pos"]).all() and (c["fp"] + c["tn"] == c["n_neg"]).all()
        assert (np.diff(c["tp"]) <= 0).all() and (np.diff(c["fp"]) <= 0).all()
        assert 0 <= c["acc_hit"] <= labels.size and not counts[17:].any()
        by_hand.update(counts, out["cls_loss_reduced"], out["loc_loss_reduced"])
        assert tr.metrics() == by_hand.result()
    r = tr.metrics()
    assert list(r) == ["cls_loss", "cls_loss_rt", "loc_loss", "loc_loss_rt", "rpn_acc"] + [k for pk in M.threshold_keys() for k in pk]
    assert 0 <= r["rpn_acc"] <= 1 and np.isfinite(r["cls_loss"])
    tr.reset_metrics()
    assert np.isnan(tr.metrics()["rpn_acc"])
    # targets assigned on the GPU from boxes: the counts are taken on the labels the step trained on
    gts = [np.array([[0.8, 0.0, -0.6, 0.6, 0.8, 1.73, 0.0]], np.float32)] * 2
    out = tr.step(frames, gt_boxes=gts)
    c = M.unpack_counts(tr.engine.train_metrics_counts())
    assert c["n_pos"] == out["num_positives"] > 0 and c["n_neg"] > 0
    tr.close()


def test_voxelnet_passes_the_option_through(pp, hip_lib):
    cfg, d, w, frames, _ = _detect_problem(pp, seed=21)
    labels, reg = _targets(d, 2, 11)
    net = pp.VoxelNet(cfg, training=True, max_batch=2, max_points_per_frame=4096, metrics=True)
    net.load_weights(w)
    out = net.train_step(frames, labels, reg)
    assert set(out["metrics"]) >= {"rpn_acc", "prec@50", "rec@95", "cls_loss_rt"} and out["metrics"]["cls_loss_rt"] == out["cls_loss_reduced"]
    net.trainer.close()
    plain = pp.VoxelNet(cfg, training=True, max_batch=2, max_points_per_frame=4096)
    plain.load_weights(w)
    assert "metrics" not in plain.train_step(frames, labels, reg)
    plain.trainer.close()


# ---- d. off means untouched ----
def test_off_is_untouched_and_on_only_reads(pp, hip_lib):
    """The kernel only reads: a trainer with the metrics on and one without compute the same bits (losses, gradients,
    parameters, BatchNorm state), so the one without is the behaviour from before the switch existed."""
    off, d, frames = _trainer(pp, False)
    on, _, _ = _trainer(pp, True)
    on2, _, _ = _trainer(pp, True)
    seen = []
    for i in range(3):
        labels, reg = _targets(d, 2, 31 + i)
        a, b, c = off.step(frames, labels, reg), on.step(frames, labels, reg), on2.step(frames, labels, reg)
        assert a == b == c, (i, a, b)
        for t in (on, on2):
            assert np.array_equal(off.grads.cpu().numpy(), t.grads.cpu().numpy()), i
            assert np.array_equal(off.params.cpu().numpy(), t.params.cpu().numpy()), i
            assert np.array_equal(off.state.cpu().numpy(), t.state.cpu().numpy()), i
        assert np.array_equal(on.engine.train_metrics_counts(), on2.engine.train_metrics_counts())     # two runs, same counts
        seen.append(on.engine.train_metrics_counts())
        with pytest.raises(RuntimeError, match="metrics off"):
            off.engine.train_metrics_counts()
    with pytest.raises(RuntimeError, match="metrics=True"):
        off.metrics()
    assert off.engine.train_metrics is False
    for t in (off, on):
        captures, replays = t.engine.train_graph_stats()
        assert captures <= 2 and replays == 3, (captures, replays)
    # switching on a live engine captures once more per input buffer, then replays again
    c0, r0 = off.engine.train_graph_stats()
    off.engine.set_train_metrics(True)
    labels, reg = _targets(d, 2, 31)
    for i in range(3):
        off.step(frames, labels, reg)
    c1, r1 = off.engine.train_graph_stats()
    assert c0 < c1 <= c0 + 2 and r1 == r0 + 3, (c0, c1, r0, r1)
    assert off.engine.train_metrics_counts().sum() > 0
    off.engine.set_train_metrics(False)
    off.step(frames, labels, reg)
    with pytest.raises(RuntimeError, match="metrics off"):
        off.engine.train_metrics_counts()
    # a step in flight: the switch and the standalone call are refused, the step is unharmed
    on.engine.upload(frames)
    on.engine.train_step_async(on.params.data_ptr(), on.grads.data_ptr(), on.state.data_ptr(), labels, reg)
    assert on.engine._lib.pp_set_train_metrics(on.engine._h, 0) == 2
    counts = np.zeros(32, np.int64)
    assert on.engine._lib.pp_get_train_metrics(on.engine._h, counts.ctypes.data) == 2
    assert on.engine._lib.pp_head_metrics(on.engine._h, labels.ctypes.data, 2, None, counts.ctypes.data) == 2
    on.engine.train_step_wait()
    assert on.engine.train_metrics_counts()[1] == (labels > 0).sum()
    for t in (off, on, on2):
        t.close()
