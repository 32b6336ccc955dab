"""Soft-NMS on the GPU: pp_soft_nms (csrc/soft_nms.hip) against what the reference's soft_nms_jit leaves
(tests/golden/ref_soft_nms.npz) and against the host restatement (pp_amd.soft_nms.soft_nms_np), and the detector's soft
mode (k_postprocess<PP_NMS_SOFT>) against the default mode (method hard: byte for byte) and against predict_soft
(tests/soft_nms_ref.py: linear, Gaussian).

Tolerances.  Rows, order, counts and anchor indices are exact everywhere.  Standalone scores: hard and linear use IEEE
+ - x / and one rounding to float32, so they are bit-equal to the restatement; Gaussian goes through exp, whose device
version may differ from numpy's in the last float64 bit, which can move the float32 rounding of a product by one ulp: a
box re-scored k times is allowed k x 2^-23 relative.  Against the fixture: 4 x the relative difference its generator
recorded (plain Python's float32 typing, see tests/test_soft_nms_host.py).  Detector fields and scores: 1e-4, the bound
tests/test_gpu_rotate_nms.py applies to the same kernel's fields (the device's expf / sinf in the box decode move the
stand-up boxes by an ulp, hence the overlaps by ~1e-6); the inputs are drawn so that every decision of the restatement
keeps a margin of 4e-4, four times that bound.

Shapes.  n <= 100 are dense draws as the fixture's.  At n = 1024 and 4096 a selection gap > 1e-5 at every round cannot be
drawn from dense boxes (n scores in (0, 1) put about n^2 x 1e-5 pairs closer than that once decays scatter them), so
those sets are a grid of disjoint boxes with scores on a permuted grid plus 16 jittered copies that do overlap: all of
PP_SNMS_MAX_BOXES rows in LDS, four per thread, the argmax across sixteen wavefronts, and a few re-scorings.
"""
import numpy as np
import pytest

from conftest import load_golden
from oracle import ref_numpy as rn

import class_nms_ref as cr
import soft_nms_ref as sr
from test_soft_nms_host import assert_matches_fixture, fixture_cases
from test_gpu_rotate_nms import _head_maps, _kept_bytes, _tiny_cfg

pytestmark = pytest.mark.gpu

TOL = 1e-4
MARGIN = 4e-4
DEFAULT = dict(sigma=0.5, iou_threshold=0.3, score_floor=0.001)


# ---------------------------------------------------------------- standalone
def test_fixture_rows_and_scores(pp, hip_lib):
    g = load_golden("ref_soft_nms.npz")
    rel = 4.0 * float(g["max_rel_score_diff"])
    for name, dets, method, sigma, nt, thr, pre, post, kept in fixture_cases(g):
        keep, scores = pp.soft_nms.soft_nms(dets, method, sigma, nt, thr, pre, post)
        assert_matches_fixture(name, dets, keep, scores, kept, rel)


def _dense(rng, n):
    side = 45.0 * np.sqrt(max(n, 1))
    xy = rng.uniform(0, side, (n, 2))
    b = np.concatenate([xy, xy + rng.uniform(10.0, 60.0, (n, 2))], axis=1)
    for i in range(n):
        if n > 2 and rng.random() < 0.33:
            j = int(rng.integers(0, n))
            if j != i:
                b[i] = b[j] + rng.normal(0, 4.0, 4)
    return np.concatenate([b, rng.uniform(0.02, 1.0, (n, 1))], axis=1).astype(np.float32)


def _sparse(rng, n, copies=16):
    """n - copies disjoint boxes (cells of 45, sides <= 40: more than 1 apart) and `copies` jittered copies of some."""
    m = n - copies
    side = int(np.ceil(np.sqrt(m)))
    cell = rng.permutation(side * side)[:m]
    xy = np.stack([cell % side, cell // side], axis=1) * 45.0 + rng.uniform(0, 4.0, (m, 2))
    b = np.concatenate([xy, xy + rng.uniform(10.0, 40.0, (m, 2))], axis=1)
    extra = b[rng.choice(m, copies, replace=False)] + rng.normal(0, 2.0, (copies, 4))
    b = np.concatenate([b, extra])[rng.permutation(n)]
    s = (rng.permutation(n) + 0.5) / n
    return np.concatenate([b, s[:, None]], axis=1).astype(np.float32)


_SETS = {}


def _seeded(pp, n, method):
    """The set of (n, method), drawn once with the fixture's margins, and the restatement's result on it."""
    if (n, method) not in _SETS:
        rng = np.random.default_rng(7900 + 3 * n + pp.soft_nms.method_id(method))
        for _ in range(200):
            dets = _dense(rng, n) if n <= 100 else _sparse(rng, n)
            m = pp.soft_nms.decision_margins(dets, method, **DEFAULT)
            if m["gap"] > 1e-5 and m["iou"] > 1e-4 and m["floor"] > 1e-6:
                break
        else:
            raise AssertionError(f"n {n} {method}: no draw with the margins")
        _SETS[(n, method)] = (dets, m, pp.soft_nms.soft_nms_np(dets, method, **DEFAULT))
    return _SETS[(n, method)]


@pytest.mark.parametrize("method", ["hard", "linear", "gaussian"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 100, 1024, 4096])
def test_seeded_sets_equal_the_restatement(pp, hip_lib, n, method):
    dets, m, (rkeep, rscores) = _seeded(pp, n, method)
    keep, scores = pp.soft_nms.soft_nms(dets, method, **DEFAULT)
    again = pp.soft_nms.soft_nms(dets, method, **DEFAULT)
    decayed = int((m["decays"] > 0).sum())
    print(f"n {n} {method}: kept {len(keep)} (host {len(rkeep)}), {decayed} of them re-scored, margins gap {m['gap']:.2e} "
          f"iou {m['iou']:.2e} floor {m['floor']:.2e}")
    assert np.array_equal(keep, rkeep)
    assert (np.diff(scores) <= 0).all()
    if n >= 63:         # the set exercises the rule: hard deletes something, the soft methods re-score something kept
        assert len(keep) < n if method == "hard" else decayed > 0
    if method == "gaussian":
        tol = m["decays"].astype(np.float64) * 2.0 ** -23 * np.abs(rscores.astype(np.float64))
        err = np.abs(scores.astype(np.float64) - rscores.astype(np.float64))
        print(f"   largest score difference {err.max():.3e}, in units of the allowed {np.max(err / np.maximum(tol, 1e-300)):.2f}")
        assert (err <= tol).all()
    else:
        assert np.array_equal(scores, rscores)
    assert keep.tobytes() == again[0].tobytes() and scores.tobytes() == again[1].tobytes()


def test_caps_empty_input_and_refusals(pp, hip_lib):
    sn = pp.soft_nms
    dets, _, _ = _seeded(pp, 100, "gaussian")
    keep, scores = sn.soft_nms(dets, "gaussian", pre_max_size=40, post_max_size=3, **DEFAULT)
    rkeep, rscores = sn.soft_nms_np(dets, "gaussian", pre_max_size=40, post_max_size=3, **DEFAULT)
    assert len(keep) == 3 and np.array_equal(keep, rkeep) and np.allclose(scores, rscores, rtol=3 * 2.0 ** -23, atol=0)
    # both caps bind: without the post cap more come back, and the pre cap keeps a box out that would come back otherwise
    pre_only = sn.soft_nms(dets, "gaussian", pre_max_size=40, **DEFAULT)[0]
    free = sn.soft_nms(dets, "gaussian", **DEFAULT)[0]
    assert len(pre_only) > 3 and len(free) > len(pre_only) and set(pre_only.tolist()) < set(free.tolist())
    assert set(pre_only.tolist()) <= set(np.argsort(-dets[:, 4], kind="stable")[:40].tolist())
    keep, scores = sn.soft_nms(np.zeros((0, 5), np.float32))
    assert keep.shape == (0,) and keep.dtype == np.int64 and scores.shape == (0,) and scores.dtype == np.float32
    many = np.zeros((sn.MAX_BOXES + 1, 5), np.float32)
    with pytest.raises(ValueError, match="PP_SNMS_MAX_BOXES"):
        sn.soft_nms(many)
    # under the cap through pre_max_size; equal scores: lower index first; identical boxes at weight exp(-2): all stay
    keep, scores = sn.soft_nms(many, "gaussian", score_floor=0.0, pre_max_size=100)
    assert np.array_equal(keep, np.arange(100)) and not scores.any()
    bad = dets.copy()
    bad[17, 4] = np.nan
    with pytest.raises(ValueError, match="finite"):
        sn.soft_nms(bad)
    L = pp._lib.lib()
    import ctypes
    nk = ctypes.c_int64(5)
    args = (0, bad.ctypes.data, len(bad))
    tail = (0, 0, None, None, ctypes.byref(nk))
    assert L.pp_soft_nms(*args, 2, ctypes.c_float(0.5), ctypes.c_float(0.3), ctypes.c_float(0.001), *tail) == 1   # NaN score
    assert nk.value == 0
    ok = (0, dets.ctypes.data, len(dets))
    assert L.pp_soft_nms(*ok, 3, ctypes.c_float(0.5), ctypes.c_float(0.3), ctypes.c_float(0.001), *tail) == 1
    assert L.pp_soft_nms(*ok, 2, ctypes.c_float(0.0), ctypes.c_float(0.3), ctypes.c_float(0.001), *tail) == 1
    assert L.pp_soft_nms(*ok, 2, ctypes.c_float(0.5), ctypes.c_float(0.3), ctypes.c_float(-1.0), *tail) == 1


# ---------------------------------------------------------------- detector: method hard is the default rule
def _predict_inputs(pp, d, seed):
    box, cls, dr, mask = _head_maps(d, seed)
    rect, trv, _ = pp.synth.default_calib()
    return box, cls, dr, mask, np.stack([rect] * 3), np.stack([trv] * 3)


@pytest.mark.parametrize("pre,post", [(100, 50), (60, 100), (100, 3)])
def test_soft_hard_is_the_default_mode_byte_for_byte(pp, hip_lib, pre, post):
    eng = pp.Engine(_tiny_cfg(pp, pre, post), max_batch=3, max_points_per_frame=4096)
    fresh = pp.Engine(_tiny_cfg(pp, pre, post), max_batch=3, max_points_per_frame=4096)
    try:
        inputs = _predict_inputs(pp, eng.d, 4000)
        assert eng.nms_mode == "standup" and eng.soft_nms == {"method": "gaussian", "sigma": 0.5, "score_floor": np.float32(0.001)}
        ddets, dn = eng.predict(*inputs)
        eng.set_soft_nms(method="hard", score_floor=1e-30)
        eng.set_nms_mode("soft")
        assert eng.nms_mode == "soft" and eng.soft_nms["method"] == "hard"
        sdets, sn_ = eng.predict(*inputs)
        print(f"pre {pre} post {post}: default kept {dn.tolist()}, soft-hard kept {sn_.tolist()}")
        assert int(dn[2]) == 0 and min(int(dn[0]), int(dn[1])) > 1          # the last frame's mask is all zero
        assert int(dn[0]) < min(pre, 100) or post < min(pre, 100)           # something was suppressed or capped
        assert np.array_equal(dn, sn_) and _kept_bytes(ddets, dn) == _kept_bytes(sdets, sn_)
        eng.set_nms_mode("standup")
        bdets, bn = eng.predict(*inputs)
        fdets, fn = fresh.predict(*inputs)
        assert np.array_equal(fn, bn) and _kept_bytes(fdets, fn) == _kept_bytes(bdets, bn)
        with pytest.raises(ValueError):
            eng.set_nms_mode("polygon")
        assert eng._lib.pp_set_nms_mode(eng._h, 7) == 1 and eng.nms_mode == "standup"       # PP_ERR_ARG
    finally:
        eng.close()
        fresh.close()


def test_soft_hard_through_detect_at_the_shipped_config(pp, hip_lib):
    cfg = pp.config.pedestrian_d435i_config(2)
    eng = pp.Engine(cfg, max_batch=2, max_points_per_frame=8192)
    try:
        eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
        frames = [pp.synth.d435i_cloud(900 + i, 4096) for i in range(2)]
        rect, trv, _ = pp.synth.default_calib()
        rect, trv = np.stack([rect] * 2), np.stack([trv] * 2)
        d0, n0 = (a.copy() for a in eng.detect(frames, rect, trv))
        eng.set_soft_nms("hard", 0.5, 1e-30)
        eng.set_nms_mode("soft")
        d1, n1 = (a.copy() for a in eng.detect(frames, rect, trv))
        print(f"detect: default kept {n0.tolist()}, soft-hard kept {n1.tolist()}")
        assert min(n0.tolist()) > 0
        assert np.array_equal(n0, n1) and _kept_bytes(d0, n0) == _kept_bytes(d1, n1)
        eng.set_nms_mode("standup")
        d2, n2 = eng.detect(frames, rect, trv)
        assert np.array_equal(n0, n2) and _kept_bytes(d0, n0) == _kept_bytes(d2, n2)
    finally:
        eng.close()


# ---------------------------------------------------------------- detector: linear and Gaussian against the restatement
def _example(anchors, mask, rect, trv):
    B = mask.shape[0]
    return (None, None, None, rect, trv, None, np.stack([anchors] * B), mask, np.arange(B), None)


def drawn_soft_case(pp, d, anchors, method, first_seed, sigma=0.5, floor=0.001):
    """Head maps redrawn on the CPU (at most 2000 seeds) until every decision margin of the restatement is > 4e-4."""
    for seed in range(first_seed, first_seed + 2000):
        box, cls, dr, mask, rect, trv = _predict_inputs(pp, d, seed)
        ex = _example(anchors, mask, rect, trv)
        margins = []
        ref = sr.predict_soft(ex, {"box_preds": box, "cls_preds": cls, "dir_cls_preds": dr}, d.nms_dict(), method, sigma,
                              floor, margins)
        if sr.margins_above(margins, MARGIN):
            return seed, (box, cls, dr, mask, rect, trv), ex, ref
    raise AssertionError("no draw keeps every decision 4e-4 from flipping")


def _assert_soft(dets, n, ref, what):
    worst = 0.0
    for b, r in enumerate(ref):
        k = len(r["anchor_index"])
        assert int(n[b]) == k, (what, b, int(n[b]), k)
        assert np.array_equal(dets[b]["anchor_index"][:k], r["anchor_index"]), (what, b)
        if k:
            assert np.array_equal(dets[b]["label"][:k], r["label_preds"]), (what, b)
            np.testing.assert_allclose(dets[b]["box3d_lidar"][:k], r["box3d_lidar"], rtol=0, atol=TOL)
            np.testing.assert_allclose(dets[b]["box3d_camera"][:k], r["box3d_camera"], rtol=0, atol=TOL)
            worst = max(worst, float(np.abs(dets[b]["score"][:k].astype(np.float64) - r["scores"]).max()))
            np.testing.assert_allclose(dets[b]["score"][:k], r["scores"], rtol=0, atol=TOL)
    print(f"{what}: largest score difference {worst:.3e}")
    return worst


FIRST_SEED = {"linear": 4000, "gaussian": 4000}


@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_detector_soft_mode_against_the_restatement(pp, hip_lib, method):
    eng = pp.Engine(_tiny_cfg(pp, 60, 20), max_batch=3, max_points_per_frame=4096)
    try:
        d = eng.d
        seed, inputs, ex, ref = drawn_soft_case(pp, d, eng.anchors, method, FIRST_SEED[method])
        ddets, dn = eng.predict(*inputs)
        eng.set_soft_nms(method=method)
        eng.set_nms_mode("soft")
        dets, n = eng.predict(*inputs)
        print(f"{method} seed {seed}: soft kept {n.tolist()}, default kept {dn.tolist()}")
        assert int(n[2]) == 0
        _assert_soft(dets, n, ref, method)
        # the case discriminates: more rows than the default rule on some frame, and some kept score was decayed
        assert any(int(n[b]) > int(dn[b]) for b in range(2))
        assert any((r["scores"] < r["sigmoid"]).any() for r in ref[:2])
        assert all((np.diff(dets[b]["score"][:n[b]]) <= 0).all() for b in range(3))
    finally:
        eng.close()


# ---------------------------------------------------------------- combinations
def _two_class_inputs(pp, d, seed):
    rng = np.random.default_rng(seed)
    A, napl = d.num_anchors, d.num_anchor_per_loc
    lg = np.stack([np.stack([rng.permutation(np.linspace(-4.0, 4.0, A)) + 1e-4 * c for c in range(2)], axis=-1)
                   for _ in range(3)]).astype(np.float32)
    preds = {"box_preds": (0.3 * rng.standard_normal((3, d.head_h, d.head_w, napl * 7))).astype(np.float32),
             "cls_preds": np.ascontiguousarray(lg.reshape(3, d.head_h, d.head_w, napl * 2)),
             "dir_cls_preds": rng.standard_normal((3, d.head_h, d.head_w, napl * 2)).astype(np.float32)}
    mask = (rng.random((3, A)) < 0.6).astype(np.uint8)
    mask[2] = 0
    return preds, mask


def drawn_per_class_case(pp, d, anchors, first_seed):
    rect, trv, _ = pp.synth.default_calib()
    rect, trv = np.stack([rect] * 3), np.stack([trv] * 3)
    for seed in range(first_seed, first_seed + 2000):
        preds, mask = _two_class_inputs(pp, d, seed)
        margins = []
        ref = cr.predict_per_class(_example(anchors, mask, rect, trv), preds, d.nms_dict(), single=sr.predict_soft,
                                   method="gaussian", margins=margins)
        if sr.margins_above(margins, MARGIN) and cr.distinct_top_scores(preds, mask, 2):
            return seed, preds, mask, rect, trv, ref
    raise AssertionError("no draw keeps every decision 4e-4 from flipping")


PER_CLASS_FIRST_SEED = 5270


def test_per_class_suppression_in_soft_mode(pp, hip_lib):
    cfg = _tiny_cfg(pp, 60, 20)
    cfg["model"]["second"].update(num_class=2, use_soft_nms=True)
    eng = pp.Engine(cfg, max_batch=3, max_points_per_frame=4096)
    try:
        d = eng.d
        eng.set_class_nms("per_class")
        assert eng.nms_mode == "soft" and eng.class_nms == "per_class" and eng.detection_rows == 40
        seed, preds, mask, rect, trv, ref = drawn_per_class_case(pp, d, eng.anchors, PER_CLASS_FIRST_SEED)
        dets, n = eng.predict(preds["box_preds"], preds["cls_preds"], preds["dir_cls_preds"], mask, rect, trv)
        print(f"per class, seed {seed}: kept {n.tolist()}, per class {[fr['class_counts'].tolist() for fr in ref]}")
        assert int(n[2]) == 0 and all((fr["class_counts"] > 0).all() for fr in ref[:2])
        _assert_soft(dets, n, ref, "per class")
        for b, fr in enumerate(ref):
            assert np.array_equal(dets[b]["dir_label"][:n[b]], fr["dir_label"])
    finally:
        eng.close()


def test_projection_in_soft_mode(pp, hip_lib):
    cfg = _tiny_cfg(pp, 60, 20)
    cfg["model"]["second"]["use_soft_nms"] = True
    eng = pp.Engine(cfg, max_batch=3, max_points_per_frame=4096)
    try:
        inputs = _predict_inputs(pp, eng.d, 4000)
        off, noff = eng.predict(*inputs)
        p2 = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2], [0, 0, 1, 0.003], [0, 0, 0, 1]], np.float64)
        dets, n = eng.predict(*inputs, p2=p2)
        assert eng.projection is True and eng.nms_mode == "soft"
        bb = eng.bboxes(3)
        assert min(int(noff[0]), int(noff[1])) > 1
        assert np.array_equal(n, noff) and _kept_bytes(dets, n) == _kept_bytes(off, noff)      # boxes, counts, scores
        for b in range(3):
            k = int(n[b])
            assert not bb[b, k:].any()
            if k:
                alone = pp.projection.box3d_to_bbox_gpu(np.ascontiguousarray(dets[b]["box3d_camera"][:k]), [k], p2)
                assert bb[b, :k].tobytes() == alone.tobytes()
    finally:
        eng.close()


# ---------------------------------------------------------------- state
def _margin_safe_prefix(ex, preds, cfg, method, sigma, floor):
    """Per frame: the restatement cut after the most selections for which every decision margin is > 4e-4 (None: not even
    the first selection is)."""
    B = ex[7].shape[0]
    best = [None] * B
    for r in range(cfg["nms_post_max_size"], 0, -1):
        margins = []
        ref = sr.predict_soft(ex, preds, dict(cfg, nms_post_max_size=r), method, sigma, floor, margins)
        for b in range(B):
            if best[b] is None and sr.margins_above([margins[b]], MARGIN) and len(ref[b]["anchor_index"]):
                best[b] = ref[b]
        if all(x is not None for x in best):
            break
    return best


def test_parameters_are_part_of_a_captured_pass(pp, hip_lib):
    """set_soft_nms between two detect calls: the second result is the one for the new sigma -- the bytes of an engine
    that had it from the start, and the restatement's on the pass's own head maps -- not a replay of the first.  A network's
    scores cannot be drawn with margins, so the restatement is compared over each frame's longest run of first selections
    whose decisions all keep the 4e-4 margin (selection r and its score depend on the rounds before it only)."""
    def engine(sigma):
        cfg = pp.config.pedestrian_d435i_config(2)
        cfg["model"]["second"].update(use_soft_nms=True, soft_nms={"method": "gaussian", "sigma": sigma})
        e = pp.Engine(cfg, max_batch=2, max_points_per_frame=8192)
        e.load_weights(pp.weights.init_weights(e.d, seed=7))
        return e
    eng, other = engine(0.5), engine(0.1)
    try:
        assert eng.nms_mode == "soft" and eng.soft_nms["sigma"] == 0.5 and other.soft_nms["sigma"] == np.float32(0.1)
        rect, trv, _ = pp.synth.default_calib()
        rect, trv = np.stack([rect] * 2), np.stack([trv] * 2)
        compared = 0
        for seed in range(900, 908):
            frames = [pp.synth.d435i_cloud(seed + 10 * i, 4096) for i in range(2)]
            eng.set_soft_nms(sigma=0.5)
            d1, n1 = (a.copy() for a in eng.detect(frames, rect, trv))
            d1b, n1b = (a.copy() for a in eng.detect(frames, rect, trv))            # a replay
            assert np.array_equal(n1, n1b) and _kept_bytes(d1, n1) == _kept_bytes(d1b, n1b)
            eng.set_soft_nms(sigma=0.1)
            d2, n2 = (a.copy() for a in eng.detect(frames, rect, trv))
            o2, on2 = (a.copy() for a in other.detect(frames, rect, trv))
            assert np.array_equal(n2, on2) and _kept_bytes(d2, n2) == _kept_bytes(o2, on2)
            assert _kept_bytes(d2, n2) != _kept_bytes(d1, n1)
            im = eng.intermediates()
            found = _margin_safe_prefix(_example(eng.anchors, im["anchors_mask"], rect, trv), im, eng.d.nms_dict(),
                                        "gaussian", 0.1, 0.001)
            rows = [0 if r is None else len(r["anchor_index"]) for r in found]
            decayed = sum(0 if r is None else int((r["scores"] < r["sigmoid"]).sum()) for r in found)
            print(f"clouds {seed}: kept {n2.tolist()}, rows whose decisions keep the margin {rows}, {decayed} of them decayed")
            if sum(rows) >= 4 and decayed >= 1:
                for b, r in enumerate(found):
                    if r is not None:
                        assert int(n2[b]) >= len(r["anchor_index"])
                        _assert_soft(d2[b:b + 1], [len(r["anchor_index"])], [r], f"detect, sigma 0.1, clouds {seed}, frame {b}")
                compared += 1
                break
        assert compared == 1, "no cloud pair whose first selections keep every decision 4e-4 from flipping"
        # refused arguments leave the settings as they were
        before = eng.soft_nms
        L, h = eng._lib, eng._h
        import ctypes
        f = ctypes.c_float
        for m, sg, fl in ((3, 0.5, 0.001), (-1, 0.5, 0.001), (2, 0.0, 0.001), (2, -1.0, 0.001), (2, float("nan"), 0.001),
                          (2, float("inf"), 0.001), (2, 0.5, -0.001), (2, 0.5, float("nan")), (2, 0.5, float("inf"))):
            assert L.pp_set_soft_nms(h, m, f(sg), f(fl)) == 1, (m, sg, fl)        # PP_ERR_ARG
            assert eng.soft_nms == before
        with pytest.raises(ValueError):
            eng.set_soft_nms(method="median")
        with pytest.raises(ValueError):
            eng.set_soft_nms(sigma=0.0)
        assert eng.soft_nms == before
        # soft re-scoring on the rotated overlap is not built: refused by name, the mode stays
        with pytest.raises(RuntimeError, match="rotated"):
            eng.set_nms_mode("rotated")
        assert eng.nms_mode == "soft"
        with pytest.raises(ValueError):
            eng.set_nms_mode("polygon")
    finally:
        eng.close()
        other.close()


def test_config_keys_equal_the_setters(pp, hip_lib):
    cfg = _tiny_cfg(pp, 60, 20)
    cfg["model"]["second"].update(use_soft_nms=True, soft_nms={"method": "linear", "sigma": 0.3, "score_floor": 0.01})
    a = pp.Engine(cfg, max_batch=3, max_points_per_frame=4096)
    b = pp.Engine(_tiny_cfg(pp, 60, 20), max_batch=3, max_points_per_frame=4096)
    try:
        assert a.nms_mode == "soft" and b.nms_mode == "standup"
        assert a.soft_nms == {"method": "linear", "sigma": np.float32(0.3), "score_floor": np.float32(0.01)}
        b.set_soft_nms("linear", 0.3, 0.01)
        b.set_nms_mode("soft")
        inputs = _predict_inputs(pp, a.d, 4000)
        adets, an = a.predict(*inputs)
        bdets, bn = b.predict(*inputs)
        assert min(int(an[0]), int(an[1])) > 1
        assert np.array_equal(an, bn) and _kept_bytes(adets, an) == _kept_bytes(bdets, bn)
    finally:
        a.close()
        b.close()
    net = pp.VoxelNet(cfg, max_batch=3, max_points_per_frame=4096)
    try:
        assert net.engine.nms_mode == "soft" and net.engine.soft_nms["method"] == "linear"
    finally:
        net.engine.close()
