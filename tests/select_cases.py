"""Inputs built to break the detector's candidate selection (csrc/postprocess.hip), shared by tests/test_select_host.py
(which asserts every fixture condition without a GPU) and tests/test_gpu_select.py (which runs them).

A case is a dict: `logit` [A, num_class] float32 and `mask` [A] uint8 of the adversarial frame, `top` -- the anchors the
tie rule (descending logit, +0.0 before -0.0, then lower anchor index) selects, written down from the construction and
not computed by the reference -- and `ncand`, the number of candidates the construction promises.  `batch` puts the
case into frame 0 of a two-frame batch whose frame 1 is a benign random map with another mask.
"""
import copy

import numpy as np

import pp_amd as pp

CCAP, KMAX, KTOP = 12288, 128, 100      # csrc/postprocess.hip; tests/test_select_host.py reads them from the source
U32, F32 = np.uint32, np.float32

# nothing is suppressed (strict `>` against 1.0) and no cap bites: the output rows are the selected 100 in rank order
TRANSPARENT = {"nms_iou_threshold": 1.0, "nms_pre_max_size": 100, "nms_post_max_size": 100}


def _nms(cfg, nms):
    s = cfg["model"]["second"]
    for k, v in nms.items():
        assert k in s, k
        s[k] = v
    return cfg


def grid_g_config(batch=2, num_class=1, **nms):
    """cfg-A on an 80 x 80 map: 12800 anchors, the smallest grid above CCAP (range and anchor offsets follow the map as
    in test_small_map_split_k_kernel_ragged_tiles)."""
    cfg = copy.deepcopy(pp.config.pedestrian_d435i_config(batch))
    cfg["eval_input_reader"]["feature_map_size"] = [1, 80, 80]
    s = cfg["model"]["second"]
    s["num_class"] = int(num_class)
    s["voxel_generator"].update(point_cloud_range=[0, -3.2, -3.0, 6.4, 3.2, 3.0])
    s["target_assigner"]["anchor_generators"]["anchor_generator_stride"].update(offsets=[0.08, -3.2, -1.465])
    return _nms(cfg, nms)


def kitti_config(batch=2, num_class=1, **nms):
    return _nms(pp.config.kitti_shaped_config(batch, num_class=num_class), nms)


def derived(cfg):
    d = pp.config.Derived(cfg)
    return d, pp.anchors.build_anchors(d)


# ---------------------------------------------------------------------------------------------- frames and batches
def _scatter(rng, A, n):
    return np.sort(rng.choice(A, int(n), replace=False))


def _filler(rng, A, lo, hi):
    return rng.uniform(lo, hi, A).astype(F32)


def _case(logit, mask, top, ncand=None, **extra):
    logit = np.ascontiguousarray(logit, dtype=F32)
    if logit.ndim == 1:
        logit = logit[:, None]
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    c = {"logit": logit, "mask": mask, "top": np.asarray(top, np.int64),
         "ncand": int(mask.sum()) if ncand is None else int(ncand)}
    c.update(extra)
    return c


def benign_frame(d, rng):
    A = d.num_anchors
    return (rng.standard_normal((A, d.num_class)) * 0.8).astype(F32), (rng.random(A) < 0.5).astype(np.uint8)


def batch(d, anchors, case, seed=0):
    """(example, preds) as oracle.ref_numpy.predict takes them: frame 0 the case, frame 1 benign.  box_preds are small
    random values, dir_cls_preds random with no equal pair."""
    rng = np.random.default_rng(1000 + seed)
    H, W, k = d.head_h, d.head_w, d.num_anchor_per_loc
    lg1, m1 = benign_frame(d, rng)
    cls = np.stack([case["logit"], lg1]).reshape(2, H, W, k * d.num_class)
    mask = np.stack([case["mask"], m1])
    box = (rng.standard_normal((2, H, W, k * 7)) * 0.1).astype(F32)
    dr = rng.standard_normal((2, H, W, k * 2)).astype(F32)
    pairs = dr.reshape(-1, 2)
    assert (pairs[:, 0] != pairs[:, 1]).all()
    rect, trv, _ = pp.synth.default_calib()
    ex = (None, None, None, np.stack([rect] * 2), np.stack([trv] * 2), None, np.stack([anchors] * 2), mask,
          np.arange(2), None)
    return ex, {"box_preds": box, "cls_preds": np.ascontiguousarray(cls), "dir_cls_preds": dr}


# ---------------------------------------------------------------------------------------------- cases, any grid
def counts(d, n):
    """Exactly n candidates by mask, distinct logits: `!found` (n < 100), "take them all", the first real cut (101)."""
    rng = np.random.default_rng(10 + n)
    A = d.num_anchors
    lg = rng.standard_normal(A).astype(F32)
    idx = _scatter(rng, A, n)
    assert len(np.unique(lg[idx])) == n
    mask = np.zeros(A, np.uint8)
    mask[idx] = 1
    return _case(lg, mask, idx[np.argsort(-lg[idx].astype(np.float64))][:KTOP], n)


def all_equal(d, ncand):
    """One logit everywhere, `ncand` anchors masked in: the floor key of the re-scan is made of index bits only."""
    rng = np.random.default_rng(20 + ncand)
    A = d.num_anchors
    mask = np.ones(A, np.uint8)
    mask[rng.choice(A, A - ncand, replace=False)] = 0
    return _case(np.full(A, 0.75, F32), mask, np.nonzero(mask)[0][:KTOP], ncand)


def ties_across_cut(d, pre=KTOP):
    """60 scattered anchors at 2.0, 500 at 1.0, the rest below, all masked in: the 60, then the 40 lowest of the 500."""
    rng = np.random.default_rng(30)
    A = d.num_anchors
    lg = _filler(rng, A, -3.0, 0.5)
    idx = rng.choice(A, 560, replace=False)
    hi, mid = np.sort(idx[:60]), np.sort(idx[60:])
    lg[hi], lg[mid] = 2.0, 1.0
    return _case(lg, np.ones(A, np.uint8), np.concatenate([hi, mid[:40]])[:pre], A)


def _placed(d, values, fill_lo, fill_hi, seed, thin):
    """`values` at scattered anchors in random order over a filler strictly below them; thin: ~60 % of the filler is
    masked out (the candidates then fit the LDS), else every anchor is a candidate (more than CCAP on grid G).  The
    expected top is the stable descending sort of the placed values: equal values by anchor index."""
    rng = np.random.default_rng(seed)
    A = d.num_anchors
    values = np.asarray(values, F32)
    assert fill_hi < values.min()
    lg = _filler(rng, A, fill_lo, fill_hi)
    idx = _scatter(rng, A, len(values))
    lg[idx] = values[rng.permutation(len(values))]
    mask = np.ones(A, np.uint8)
    if thin:
        mask = (rng.random(A) < 0.4).astype(np.uint8)
        mask[idx] = 1
    v = lg[idx]
    order = np.lexsort((idx, np.signbit(v), -v.astype(np.float64)))
    return _case(lg, mask, idx[order][:KTOP])


def _run(first_bits, n=300, copies=3):
    """n consecutive float32 values from the one with bit pattern first_bits (increasing magnitude), `copies` anchors
    each: the cut lands inside a group of equal keys."""
    v = (U32(first_bits) + np.arange(n, dtype=U32)).view(F32)
    return np.repeat(v, copies)


def radix(d, name, thin):
    one, mone, two = (int(np.array(x, F32).view(U32)) for x in (1.0, -1.0, 2.0))
    rng = np.random.default_rng(40)
    if name == "up_from_1":          # differ in the lowest mantissa byte only (and one carry into the next)
        return _placed(d, _run(one), -3.0, 0.5, 41, thin)
    if name == "down_from_-1":       # the inverted branch of comp_key
        v = _run(mone)
        assert (v <= -1.0).all()
        return _placed(d, v, -60.0, -50.0, 42, thin)
    if name == "across_2":           # 150 values below 2.0, 150 from it upward: the exponent changes inside the run
        return _placed(d, _run(two - 150), -3.0, 0.5, 43, thin)
    if name == "signs_zeros_subnormals":
        sub = rng.integers(1, 0x7fffff, 20).astype(U32)
        nsub = (rng.integers(1, 0x7fffff, 30).astype(U32) | U32(0x80000000))
        v = np.concatenate([rng.uniform(0.1, 5.0, 40).astype(F32), sub.view(F32), np.full(30, 0.0, F32),
                            np.full(30, -0.0, F32), nsub.view(F32), rng.uniform(-5.0, -0.1, 50).astype(F32)])
        c = _placed(d, v, -60.0, -50.0, 44, thin)
        t = c["logit"][c["top"], 0]      # 40 + 20 positive, the 30 +0.0, then the 10 lowest-index -0.0
        assert (t[:60] > 0).all() and (t[60:] == 0).all()
        assert not np.signbit(t[60:90]).any() and np.signbit(t[90:]).all()
        return c
    if name == "saturating":         # float32 scores 1.0 (logit >= 17) and 0.0 (-100) while the logits stay ordered
        v = np.repeat(np.array([100, 80, 20, 18, 17.5, 17, -17, -20, -80, -100], F32), 12)
        c = _placed(d, v, -300.0, -200.0, 45, thin)
        t = c["logit"][c["top"], 0]
        assert (t[:72] >= 17).all() and (t[72:84] == -17).all() and (t[84:96] == -20).all() and (t[96:] == -80).all()
        return c
    if name in ("bucket_100", "bucket_101"):
        # [2, 8) is one value of the key's top byte (0xc0) and everything below 2 lies in lower ones: pass 0 of the
        # select meets s_hist[digit] == need with 100 keys there, and has to go on with 101
        n = int(name[-3:])
        v = rng.uniform(2.0, 7.99, n).astype(F32)
        assert len(np.unique(v)) == n and ((v.view(U32) >> U32(24)) == 0x40).all()
        return _placed(d, v, -3.0, 1.9, 46 + n, thin)
    raise ValueError(name)


RADIX = ("up_from_1", "down_from_-1", "across_2", "signs_zeros_subnormals", "saturating", "bucket_100", "bucket_101")


def threshold_edge(d, few):
    """nms_score_threshold = 0.5: +0.0, -0.0 and the first float32 on either side of zero all score exactly 0.5 and
    `>=` keeps them; the rest of the map is positive (kept) or negative (dropped), at least 0.01 from zero."""
    rng = np.random.default_rng(50 + int(few))
    A = d.num_anchors
    npos, nz, nt = (20, 5, 5) if few else (50, 30, 10)
    tiny = np.array(1, U32).view(F32)
    lg = _filler(rng, A, -3.0, -0.01)
    idx = rng.choice(A, npos + 2 * nz + 2 * nt, replace=False)
    parts = np.split(idx, np.cumsum([npos, nt, nz, nz]))
    pos, ptiny, pz, nzr, ntiny = (np.sort(p) for p in parts)
    lg[pos] = rng.uniform(0.01, 3.0, npos).astype(F32)
    lg[ptiny], lg[pz], lg[nzr], lg[ntiny] = tiny, 0.0, -0.0, -tiny
    assert len(np.unique(lg[pos])) == npos
    top = np.concatenate([pos[np.argsort(-lg[pos].astype(np.float64))], ptiny, pz, nzr, ntiny])
    return _case(lg, np.ones(A, np.uint8), top[:KTOP], len(top), edge=np.concatenate([ptiny, pz, nzr, ntiny]))


def classes(d):
    """Several classes: the anchor's largest class logit follows `ties_across_cut`; a random non-empty set of classes
    attains it (label = the first of them), the others lie 0.5 .. 2 below.  `top` is the joint mode's."""
    rng = np.random.default_rng(60 + d.num_class)
    base = ties_across_cut(d)
    A, C = d.num_anchors, d.num_class
    m = base["logit"][:, 0]
    at_max = rng.random((A, C)) < 0.6
    at_max[np.arange(A), rng.integers(0, C, A)] = True
    lg = np.where(at_max, m[:, None], m[:, None] - rng.uniform(0.5, 2.0, (A, C)).astype(F32)).astype(F32)
    return _case(lg, base["mask"], base["top"], A, label=np.argmax(at_max, axis=1))


# ---------------------------------------------------------------------------------------------- cases for cfg-K
def order_adversarial(d, name):
    """Every anchor a candidate (several multiples of CCAP).  `ascending`: the best are scanned last, so the floor taken
    from the first-stored CCAP keys leaves far more than CCAP keys at or above it -- the input of the third selection
    path, for any plausible wavefront order."""
    A = d.num_anchors
    a = np.arange(A)
    if name in ("ascending", "descending"):
        lg = np.linspace(-4.0, 4.0, A).astype(F32)
        assert (np.diff(lg) > 0).all()
        if name == "descending":
            lg = lg[::-1]
        top = np.argsort(-lg.astype(np.float64), kind="stable")[:KTOP]
    elif name == "sawtooth":         # period 1000: every value at 107 or 108 anchors
        lg = ((a % 1000) * 0.005 - 2.0).astype(F32)
        top = a[a % 1000 == 999][:KTOP]
        assert len(top) == KTOP
    elif name == "plateaus":         # ascending in plateaus of 1000 equal values; the last one has A % 1000 anchors
        lg = ((a // 1000) * 0.05 - 2.0).astype(F32)
        assert (np.diff(np.unique(lg)) > 0).all() and len(np.unique(lg)) == -(-A // 1000)
        top = a[a // 1000 == (A - 1) // 1000][:KTOP]
        assert len(top) == KTOP
    else:
        raise ValueError(name)
    return _case(lg, np.ones(A, np.uint8), top, A)


ORDERS = ("ascending", "descending", "sawtooth", "plateaus")


# ---------------------------------------------------------------------------------------------- the fused path
def zero_weights(d, cls_bias, dir_bias):
    """Weights whose every convolution and deconvolution kernel is zero and whose normalisations map zero to zero: every
    logit of a frame is the rpn/conv_cls bias of its (anchor-in-location, class) slot, exactly."""
    w = pp.weights.init_weights(d, seed=1)
    for k in w:
        if k.endswith("/gamma") or k.endswith("/moving_variance"):
            w[k] = np.ones_like(w[k])
        else:
            w[k] = np.zeros_like(w[k])
    w["rpn/conv_cls/bias"] = np.asarray(cls_bias, F32).reshape(w["rpn/conv_cls/bias"].shape)
    w["rpn/conv_dir_cls/bias"] = np.asarray(dir_bias, F32).reshape(w["rpn/conv_dir_cls/bias"].shape)
    return w


def uniform_frames(d, counts_, seed=70):
    lo, hi = d.pc_range[:3], d.pc_range[3:]
    out = []
    for i, n in enumerate(counts_):
        rng = np.random.default_rng(1000 * seed + i)
        xyz = rng.uniform(lo, hi, (n, 3))
        extra = rng.uniform(0, 1, (n, d.num_point_features - 3))
        out.append(np.concatenate([xyz, extra], axis=1).astype(F32))
    return out


# slot-major [anchor-in-location, class] biases of the two-class cfg-K head
BIASES_K = {"all_equal": [[0.25, 0.25], [0.25, 0.25]],
            "class1_above": [[0.25, 0.75], [0.25, 0.75]],
            "slot1_above": [[0.25, 0.25], [0.75, 0.75]]}
DIR_BIAS = [[0.1, 0.3], [0.4, 0.2]]      # dir label 1 for slot 0, 0 for slot 1
FUSED_K_POINTS = [20000] * 3 + [0] + [20000] * 5 + [400] + [20000] * 22        # B = 32: frame 3 empty, frame 9 sparse
FUSED_A_POINTS = [16384] * 5 + [0] + [16384] * 4 + [7] + [16384] * 53        # B = 64


def fused_expected(mask, cls_bias):
    """(anchors, labels) the tie rule selects from one frame's anchor mask when every logit is its slot's bias."""
    bias = np.asarray(cls_bias, F32)
    k = bias.shape[0]
    cand = np.nonzero(np.asarray(mask) == 1)[0]
    val = bias.max(axis=1)[cand % k]
    top = cand[np.lexsort((cand, -val.astype(np.float64)))][:KTOP]
    return top, np.argmax(bias, axis=1)[top % k]


# ---------------------------------------------------------------------------------------------- the catalogue
def _t(**over):
    return dict(TRANSPARENT, **over)


# id -> (num_class, NMS settings over the config's, builder(d)); all through Engine.predict on grid G
CASES_G = {}
for _n in (0, 1, 99, 100, 101):
    CASES_G[f"counts_{_n}"] = (1, _t(), lambda d, n=_n: counts(d, n))
for _n in (12800, CCAP - 1, CCAP, CCAP + 1):
    CASES_G[f"all_equal_{_n}"] = (1, _t(), lambda d, n=_n: all_equal(d, n))
CASES_G["ties_across_cut"] = (1, _t(), ties_across_cut)
CASES_G["ties_across_cut_pre30"] = (1, _t(nms_pre_max_size=30), lambda d: ties_across_cut(d, 30))
for _name in RADIX:
    for _thin in (True, False):
        CASES_G[f"radix_{_name}_{'thin' if _thin else 'full'}"] = (1, _t(), lambda d, a=_name, b=_thin: radix(d, a, b))
CASES_G["threshold_edge"] = (1, _t(nms_score_threshold=0.5), lambda d: threshold_edge(d, False))
CASES_G["threshold_edge_few"] = (1, _t(nms_score_threshold=0.5), lambda d: threshold_edge(d, True))
CASES_G["classes_2"] = (2, _t(), classes)
CASES_G["classes_3"] = (3, _t(), classes)

# cfg-K, selection-transparent: several multiples of CCAP candidates in adversarial orders
CASES_K = {name: (1, _t(), lambda d, a=name: order_adversarial(d, a)) for name in ORDERS}

# cfg-K under the config's own thresholds (iou 0.5, pre 100, post 50), every suppression rule: map -> (builder, the seed
# of `batch` -- chosen on the host so that every decision margin of postprocess_ref.predict is above MARGIN)
MARGIN = 1e-4
RULES = ("standup", "rotated", "soft")
RULE_MAPS_K = {"plateaus": (lambda d: order_adversarial(d, "plateaus"), 0), "ties_across_cut": (ties_across_cut, 0)}
