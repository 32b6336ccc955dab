"""Soft-NMS on the GPU (csrc/soft_nms.hip through pp_soft_nms) and its host restatement.

Replaces the reference's soft_nms_jit (second/core/non_max_suppression/nms_cpu.py:79-169), which it compiles and exports
but never calls, with the pre / post caps of nms() around it (libraries/eval_helper_functions.py:463-492).  The detector
uses the same rule inside its post-process with `Engine.set_nms_mode("soft")` / `Engine.set_soft_nms(...)` or the config
keys `model.second.use_soft_nms` and `model.second.soft_nms`.

The rule (numba's typing: float32 meeting an integer literal becomes float64).  Every box starts alive.  Each round selects
the alive box with the largest current score -- that score is final -- and re-scores every other alive box j whose overlap
with the selected box t has positive width and height under the `+1` pixel convention:

    iw = float64(float32(min(tx2, x2) - max(tx1, x1))) + 1, ih likewise; both > 0
    ua = (float64(tx2 - tx1) + 1) * (float64(ty2 - ty1) + 1) + (float64(x2 - x1) + 1) * (float64(y2 - y1) + 1) - iw * ih
    ov = iw * ih / ua
    weight = hard: 0 if ov > Nt else 1;  linear: 1 - ov if ov > Nt else 1;  gaussian: exp(-ov * ov / sigma)
    score_j = float32(weight * float64(score_j));  score_j < score_floor (float32): box j is dropped

The floor is checked only where a box was re-scored, weight 1 included: a box below the floor that overlaps no selected
box is kept.  Equal current scores: the box earlier in the input wins (the reference decides by array slot after its
in-place swaps and loses the original indices; neither is reproduced).
"""
import ctypes

import numpy as np

from . import _lib

MAX_BOXES = _lib.PP_SNMS_MAX_BOXES       # most boxes that enter the rounds (after pre_max_size)
METHODS = {"hard": _lib.PP_SOFT_NMS_HARD, "linear": _lib.PP_SOFT_NMS_LINEAR, "gaussian": _lib.PP_SOFT_NMS_GAUSSIAN}


def method_id(method):
    """'hard' / 'linear' / 'gaussian' or the reference's 0 / 1 / 2 -> 0 / 1 / 2."""
    if isinstance(method, str):
        if method not in METHODS:
            raise ValueError(f"method must be one of {sorted(METHODS)} (or 0, 1, 2), got {method!r}")
        return METHODS[method]
    if isinstance(method, (int, np.integer)) and not isinstance(method, bool) and int(method) in (0, 1, 2):
        return int(method)
    raise ValueError(f"method must be one of {sorted(METHODS)} (or 0, 1, 2), got {method!r}")


def check_params(sigma, score_floor, iou_threshold=0.0):
    sigma, score_floor, iou_threshold = float(sigma), float(score_floor), float(iou_threshold)
    if not (np.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f"sigma must be finite and > 0, got {sigma}")
    if not (np.isfinite(score_floor) and score_floor >= 0.0):
        raise ValueError(f"score_floor must be finite and >= 0, got {score_floor}")
    if not np.isfinite(iou_threshold):
        raise ValueError(f"iou_threshold must be finite, got {iou_threshold}")
    return sigma, score_floor, iou_threshold


def _checked(dets, method, sigma, iou_threshold, score_floor, pre_max_size, post_max_size):
    d = np.ascontiguousarray(dets, dtype=np.float32)
    if d.ndim != 2 or d.shape[1] != 5:
        raise ValueError(f"dets must be [N,5] (x1, y1, x2, y2, score), got {d.shape}")
    if not np.isfinite(d[:, 4]).all():
        raise ValueError("soft_nms: scores must be finite")
    sigma, score_floor, iou_threshold = check_params(sigma, score_floor, iou_threshold)
    pre = 0 if pre_max_size is None else int(pre_max_size)
    post = 0 if post_max_size is None else int(post_max_size)
    return d, method_id(method), sigma, iou_threshold, score_floor, pre, post


def soft_nms(dets, method="gaussian", sigma=0.5, iou_threshold=0.3, score_floor=0.001, pre_max_size=None,
             post_max_size=None, device=0):
    """dets [N,5] (x1, y1, x2, y2, score) -> (keep int64 indices into dets in selection order, their final float32
    scores, non-increasing).  pre_max_size: only the best that many by score enter (at most MAX_BOXES may);
    post_max_size: at most that many are returned; None (or <= 0): no cap."""
    d, m, sigma, nt, floor, pre, post = _checked(dets, method, sigma, iou_threshold, score_floor, pre_max_size, post_max_size)
    n = d.shape[0]
    keep = np.zeros((max(n, 1),), dtype=np.int32)
    scores = np.zeros((max(n, 1),), dtype=np.float32)
    nk = ctypes.c_int64(0)
    L = _lib.lib()
    st = L.pp_soft_nms(int(device), d.ctypes.data, n, m, ctypes.c_float(sigma), ctypes.c_float(nt), ctypes.c_float(floor),
                       pre, post, keep.ctypes.data, scores.ctypes.data, ctypes.byref(nk))
    if st != 0:
        msg = L.pp_last_error(None)
        cls = ValueError if st == 1 else RuntimeError
        raise cls(f"soft_nms: {msg.decode() if msg else st}")
    return keep[:nk.value].astype(np.int64), scores[:nk.value].copy()


def _rounds(d, m, sigma, nt, floor, pre, post, stats=None):
    n = d.shape[0]
    enter = np.arange(n)
    if 0 < pre < n:
        enter = np.sort(np.argsort(-d[:, 4].astype(np.float64), kind="stable")[:pre])   # the best by score, in input order
    box, s = d[enter, :4], d[enter, 4].copy()
    cap = len(enter) if post <= 0 else min(post, len(enter))
    alive = np.ones(len(enter), dtype=bool)
    decays = np.zeros(len(enter), dtype=np.int64)
    dnt, dsig, ffloor = np.float64(np.float32(nt)), np.float64(np.float32(sigma)), np.float32(floor)
    keep, out, kdec = [], [], []
    one = np.float64(1.0)
    while alive.any() and len(keep) < cap:
        cand = np.nonzero(alive)[0]
        t = cand[np.argmax(s[cand])]                       # first maximum: the lower index on ties
        if stats is not None and len(cand) > 1:
            top = np.sort(s[cand].astype(np.float64))
            stats["gap"] = min(stats["gap"], float(top[-1] - top[-2]))
        keep.append(enter[t]); out.append(s[t]); kdec.append(decays[t])
        alive[t] = False
        r = np.nonzero(alive)[0]
        if len(r) == 0:
            break
        b, tb = box[r], box[t]
        iw = (np.minimum(tb[2], b[:, 2]) - np.maximum(tb[0], b[:, 0])).astype(np.float64) + one     # float32 differences
        ih = (np.minimum(tb[3], b[:, 3]) - np.maximum(tb[1], b[:, 1])).astype(np.float64) + one
        hit = (iw > 0) & (ih > 0)
        if not hit.any():
            continue
        r, b, iw, ih = r[hit], b[hit], iw[hit], ih[hit]
        area = ((b[:, 2] - b[:, 0]).astype(np.float64) + one) * ((b[:, 3] - b[:, 1]).astype(np.float64) + one)
        tarea = (np.float64(tb[2] - tb[0]) + one) * (np.float64(tb[3] - tb[1]) + one)
        inter = iw * ih
        ov = inter / (tarea + area - inter)
        if m == 1:
            w = np.where(ov > dnt, one - ov, one)
        elif m == 2:
            w = np.exp(-(ov * ov) / dsig)
        else:
            w = np.where(ov > dnt, 0.0, one)
        new = (w * s[r].astype(np.float64)).astype(np.float32)
        if stats is not None:
            if m != 2:
                stats["iou"] = min(stats["iou"], float(np.abs(ov - dnt).min()))
            stats["floor"] = min(stats["floor"], float(np.abs(new.astype(np.float64) - np.float64(ffloor)).min()))
        s[r] = new
        decays[r] += 1
        alive[r[new < ffloor]] = False
    if stats is not None:
        stats["decays"] = np.array(kdec, dtype=np.int64)
    return np.array(keep, dtype=np.int64), np.array(out, dtype=np.float32)


def soft_nms_np(dets, method="gaussian", sigma=0.5, iou_threshold=0.3, score_floor=0.001, pre_max_size=None,
                post_max_size=None):
    """The host restatement of `soft_nms` (numpy, float64 where numba widens, the same tie rule and caps): the oracle of
    pp_soft_nms and of the detector's soft mode.  Same arguments, same return."""
    return _rounds(*_checked(dets, method, sigma, iou_threshold, score_floor, pre_max_size, post_max_size))


def decision_margins(dets, method="gaussian", sigma=0.5, iou_threshold=0.3, score_floor=0.001, pre_max_size=None,
                     post_max_size=None):
    """How far the restatement's decisions are from flipping, over the rounds it runs: dict with `gap`, the smallest
    difference between the two largest current scores at a selection; `iou`, the smallest |ov - Nt| over the re-scorings
    (inf for 'gaussian', whose weight does not look at Nt); `floor`, the smallest |re-scored value - score_floor|; and
    `decays` [kept], how often each returned box was re-scored.  inf where nothing was compared."""
    stats = {"gap": float("inf"), "iou": float("inf"), "floor": float("inf")}
    _rounds(*_checked(dets, method, sigma, iou_threshold, score_floor, pre_max_size, post_max_size), stats=stats)
    return stats
