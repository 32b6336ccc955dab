"""Host reference of the detector's post-process with the tie order defined (no GPU).

oracle.ref_numpy.predict picks its candidates with np.argpartition and argsort()[::-1] on float32 scores; what those do
with equal scores is implementation-defined, so every test built on it keeps its scores distinct.  The kernel
(csrc/postprocess.hip) does define the order, through its 64-bit comp_key, and `predict` below restates
oracle.ref_numpy.predict with that rule in place of the two implementation-defined steps:

    candidates   mask byte == 1, then float32 sigmoid(logit) >= nms_score_threshold (when the threshold is > 0)
    order        logit descending as a float value; +0.0 before -0.0; anchor index ascending
    selection    the first 100 of that order, then the first min(100, nms_pre_max_size)

The logit of an anchor: its largest class logit, label = first maximum (joint mode); class c's logit alone, label c, once
per class and laid end to end as tests/class_nms_ref.py does (per_class mode).  Everything after the selection is the
oracle's own code on boxes already in that order, with no argsort inside: second_box_decode, center_to_corner_box2d,
corner_to_standup, nms_mask, nms_postprocess, the direction flip and box_lidar_to_camera.  The rotated and soft rules
hand the same ordered set to tests/rotate_nms_ref.py and pp_amd.soft_nms.soft_nms_np, which already break ties "lower
index first".

The order is a refinement of the oracle's: sigmoid is monotone, so descending logit is non-increasing float32 score, and
where the float32 scores are pairwise distinct the two agree (tests/test_select_host.py holds both to that).
"""
import numpy as np

from oracle import ref_numpy as rn

KTOP = 100     # model/voxelnet.py:1207 (hard-coded)


def sigmoid32(x):
    """rn.sigmoid_array on float32 logits; exp(-x) overflowing to inf (logit below about -88) gives score 0."""
    with np.errstate(over="ignore"):
        return rn.sigmoid_array(np.asarray(x, dtype=np.float32))


def candidate_order(logit, mask, thr):
    """Anchor indices of one frame's candidates in the kernel's order.  logit [A] float32, mask [A]."""
    logit = np.asarray(logit, dtype=np.float32)
    cand = np.nonzero(np.asarray(mask) == 1)[0]
    if thr > 0.0:
        cand = cand[sigmoid32(logit[cand]) >= thr]
    lg = logit[cand]
    # lexsort: last key first.  -lg compares +0.0 and -0.0 equal, the sign bit then puts +0.0 first
    return cand[np.lexsort((cand, np.signbit(lg), -lg.astype(np.float64)))]


def joint_logit(cls):
    """[A, ncls] -> (largest class logit [A], first maximum [A])."""
    lab = np.argmax(cls, axis=-1)
    return np.take_along_axis(cls, lab[:, None], axis=-1)[:, 0], lab


def _iou_matrix(standup):
    """rn.nms_iou for every pair, vectorised (float32 differences, float64 after the `+ 1`)."""
    b = np.asarray(standup, dtype=np.float32)
    one = np.float64(1.0)
    left, right = np.maximum(b[:, None, 0], b[None, :, 0]), np.minimum(b[:, None, 2], b[None, :, 2])
    top, bottom = np.maximum(b[:, None, 1], b[None, :, 1]), np.minimum(b[:, None, 3], b[None, :, 3])
    w = np.maximum((right - left).astype(np.float64) + one, 0.0)
    h = np.maximum((bottom - top).astype(np.float64) + one, 0.0)
    inter = w * h
    area = ((b[:, 2] - b[:, 0]).astype(np.float64) + one) * ((b[:, 3] - b[:, 1]).astype(np.float64) + one)
    return inter / (area[:, None] + area[None, :] - inter)


def _sweep_margin(iou, keep, thr):
    """Smallest |IoU - thr| over the pairs the greedy sweep compares: (i, j > i) for every kept row i."""
    thr = np.float64(np.float32(thr))
    best = float("inf")
    for i in keep:
        row = iou[i, i + 1:]
        row = row[np.isfinite(row)]
        if row.size:
            best = min(best, float(np.abs(row - thr).min()))
    return best


def _single(order, box_all, anchors, cfg, rule, soft):
    """NMS and what follows it for one ordered candidate list.  Returns (rows into `order` that are kept, decoded boxes
    of the top set, final scores or None, iou margin, floor margin)."""
    pre, post, nt = cfg["nms_pre_max_size"], cfg["nms_post_max_size"], cfg["nms_iou_threshold"]
    box = rn.second_box_decode(box_all[order], anchors[order])
    n = min(len(order), pre)
    inf = float("inf")
    if rule == "rotated":
        import rotate_nms_ref as rr
        b5 = np.ascontiguousarray(box[:n][:, [0, 1, 3, 4, 6]], dtype=np.float32)
        keep = rn.nms_postprocess(rr.rotate_nms_mask(b5, nt), n)[:post]
        return np.array(keep, np.int64), box, None, _sweep_margin(rr.sorted_iou(b5).astype(np.float64), keep, nt), inf
    bev = box[:n][:, [0, 1, 3, 4, 6]]
    standup = rn.corner_to_standup(rn.center_to_corner_box2d(bev[:, :2], bev[:, 2:4], bev[:, 4]))
    if rule == "soft":
        import pp_amd
        sn = pp_amd.soft_nms
        dets = np.concatenate([standup, soft["scores"][:n, None]], axis=1).astype(np.float32)
        args = (dets, soft["method"], soft["sigma"], nt, soft["score_floor"], None, post)
        keep, final = sn.soft_nms_np(*args)
        dm = sn.decision_margins(*args)
        return keep, box, final, dm["iou"], dm["floor"]
    if rule != "standup":
        raise ValueError(rule)
    dets = np.concatenate([standup, np.zeros((n, 1), np.float32)], axis=1).astype(np.float32)
    keep = rn.nms_postprocess(rn.nms_mask(dets, nt), n)[:post]
    return np.array(keep, np.int64), box, None, _sweep_margin(_iou_matrix(standup), keep, nt), inf


def predict(example, preds, cfg, rule="standup", class_nms="joint", method="gaussian", sigma=0.5, score_floor=0.001):
    """One dict per frame: n, anchor_index, label, dir_label, score (float32 sigmoid; the decayed score under the soft
    rule), box3d_lidar, box3d_camera (arrays, length 0 for an empty frame), top (the selected <= 100 anchors in rank
    order; per_class: one array per class), iou_margin (smallest |IoU - nms_iou_threshold| over the pairs the sweep
    compares, inf where none is) and floor_margin (soft rule: smallest gap of a re-scored value to score_floor).
    example / preds / cfg as oracle.ref_numpy.predict takes them."""
    anchors_b = example[6]
    B = anchors_b.shape[0]
    rect_b, trv_b, mask_b = example[3], example[4], example[7]
    box_b = np.reshape(np.asarray(preds["box_preds"], np.float32), (B, -1, 7))
    ncls = int(cfg.get("num_class", 1))
    use_dir = bool(cfg.get("use_direction_classifier", True))
    cls_b = np.reshape(np.asarray(preds["cls_preds"], np.float32), (B, -1, ncls))
    dir_b = np.reshape(preds["dir_cls_preds"], (B, -1, 2)) if use_dir else None
    thr = cfg["nms_score_threshold"]
    out = []
    for b in range(B):
        if class_nms == "per_class":
            passes = [(cls_b[b][:, c], np.full((cls_b[b].shape[0],), c, np.int64)) for c in range(ncls)]
        elif class_nms == "joint":
            passes = [joint_logit(cls_b[b])]
        else:
            raise ValueError(class_nms)
        rows = {k: [] for k in ("anchor_index", "label", "dir_label", "score", "box3d_lidar", "box3d_camera")}
        tops, im, fm = [], float("inf"), float("inf")
        for logit, label in passes:
            order = candidate_order(logit, mask_b[b], thr)[:KTOP]
            tops.append(order)
            if len(order) == 0:
                continue
            scores = sigmoid32(logit[order])
            soft = {"scores": scores, "method": method, "sigma": sigma, "score_floor": score_floor}
            keep, box, final, m_iou, m_floor = _single(order, box_b[b], anchors_b[b], cfg, rule, soft)
            im, fm = min(im, m_iou), min(fm, m_floor)
            if len(keep) == 0:
                continue
            sel = order[keep]
            fbox = box[keep]
            fdir = np.argmax(dir_b[b][sel], axis=-1) if use_dir else np.zeros((len(sel),), np.int64)
            if use_dir:
                opp = ((fbox[..., -1] > 0) ^ fdir) > 0       # model/voxelnet.py:1305 precedence
                fbox[..., -1] += np.where(opp, np.pi, 0.0)
            rows["anchor_index"].append(sel.astype(np.int64))
            rows["label"].append(np.asarray(label)[sel].astype(np.int64))
            rows["dir_label"].append(fdir.astype(np.int64))
            rows["score"].append(scores[keep] if final is None else final)
            rows["box3d_lidar"].append(fbox)
            rows["box3d_camera"].append(rn.box_lidar_to_camera(fbox, rect_b[b], trv_b[b]))
        empty = {"anchor_index": (0,), "label": (0,), "dir_label": (0,), "score": (0,), "box3d_lidar": (0, 7),
                 "box3d_camera": (0, 7)}
        fr = {k: (np.concatenate(v, axis=0) if v else np.zeros(empty[k])) for k, v in rows.items()}
        fr["n"] = len(fr["anchor_index"])
        fr["top"] = tops[0] if class_nms == "joint" else tops
        fr["iou_margin"], fr["floor_margin"] = im, fm
        out.append(fr)
    return out
