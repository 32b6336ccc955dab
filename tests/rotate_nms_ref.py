"""Host restatement of the rotated NMS (no GPU): rotate_nms_gpu -> rotate_nms_kernel -> nms_postprocess
(second/core/non_max_suppression/nms_gpu.py:419-490, :111-128) on the project's C twin of devRotateIoU, and a
predict() that follows oracle.ref_numpy.predict step for step except for the boxes handed to NMS.
tests/test_rotate_nms_host.py pins it to the reference's keep lists (tests/golden/ref_rotate_nms.npz)."""
import numpy as np

from oracle import c_oracle, ref_numpy as rn


def sorted_iou(boxes5):
    """iou[i][j] = devRotateIoU(box_i, box_j): the oracle's query is the first argument."""
    b = np.ascontiguousarray(boxes5, dtype=np.float32)
    return c_oracle.rotate_iou_eval(b, b, -1).T


def rotate_nms_mask(boxes5, thr):
    """rotate_nms_kernel: uint64 [n * col_blocks]; bit j % 64 of word (i, j // 64) iff j > i and IoU(i, j) > thr."""
    n = boxes5.shape[0]
    cb = -(-n // 64)
    over = sorted_iou(boxes5) > np.float32(thr)       # a NaN IoU compares False
    mask = np.zeros((n * cb,), dtype=np.uint64)
    for i in range(n):
        for j in np.nonzero(over[i, i + 1:])[0] + i + 1:
            mask[i * cb + j // 64] |= np.uint64(1) << np.uint64(j % 64)
    return mask


def rotate_nms_ref(dets, thr, pre_max_size=None, post_max_size=None):
    """Indices into dets of the kept boxes (int64), with the caps of nms() (libraries/eval_helper_functions.py:463-492);
    ties in the scores: lower index first."""
    dets = np.asarray(dets, dtype=np.float32).reshape(-1, 6)
    order = np.argsort(-dets[:, 5].astype(np.float64), kind="stable")
    if pre_max_size is not None and pre_max_size > 0:
        order = order[:min(len(order), pre_max_size)]
    n = len(order)
    if n == 0:
        return np.zeros((0,), np.int64)
    keep = rn.nms_postprocess(rotate_nms_mask(dets[order, :5], thr), n)
    if post_max_size is not None and post_max_size > 0:
        keep = keep[:post_max_size]
    return order[np.array(keep, dtype=np.int64)].astype(np.int64)


def min_margin(boxes5, thr):
    """Smallest |IoU - thr| over the ordered pairs of different boxes (inf without a finite one)."""
    iou = sorted_iou(boxes5).astype(np.float64)
    d = np.abs(iou[~np.eye(len(iou), dtype=bool)] - thr)
    d = d[np.isfinite(d)]
    return float(d.min()) if d.size else float("inf")


def predict_rotated(example, preds, cfg, margins=None):
    """oracle.ref_numpy.predict with the rotated rule: the boxes handed to NMS are box[:, [0, 1, 3, 4, 6]] before the
    direction flip (boxes_for_nms before its corner conversion, model/voxelnet.py:1233).  Each frame's dict also carries
    `anchor_index`.  margins (a list): receives every frame's min_margin over the boxes that entered the NMS."""
    anchors_b = example[6]
    B = anchors_b.shape[0]
    rect_b, trv_b, mask_b, idx_b = example[3], example[4], example[7], example[8]
    box_b = np.reshape(preds["box_preds"], (B, -1, 7))
    ncls = int(cfg.get("num_class", 1))
    use_dir = bool(cfg.get("use_direction_classifier", True))
    cls_b = np.reshape(preds["cls_preds"], (B, -1, ncls))
    dir_b = np.reshape(preds["dir_cls_preds"], (B, -1, 2)) if use_dir else [None] * B
    out = []
    for b in range(B):
        sel = np.where(mask_b[b] == 1)[0]
        box, cls, anc = box_b[b][sel], cls_b[b][sel], anchors_b[b][sel]
        dir_labels = np.argmax(dir_b[b][sel], axis=-1) if use_dir else np.zeros(box.shape[0], dtype=np.int64)
        total = rn.sigmoid_array(cls)
        if ncls == 1:
            scores = np.squeeze(total, axis=-1)
            labels = np.zeros(scores.shape[0], dtype=int)
        else:
            scores = total.max(axis=-1)
            labels = np.argmax(total, axis=-1)
        thr = cfg["nms_score_threshold"]
        if thr > 0.0:
            k = scores >= thr
            scores, box, anc, dir_labels, labels, sel = scores[k], box[k], anc[k], dir_labels[k], labels[k], sel[k]
        n_top = np.minimum(len(scores), 100)
        top = np.argpartition(scores, -n_top)[-n_top:] if len(scores) else np.zeros((0,), dtype=np.int64)
        scores, box, anc, dir_labels, labels, sel = scores[top], box[top], anc[top], dir_labels[top], labels[top], sel[top]
        selected = np.zeros((0,), np.int64)
        if scores.shape[0] != 0:
            box = rn.second_box_decode(box, anc)
            dets = np.concatenate([box[:, [0, 1, 3, 4, 6]], scores[:, None]], axis=1).astype(np.float32)
            selected = rotate_nms_ref(dets, cfg["nms_iou_threshold"], cfg["nms_pre_max_size"], cfg["nms_post_max_size"])
            if margins is not None:
                order = np.argsort(-dets[:, 5].astype(np.float64), kind="stable")[:max(cfg["nms_pre_max_size"], 0) or None]
                margins.append(min_margin(dets[order, :5], cfg["nms_iou_threshold"]))
        elif margins is not None:
            margins.append(float("inf"))
        if len(selected):
            fbox = box[selected]
            fdir = dir_labels[selected]
            if use_dir:
                opp = ((fbox[..., -1] > 0) ^ fdir) > 0
                fbox[..., -1] += np.where(opp, np.pi, 0.0)
            out.append({"box3d_camera": rn.box_lidar_to_camera(fbox, rect_b[b], trv_b[b]), "box3d_lidar": fbox,
                        "scores": scores[selected], "label_preds": labels[selected], "anchor_index": sel[selected],
                        "batch_idx": idx_b[b]})
        else:
            out.append({"box3d_camera": None, "box3d_lidar": None, "scores": None, "label_preds": None,
                        "anchor_index": np.zeros((0,), np.int64), "batch_idx": idx_b[b]})
    return out
