"""Host restatement of the detector's soft mode (no GPU): oracle.ref_numpy.predict step for step, with
pp_amd.soft_nms.soft_nms_np on the stand-up boxes in place of nms().  tests/test_soft_nms_host.py pins soft_nms_np to the
reference's soft_nms_jit (tests/golden/ref_soft_nms.npz).

The candidates are put in the kernel's order -- descending score, equal scores by ascending anchor index -- before the
top 100 are taken, so that the rule's tie-break ("the earlier box wins") means the same on both sides."""
import numpy as np

import pp_amd
from oracle import ref_numpy as rn

sn = pp_amd.soft_nms


def predict_soft(example, preds, cfg, method="gaussian", sigma=0.5, score_floor=0.001, margins=None):
    """One dict per frame: anchor_index, scores (decayed), sigmoid (the kept boxes' scores before any decay),
    label_preds, box3d_lidar, box3d_camera (None / empty for an empty frame).  margins (a list) receives every frame's
    soft_nms.decision_margins dict."""
    anchors_b = example[6]
    B = anchors_b.shape[0]
    rect_b, trv_b, mask_b, idx_b = example[3], example[4], example[7], example[8]
    box_b = np.reshape(preds["box_preds"], (B, -1, 7))
    ncls = int(cfg.get("num_class", 1))
    use_dir = bool(cfg.get("use_direction_classifier", True))
    cls_b = np.reshape(preds["cls_preds"], (B, -1, ncls))
    dir_b = np.reshape(preds["dir_cls_preds"], (B, -1, 2)) if use_dir else [None] * B
    pre, post, nt = cfg["nms_pre_max_size"], cfg["nms_post_max_size"], cfg["nms_iou_threshold"]
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
        top = np.lexsort((sel, -scores.astype(np.float64)))[:100]
        scores, box, anc, dir_labels, labels, sel = scores[top], box[top], anc[top], dir_labels[top], labels[top], sel[top]
        keep = np.zeros((0,), np.int64)
        if scores.shape[0] != 0:
            box = rn.second_box_decode(box, anc)
            bev = box[..., [0, 1, 3, 4, 6]]
            standup = rn.corner_to_standup(rn.center_to_corner_box2d(bev[:, :2], bev[:, 2:4], bev[:, 4]))
            dets = np.concatenate([standup, scores[:, None]], axis=1).astype(np.float32)
            keep, final = sn.soft_nms_np(dets, method, sigma, nt, score_floor, pre, post)
            if margins is not None:
                margins.append(sn.decision_margins(dets, method, sigma, nt, score_floor, pre, post))
        elif margins is not None:
            margins.append({"gap": float("inf"), "iou": float("inf"), "floor": float("inf"), "decays": np.zeros((0,), np.int64)})
        if len(keep):
            fbox = box[keep]
            fdir = dir_labels[keep]
            if use_dir:
                opp = ((fbox[..., -1] > 0) ^ fdir) > 0
                fbox[..., -1] += np.where(opp, np.pi, 0.0)
            out.append({"box3d_camera": rn.box_lidar_to_camera(fbox, rect_b[b], trv_b[b]), "box3d_lidar": fbox,
                        "scores": final, "sigmoid": scores[keep], "label_preds": labels[keep], "anchor_index": sel[keep],
                        "batch_idx": idx_b[b]})
        else:
            out.append({"box3d_camera": None, "box3d_lidar": None, "scores": None, "sigmoid": None, "label_preds": None,
                        "anchor_index": np.zeros((0,), np.int64), "batch_idx": idx_b[b]})
    return out


def margins_above(margins, bound):
    """Every frame's three decision margins above `bound`."""
    return all(min(m["gap"], m["iou"], m["floor"]) > bound for m in margins)
