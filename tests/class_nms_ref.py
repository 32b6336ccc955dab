"""Host oracle of the per-class post-process (model.second.use_multi_class_nms; no GPU).

The reference's predict() leaves this branch as `pass` (model/voxelnet.py:1170-1171), so nothing of the reference can be
run for it.  The rule is "the single pass of :1172-1286, once per class, on that class's score alone", and that single
pass is what oracle.ref_numpy.predict restates: `predict_per_class` calls it once per class with the class's logit
column as a one-class cls_preds and num_class = 1, sets the labels to the class and lays the classes' results end to
end.  `single` swaps the pass (tests/rotate_nms_ref.predict_rotated for the rotated rule)."""
import numpy as np

from oracle import ref_numpy as rn


def class_logits(preds, num_class):
    """[B, A, num_class] view of cls_preds (the reference reshapes to [B, -1, num_class], model/voxelnet.py:1090)."""
    cls = np.asarray(preds["cls_preds"])
    return cls.reshape(cls.shape[0], -1, num_class)


def _anchor_index(scores, logits, mask, thr):
    """The anchors a single-pass result came from: the candidate whose float32 sigmoid equals the returned score.  The
    oracle does not carry the index through its argpartition; the scores of the candidates that matter are distinct (the
    tests assert that first), so the score names the anchor."""
    cand = np.nonzero(mask == 1)[0]
    s_all = rn.sigmoid_array(logits[cand])
    if thr > 0.0:
        keep = s_all >= thr
        cand, s_all = cand[keep], s_all[keep]
    order = np.argsort(s_all, kind="stable")
    pos = np.searchsorted(s_all[order], scores)
    out = np.zeros((len(scores),), np.int64)
    for i, (p, s) in enumerate(zip(pos, scores)):
        hits = 0
        while p + hits < len(order) and s_all[order[p + hits]] == s:
            hits += 1
        assert hits == 1, f"score {s!r} names {hits} candidates: the recipe must keep the scores distinct"
        out[i] = cand[order[p]]
    return out


def predict_per_class(example, preds, cfg, single=rn.predict, **kw):
    """One dict per frame: scores, label_preds, anchor_index, dir_label, box3d_lidar, box3d_camera (arrays, length 0 for
    an empty frame) and class_counts [num_class] -- class 0's kept boxes in descending score, then class 1's, ..."""
    ncls = int(cfg["num_class"])
    one = dict(cfg, num_class=1)
    use_dir = bool(cfg.get("use_direction_classifier", True))
    logits = class_logits(preds, ncls)
    B = logits.shape[0]
    lead = np.asarray(preds["cls_preds"]).shape[:-1]
    mask_b = example[7]
    dirs = np.reshape(preds["dir_cls_preds"], (B, -1, 2)) if use_dir else None
    per_class = []
    for c in range(ncls):
        p = dict(preds, cls_preds=np.ascontiguousarray(logits[:, :, c]).reshape(lead + (-1,)))
        per_class.append(single(example, p, one, **kw))
    out = []
    for b in range(B):
        rows = {k: [] for k in ("scores", "label_preds", "anchor_index", "dir_label", "box3d_lidar", "box3d_camera")}
        counts = []
        for c in range(ncls):
            r = per_class[c][b]
            n = 0 if r["scores"] is None else len(r["scores"])
            counts.append(n)
            if n == 0:
                continue
            a = r["anchor_index"] if "anchor_index" in r else \
                _anchor_index(r["scores"], logits[b, :, c], mask_b[b], cfg["nms_score_threshold"])
            rows["scores"].append(r["scores"])
            rows["label_preds"].append(np.full((n,), c, np.int64))
            rows["anchor_index"].append(np.asarray(a, np.int64))
            rows["dir_label"].append(np.argmax(dirs[b][a], axis=-1) if use_dir else np.zeros((n,), np.int64))
            rows["box3d_lidar"].append(r["box3d_lidar"])
            rows["box3d_camera"].append(r["box3d_camera"])
        empty = {"scores": (0,), "label_preds": (0,), "anchor_index": (0,), "dir_label": (0,), "box3d_lidar": (0, 7),
                 "box3d_camera": (0, 7)}
        fr = {k: (np.concatenate(v, axis=0) if v else np.zeros(empty[k])) for k, v in rows.items()}
        fr["class_counts"] = np.array(counts, np.int64)
        out.append(fr)
    return out


def distinct_top_scores(preds, mask, num_class, top=200):
    """True when, per frame and class, the float32 sigmoid scores of the `top` best masked anchors are pairwise distinct
    (np.argpartition / argsort of the oracle are then free of ties)."""
    logits = class_logits(preds, num_class)
    for b in range(logits.shape[0]):
        on = mask[b] == 1
        for c in range(num_class):
            s = np.sort(rn.sigmoid_array(logits[b, on, c]))[-top:]
            if len(np.unique(s)) != len(s):
                return False
    return True
