"""Training metrics: accuracy, precision / recall at seven score thresholds and the running loss means
(SURVEY section 8f, row f8).

The reference's monitoring block, libraries/metrics.py -- `Accuracy` :46-83, `PrecisionRecall` :86-161, `Scalar`
:33-43, `update_metrics` :164-198, with `train_config.net_metrics_steps: 500` beside it in the shipped YAML -- which
the reference ships but does not wire in (train.py:48).  For encode_background_as_zeros = true and use_sigmoid_score =
true, the only combination the configuration accepts.

Two halves.  The counting over the anchors of a step (`head_metrics_np` here, csrc/metrics.hip on the GPU:
`Engine.head_metrics`, `Engine.train_metrics_counts`) produces 17 integers; everything else is arithmetic on those
integers and needs neither a GPU nor the logits:

    tm = TrainMetrics()
    tm.update(engine.train_metrics_counts(), losses["cls_loss_reduced"], losses["loc_loss_reduced"])
    tm.result()      # {"cls_loss", "cls_loss_rt", "loc_loss", "loc_loss_rt", "rpn_acc", "prec@10", "rec@10", ...}

Rules kept from the reference: Accuracy's denominator grows by clip(cared anchors, 1, 1e6) per step and its numerator
counts predicted label == label over ALL anchors; a step whose tp + fp (tp + fn) is 0 adds nothing to the precision
(recall) accumulators of that threshold, and the final division clips the denominator to at least 1; Scalar skips a loss
that is exactly 0 and is NaN before its first sample.

One deliberate difference: the totals here are exact int64 and the ratios are taken in float64.  The reference keeps
them in float32 variables, which stop counting exactly above 2**24 anchors -- at the shipped shape and batch 2 that is
410 steps -- and it clips the final precision / recall denominators to at most 1e5, which a few steps exceed.  Neither
is reproduced: up to 2**24 anchors the values agree with the reference's to float32 rounding, beyond that these stay
exact.
"""
import numpy as np

THRESHOLDS = (0.1, 0.3, 0.5, 0.7, 0.8, 0.9, 0.95)      # PrecisionRecall._thresholds; compared as float32
NCOUNTS = 32        # PP_METRICS_COUNTS: [0] acc_hit, [1] n_pos, [2] n_neg, [3..9] tp, [10..16] fp, then zeros
_NT = len(THRESHOLDS)
THRESHOLD_MARGIN = 4.0 * 2.0 ** -24     # a float64 score this close to a threshold may fall either side in float32


def threshold_keys():
    """("prec@10", "rec@10"), ... in the reference's order."""
    return [(f"prec@{int(t * 100)}", f"rec@{int(t * 100)}") for t in THRESHOLDS]


def unpack_counts(counts):
    """counts[32] -> {"acc_hit", "n_pos", "n_neg", "tp", "fp", "fn", "tn"} (the last four int64[7])."""
    c = np.asarray(counts, np.int64).reshape(NCOUNTS)
    tp, fp = c[3:3 + _NT].copy(), c[3 + _NT:3 + 2 * _NT].copy()
    return {"acc_hit": int(c[0]), "n_pos": int(c[1]), "n_neg": int(c[2]), "tp": tp, "fp": fp,
            "fn": c[1] - tp, "tn": c[2] - fp}


def _scores_f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(1.0) / (np.float32(1.0) + np.exp(-x))


def head_metrics_np(labels, cls_preds, cared=None):
    """Host restatement of csrc/metrics.hip: the counts of one step.  labels [B, A] (>0 class, 0 background, -1
    ignored), cls_preds [B, A, num_class] logits; cared: the `sampled` weight update_metrics is handed, 0 or 1
    (None: labels != -1).  float32 throughout, a NaN compares false everywhere (a NaN score stays a NaN).  Returns
    int64[32]."""
    labels = np.asarray(labels)
    B = labels.shape[0]
    labels = labels.reshape(B, -1).astype(np.int64)
    x = np.asarray(cls_preds, np.float32).reshape(B, labels.shape[1], -1)
    ncls = x.shape[2]
    cared = (labels != -1) if cared is None else (np.asarray(cared).reshape(labels.shape) != 0)
    s = _scores_f32(x)
    # first maximum of the logits by strict comparison; the largest score, a NaN taking over
    best, arg, score = x[..., 0].copy(), np.zeros(labels.shape, np.int64), s[..., 0].copy()
    for c in range(1, ncls):
        with np.errstate(invalid="ignore"):
            up = x[..., c] > best
            take = (s[..., c] > score) | np.isnan(s[..., c])
        best = np.where(up, x[..., c], best)
        arg = np.where(up, c, arg)
        score = np.where(take, s[..., c], score)
    with np.errstate(invalid="ignore"):
        anyc = (s > np.float32(0.5)).any(axis=-1)
    pred = np.where(anyc, arg + 1, 0)
    pos, neg = cared & (labels > 0), cared & (labels == 0)
    out = np.zeros(NCOUNTS, np.int64)
    out[0], out[1], out[2] = (pred == labels).sum(), pos.sum(), neg.sum()
    for i, t in enumerate(THRESHOLDS):
        with np.errstate(invalid="ignore"):
            over = score > np.float32(t)
        out[3 + i] = (pos & over).sum()
        out[3 + _NT + i] = (neg & over).sum()
    return out


def near_threshold(cls_preds, margin=THRESHOLD_MARGIN):
    """Boolean [B, A]: anchors with a class score (float64) within `margin` of a threshold -- float32 implementations
    whose exp differs in the last place may put those on either side.  A logit of exactly 0 (score exactly 0.5 in any
    precision) and NaN logits are not counted."""
    x = np.asarray(cls_preds, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
        near = np.zeros(x.shape, bool)
        for t in THRESHOLDS:
            near |= np.abs(s - float(np.float32(t))) <= margin
    near &= x != 0.0
    return near.any(axis=-1)


class Scalar:
    """Running mean of a loss (metrics.py:33-43): a value of exactly 0 is skipped; NaN before the first sample."""

    def __init__(self):
        self.total, self.count = 0.0, 0.0

    def update(self, value):
        value = float(value)
        if value != 0.0:
            self.count += 1.0
            self.total += value
        return self.value()

    __call__ = update

    def value(self):
        return self.total / self.count if self.count else float("nan")


class Accuracy:
    """metrics.py:46-83 on a step's counts: total += acc_hit; count += clip(cared anchors, 1, 1e6)."""

    def __init__(self):
        self.total, self.count = 0, 0

    def update(self, acc_hit, n_cared):
        self.total += int(acc_hit)
        self.count += int(min(max(int(n_cared), 1), 1000000))
        return self.value()

    def value(self):
        return self.total / self.count if self.count else float("nan")


class PrecisionRecall:
    """metrics.py:86-140 on a step's counts: a threshold whose tp + fp (tp + fn) is 0 in a step adds nothing."""

    def __init__(self):
        self.prec_total = np.zeros(_NT, np.int64)
        self.prec_count = np.zeros(_NT, np.int64)
        self.rec_total = np.zeros(_NT, np.int64)
        self.rec_count = np.zeros(_NT, np.int64)

    def update(self, tp, fp, fn):
        tp, fp, fn = (np.asarray(a, np.int64).reshape(_NT) for a in (tp, fp, fn))
        rec, prec = (tp + fn) > 0, (tp + fp) > 0
        self.rec_count += np.where(rec, tp + fn, 0)
        self.rec_total += np.where(rec, tp, 0)
        self.prec_count += np.where(prec, tp + fp, 0)
        self.prec_total += np.where(prec, tp, 0)
        return self.value()

    def value(self):
        """(precision[7], recall[7]) float64; a denominator of 0 is taken as 1."""
        return (self.prec_total / np.maximum(self.prec_count, 1).astype(np.float64),
                self.rec_total / np.maximum(self.rec_count, 1).astype(np.float64))


class TrainMetrics:
    """The four accumulators update_metrics feeds (rpn_acc, rpn_metrics, rpn_cls_loss, rpn_loc_loss) and the last
    step's two losses, fed from a step's counts."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.acc, self.pr = Accuracy(), PrecisionRecall()
        self.cls_loss, self.loc_loss = Scalar(), Scalar()
        self.cls_loss_rt = self.loc_loss_rt = float("nan")
        self.steps = 0

    def update(self, counts, cls_loss_reduced, loc_loss_reduced, n_cared=None):
        """counts: int64[32] of one step (pp_get_train_metrics / head_metrics_np).  n_cared: anchors with a non-zero
        `sampled` weight; None = n_pos + n_neg, which is the same for labels in {-1, 0, 1..num_class}."""
        c = unpack_counts(counts)
        self.acc.update(c["acc_hit"], c["n_pos"] + c["n_neg"] if n_cared is None else n_cared)
        self.pr.update(c["tp"], c["fp"], c["fn"])
        self.cls_loss.update(cls_loss_reduced)
        self.loc_loss.update(loc_loss_reduced)
        self.cls_loss_rt, self.loc_loss_rt = float(cls_loss_reduced), float(loc_loss_reduced)
        self.steps += 1
        return self.result()

    def result(self):
        """update_metrics' dict: cls_loss, cls_loss_rt, loc_loss, loc_loss_rt, rpn_acc, prec@10, rec@10, ... rec@95."""
        prec, rec = self.pr.value()
        ret = {"cls_loss": self.cls_loss.value(), "cls_loss_rt": self.cls_loss_rt, "loc_loss": self.loc_loss.value(),
               "loc_loss_rt": self.loc_loss_rt, "rpn_acc": self.acc.value()}
        for i, (pk, rk) in enumerate(threshold_keys()):
            ret[pk] = float(prec[i])
            ret[rk] = float(rec[i])
        return ret

    # ---- the accumulators as two flat arrays (all-reduce, checkpoints) ----
    def _pack(self):
        ints = np.concatenate([[self.acc.total, self.acc.count, self.steps], self.pr.prec_total, self.pr.prec_count,
                               self.pr.rec_total, self.pr.rec_count]).astype(np.int64)
        floats = np.array([self.cls_loss.total, self.cls_loss.count, self.loc_loss.total, self.loc_loss.count], np.float64)
        return ints, floats

    def _unpack(self, ints, floats):
        self.acc.total, self.acc.count, self.steps = int(ints[0]), int(ints[1]), int(ints[2])
        p = self.pr
        p.prec_total, p.prec_count, p.rec_total, p.rec_count = (np.array(ints[3 + k * _NT:3 + (k + 1) * _NT], np.int64)
                                                               for k in range(4))
        self.cls_loss.total, self.cls_loss.count, self.loc_loss.total, self.loc_loss.count = (float(v) for v in floats)

    def allreduce(self, dist=None, device=None):
        """The totals over all ranks, as a new TrainMetrics (this one keeps counting its own rank): one SUM of the int64
        accumulators and one of the four loss accumulators.  `dist` is torch.distributed (None / uninitialised / one
        rank: a copy); `device`: where the two small tensors live (a backend that only moves device memory needs the
        rank's GPU).  cls_loss_rt / loc_loss_rt stay this rank's last step."""
        out = TrainMetrics()
        ints, floats = self._pack()
        if dist is not None and dist.is_initialized() and dist.get_world_size() > 1:
            import torch
            ti = torch.from_numpy(ints).to(device) if device is not None else torch.from_numpy(ints)
            tf = torch.from_numpy(floats).to(device) if device is not None else torch.from_numpy(floats)
            dist.all_reduce(ti, op=dist.ReduceOp.SUM)
            dist.all_reduce(tf, op=dist.ReduceOp.SUM)
            ints, floats = ti.cpu().numpy(), tf.cpu().numpy()
        out._unpack(ints, floats)
        out.cls_loss_rt, out.loc_loss_rt = self.cls_loss_rt, self.loc_loss_rt
        return out


def update_metrics(config, cls_loss, loc_loss, cls_preds, labels, sampled, rpn_acc, rpn_metrics, rpn_cls_loss,
                   rpn_loc_loss):
    """metrics.py:164-198 with the reference's argument list, on numpy: counts the step on the host (head_metrics_np)
    and feeds the four accumulators (an Accuracy, a PrecisionRecall, two Scalars of this module)."""
    second = config["model"]["second"]
    if not second.get("encode_background_as_zeros", True) or not second.get("use_sigmoid_score", True):
        raise ValueError("metrics: encode_background_as_zeros and use_sigmoid_score must both be true")
    num_class = int(second["num_class"])
    cls_preds = np.asarray(cls_preds, np.float32)
    batch = cls_preds.shape[0]
    cls_preds = cls_preds.reshape(batch, -1, num_class)
    cared = np.asarray(sampled).reshape(batch, -1) != 0
    c = unpack_counts(head_metrics_np(labels, cls_preds, cared))
    acc = rpn_acc.update(c["acc_hit"], int(cared.sum()))
    prec, rec = rpn_metrics.update(c["tp"], c["fp"], c["fn"])
    ret = {"cls_loss": rpn_cls_loss.update(cls_loss), "cls_loss_rt": float(cls_loss),
           "loc_loss": rpn_loc_loss.update(loc_loss), "loc_loss_rt": float(loc_loss), "rpn_acc": float(acc)}
    for i, (pk, rk) in enumerate(threshold_keys()):
        ret[pk] = float(prec[i])
        ret[rk] = float(rec[i])
    return ret
