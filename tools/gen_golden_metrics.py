"""Writes tests/golden/ref_train_metrics.npz: seeded steps of class logits / labels / losses and what the REFERENCE's
monitoring block makes of them (data only).

TEST INFRASTRUCTURE, run where the reference tree is available (tools/ref_shim.py).  The reference's `Accuracy`,
`PrecisionRecall`, `Scalar`, `_calc_binary_metrics` and `update_metrics` (libraries/metrics.py) run unmodified; what
they import as `tensorflow` is the small stand-in below, on float32 numpy, which covers exactly the calls that file
makes: sigmoid, argmax, where, keras.backend.any, reduce_sum, reduce_max, cast, clip_by_value, reshape, equal, constant,
zeros, Variable.assign_add / scatter_nd_add, and keras.Model as a plain base class.  float32 where TensorFlow is float32:
the variables, the sigmoid, the sums (all sums here are of 0 / 1 values far below 2**24, so their order does not
matter) and the final divisions.

Per case (batch, anchors, num_class) the file holds 6 steps: logits, labels, the two losses; per step the reference's
tp / tn / fp / fn at the seven thresholds, its variables after the step and the dict update_metrics returned.  Step 2
has no positive label, step 4 a classification loss of exactly 0.  No float64 score of any logit lies within
4 * 2**-24 of a threshold (metrics.near_threshold), so float32 implementations whose exp differs in the last place
still count the same.

    python tools/gen_golden_metrics.py
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ref_shim  # noqa: E402

CASES = (("b2c1", 2, 640, 1, 11), ("b3c2", 3, 640, 2, 12), ("b1c3", 1, 640, 3, 13))     # name, batch, anchors, classes, seed
STEPS = 6


# ---- the tensorflow stand-in ----
class _T(np.ndarray):
    """A tensor: a numpy array with .numpy()."""

    def numpy(self):
        return np.asarray(self)


def _t(x, dtype=None):
    return np.asarray(x, dtype=dtype).view(_T)


class _Variable:
    def __init__(self, initial_value=0.0, trainable=False, dtype=np.float32, name=None):
        self.v = np.array(initial_value, dtype=dtype)

    def assign_add(self, x):
        self.v = np.array(self.v + np.asarray(x, self.v.dtype), dtype=self.v.dtype)

    def scatter_nd_add(self, indices, updates):
        for idx, u in zip(indices, updates):
            self.v[tuple(idx)] = self.v.dtype.type(self.v[tuple(idx)] + self.v.dtype.type(u))

    def __array__(self, dtype=None, copy=None):
        return np.array(self.v, dtype=dtype)

    def __truediv__(self, other):
        return _t(self.v / np.asarray(other), self.v.dtype)

    def numpy(self):
        return self.v.copy()


class _Model:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return self.call(*a, **k)


def _sigmoid(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        return _t(np.float32(1.0) / (np.float32(1.0) + np.exp(-x)), np.float32)


def _clip(x, clip_value_min, clip_value_max):
    x = np.asarray(x)
    return _t(np.clip(x, x.dtype.type(clip_value_min), x.dtype.type(clip_value_max)), x.dtype)


def _make_tf():
    tf = ref_shim._Anything("tensorflow")      # (whatever else the file imports stays a permissive stub)
    tf.__path__ = []
    tf.float32, tf.int64 = np.float32, np.int64
    tf.Variable = _Variable
    tf.zeros = lambda n, dtype=np.float32: np.zeros(n, dtype)
    tf.constant = lambda v, dtype=None: _t(v, dtype)
    tf.cast = lambda x, dtype: _t(np.asarray(x).astype(dtype))
    tf.reshape = lambda x, shape: _t(np.asarray(x).reshape(shape))
    tf.equal = lambda a, b: _t(np.asarray(a) == np.asarray(b))
    tf.argmax = lambda x, axis=None: _t(np.argmax(np.asarray(x), axis=axis), np.int64)
    tf.where = lambda condition, x, y: _t(np.where(np.asarray(condition), np.asarray(x), np.asarray(y)))
    tf.reduce_sum = lambda x: _t(np.sum(np.asarray(x), dtype=np.asarray(x).dtype))
    tf.clip_by_value = _clip
    tf.math = types.SimpleNamespace(sigmoid=_sigmoid, reduce_max=lambda x, axis=None: _t(np.max(np.asarray(x), axis=axis)))
    keras = ref_shim._Anything("tensorflow.keras")
    keras.__path__ = []
    keras.Model = _Model
    keras.backend = types.SimpleNamespace(any=lambda x, axis=None: _t(np.any(np.asarray(x), axis=axis)))
    tf.keras = keras
    sys.modules["tensorflow"] = tf
    sys.modules["tensorflow.keras"] = keras
    return tf


def load_reference_metrics():
    _make_tf()
    ref_shim.install()
    return importlib.import_module("libraries.metrics")


# ---- seeded inputs ----
def make_case(batch, anchors, ncls, seed):
    from pp_amd import metrics as M
    rs = np.random.RandomState(seed)
    logits = (rs.standard_normal((STEPS, batch, anchors, ncls)) * 2.5).astype(np.float32)
    for _ in range(100):        # redraw what sits on a threshold (none expected: the margin is 2.4e-7 wide)
        near = M.near_threshold(logits.reshape(-1, 1, ncls)).reshape(STEPS, batch, anchors)
        bad = near | (logits == 0).any(-1)
        if not bad.any():
            break
        logits[bad] = (rs.standard_normal((int(bad.sum()), ncls)) * 2.5).astype(np.float32)
    else:
        raise RuntimeError("could not clear the threshold margins")
    labels = rs.choice(np.arange(-1, ncls + 1), size=(STEPS, batch, anchors),
                       p=[0.15, 0.65] + [0.2 / ncls] * ncls).astype(np.int32)
    labels[2][labels[2] > 0] = 0                 # a step without positives
    cls_loss = rs.uniform(0.1, 2.0, STEPS).astype(np.float32)
    loc_loss = rs.uniform(0.1, 2.0, STEPS).astype(np.float32)
    cls_loss[4] = 0.0                            # a loss of exactly 0: Scalar skips it
    return logits, labels, cls_loss, loc_loss


def run_reference(ref, logits, labels, cls_loss, loc_loss, ncls):
    config = {"model": {"second": {"num_class": ncls, "encode_background_as_zeros": True, "use_sigmoid_score": True}}}
    acc, pr, s_cls, s_loc = ref.Accuracy(config), ref.PrecisionRecall(config), ref.Scalar(), ref.Scalar()
    keys = ["cls_loss", "cls_loss_rt", "loc_loss", "loc_loss_rt", "rpn_acc"]
    for t in pr._thresholds:
        keys += [f"prec@{int(t * 100)}", f"rec@{int(t * 100)}"]
    out = {k: [] for k in ("binary", "acc_total", "acc_count", "prec_total", "prec_count", "rec_total", "rec_count", "ret")}
    for s in range(STEPS):
        lab = _t(labels[s])
        preds = _t(logits[s])
        sampled = _t((labels[s] != -1).astype(np.float32))
        # the step's own tp / tn / fp / fn, from the reference's _calc_binary_metrics as PrecisionRecall.call calls it
        scores = np.max(_sigmoid(preds), axis=-1)
        out["binary"].append([[float(v) for v in ref._calc_binary_metrics(lab, _t(scores), sampled, -1, th)]
                              for th in pr._thresholds])
        ret = ref.update_metrics(config, _t(cls_loss[s]), _t(loc_loss[s]), preds, lab, sampled, acc, pr, s_cls, s_loc)
        assert list(ret.keys()) == keys, list(ret.keys())
        out["ret"].append([ret[k] for k in keys])
        out["acc_total"].append(float(acc.total.numpy()))
        out["acc_count"].append(float(acc.count.numpy()))
        for k in ("prec_total", "prec_count", "rec_total", "rec_count"):
            out[k].append(getattr(pr, k).numpy().astype(np.float64))
    res = {k: np.asarray(v, np.float64) for k, v in out.items()}
    for k in ("binary", "acc_total", "acc_count", "prec_total", "prec_count", "rec_total", "rec_count"):
        assert np.all(res[k] == np.round(res[k])) and res[k].max() < 2 ** 24      # exact integers in float32
        res[k] = res[k].astype(np.int64)
    return res, keys


def main():
    ref = load_reference_metrics()
    blob = {}
    keys = None
    for name, batch, anchors, ncls, seed in CASES:
        logits, labels, cls_loss, loc_loss = make_case(batch, anchors, ncls, seed)
        res, keys = run_reference(ref, logits, labels, cls_loss, loc_loss, ncls)
        blob[f"{name}/logits"], blob[f"{name}/labels"] = logits, labels
        blob[f"{name}/cls_loss"], blob[f"{name}/loc_loss"] = cls_loss, loc_loss
        for k, v in res.items():
            blob[f"{name}/{k}"] = v
    blob["cases"] = np.array([c[0] for c in CASES])
    blob["ret_keys"] = np.array(keys)
    path = os.path.join(ROOT, "tests", "golden", "ref_train_metrics.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
