"""Training metrics (row f8), the parts that need no GPU: metrics.py against the reference's own classes (fixture
tests/golden/ref_train_metrics.npz, written by tools/gen_golden_metrics.py), the exact-integer deviation, the
all-reduce, and the C-ABI's declarations."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pp_head_metrics", "pp_set_train_metrics", "pp_get_train_metrics_enabled", "pp_get_train_metrics")


@pytest.fixture(scope="module")
def gold():
    return load_golden("ref_train_metrics.npz")


def _cases(gold):
    return [str(c) for c in gold["cases"]]


def test_committed_inputs_keep_clear_of_the_thresholds(pp, gold):
    """What makes the GPU comparison on these logits exact: no float64 score within 4 * 2**-24 of a threshold, no
    logit of exactly 0, nothing non-finite."""
    M = pp.metrics
    assert M.THRESHOLD_MARGIN == 4 * 2.0 ** -24
    assert _cases(gold) == ["b2c1", "b3c2", "b1c3"]
    for name in _cases(gold):
        x = gold[f"{name}/logits"]
        assert x.dtype == np.float32 and np.isfinite(x).all() and (x != 0).all()
        s = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
        for t in M.THRESHOLDS:
            assert np.abs(s - float(np.float32(t))).min() > M.THRESHOLD_MARGIN
        assert not M.near_threshold(x.reshape(-1, 1, x.shape[-1])).any()
        lab = gold[f"{name}/labels"]
        assert lab.min() == -1 and lab.max() == x.shape[-1]
        assert (lab[2] <= 0).all() and gold[f"{name}/cls_loss"][4] == 0.0      # the two special steps


def test_counts_and_running_values_match_the_reference(pp, gold):
    M = pp.metrics
    keys = [str(k) for k in gold["ret_keys"]]
    for name in _cases(gold):
        logits, labels = gold[f"{name}/logits"], gold[f"{name}/labels"]
        tm = M.TrainMetrics()
        for s in range(logits.shape[0]):
            counts = M.head_metrics_np(labels[s], logits[s])
            assert counts.dtype == np.int64 and counts.shape == (32,) and not counts[17:].any()
            c = M.unpack_counts(counts)
            tp, tn, fp, fn = gold[f"{name}/binary"][s].T            # the reference's _calc_binary_metrics, per threshold
            assert np.array_equal(c["tp"], tp) and np.array_equal(c["tn"], tn)
            assert np.array_equal(c["fp"], fp) and np.array_equal(c["fn"], fn)
            assert c["n_pos"] == (labels[s] > 0).sum() and c["n_neg"] == (labels[s] == 0).sum()
            ret = tm.update(counts, gold[f"{name}/cls_loss"][s], gold[f"{name}/loc_loss"][s])
            # the accumulators: the reference's float32 variables hold exact integers here
            assert tm.acc.total == gold[f"{name}/acc_total"][s] and tm.acc.count == gold[f"{name}/acc_count"][s]
            for k in ("prec_total", "prec_count", "rec_total", "rec_count"):
                assert np.array_equal(getattr(tm.pr, k), gold[f"{name}/{k}"][s]), (name, s, k)
            assert list(ret.keys()) == keys
            np.testing.assert_allclose([ret[k] for k in keys], gold[f"{name}/ret"][s], rtol=1e-6, atol=0, equal_nan=True)
            assert ret == tm.result()
        assert tm.steps == logits.shape[0]
        assert tm.cls_loss.count == logits.shape[0] - 1 and tm.loc_loss.count == logits.shape[0]     # the 0 loss was skipped


def test_update_metrics_with_the_reference_argument_list(pp, gold):
    M = pp.metrics
    keys = [str(k) for k in gold["ret_keys"]]
    name = "b3c2"
    cfg = {"model": {"second": {"num_class": 2, "encode_background_as_zeros": True, "use_sigmoid_score": True}}}
    acc, pr, sc, sl = M.Accuracy(), M.PrecisionRecall(), M.Scalar(), M.Scalar()
    for s in range(6):
        lab = gold[f"{name}/labels"][s]
        ret = M.update_metrics(cfg, gold[f"{name}/cls_loss"][s], gold[f"{name}/loc_loss"][s],
                               gold[f"{name}/logits"][s].reshape(3, 320, 4), lab, (lab != -1).astype(np.float32), acc, pr, sc, sl)
        np.testing.assert_allclose([ret[k] for k in keys], gold[f"{name}/ret"][s], rtol=1e-6, atol=0, equal_nan=True)
    cfg["model"]["second"]["use_sigmoid_score"] = False
    with pytest.raises(ValueError):
        M.update_metrics(cfg, 1.0, 1.0, np.zeros((1, 4, 2)), np.zeros((1, 4)), np.ones((1, 4)), acc, pr, sc, sl)


def test_hand_placed_logits(pp):
    """0 is a score of exactly 0.5 (not above it), +-80 saturate, a NaN compares false everywhere, a tie takes the
    first class."""
    M = pp.metrics
    nan = np.float32("nan")
    x = np.array([[[0.0, -3.0], [80.0, -80.0], [-80.0, -80.0], [nan, 5.0], [5.0, nan], [2.0, 2.0], [-1.0, 0.5], [nan, nan]]],
                 np.float32)
    lab = np.array([[0, 1, 0, 2, 1, 1, 2, 0]], np.int32)
    c = M.unpack_counts(M.head_metrics_np(lab, x))
    # predicted labels: 0 (no score above 0.5), 1, 0, 1 (the NaN in front stays the maximum; 5.0 passes 0.5),
    # 1 (a later NaN never compares greater), 1 (tie: first), 2, 0 -> the matches are anchors 0, 1, 2, 4, 5, 6, 7
    assert c["acc_hit"] == 7 and c["n_pos"] == 5 and c["n_neg"] == 3
    # scores: 0.5, 1, ~0, NaN, NaN, .88, .62, NaN -- positives over t: anchor 1 always, 5 up to 0.8, 6 up to 0.5
    assert c["tp"].tolist() == [3, 3, 3, 2, 2, 1, 1]
    assert c["fp"].tolist() == [1, 1, 0, 0, 0, 0, 0]          # anchor 0: 0.5 > 0.3 but not > 0.5
    assert (c["tp"] + c["fn"] == 5).all() and (c["fp"] + c["tn"] == 3).all()
    ign = M.unpack_counts(M.head_metrics_np(np.full((1, 8), -1), x))
    assert ign["acc_hit"] == 0 and ign["n_pos"] == 0 and ign["n_neg"] == 0 and not ign["tp"].any() and not ign["fp"].any()


def test_totals_stay_exact_beyond_2_to_the_24(pp):
    """The deliberate difference from the reference: its float32 variables stop counting exactly above 2**24 (at the
    shipped shape, 20480 anchors a frame, batch 2: 410 steps); these are int64."""
    M = pp.metrics
    assert int(np.ceil(2 ** 24 / (2 * 20480))) == 410
    counts = np.zeros(32, np.int64)
    counts[0], counts[1], counts[2] = 600001, 300001, 600000          # acc_hit, n_pos, n_neg: 900001 cared anchors
    counts[3:10] = 250001
    counts[10:17] = 100001
    tm = M.TrainMetrics()
    f32_total = np.float32(0)
    for _ in range(40):
        tm.update(counts, 1.0, 1.0)
        f32_total = np.float32(f32_total + np.float32(600001))
    assert tm.acc.total == 40 * 600001 > 2 ** 24 and tm.acc.count == 40 * 900001
    assert int(f32_total) != tm.acc.total                             # what the reference's variable would hold
    assert (tm.pr.rec_total == 40 * 250001).all() and (tm.pr.rec_count == 40 * 300001).all()
    assert (tm.pr.prec_count == 40 * 350002).all()
    r = tm.result()
    assert r["rpn_acc"] == (40 * 600001) / (40 * 900001)
    assert r["rec@50"] == 250001 / 300001 and r["prec@50"] == 250001 / 350002      # no 1e5 cap on the denominator
    # Accuracy's per-step clip: at least 1, at most 1e6 cared anchors
    a = M.Accuracy()
    a.update(0, 0)
    assert a.count == 1
    a.update(5, 3000000)
    assert a.count == 1000001 and a.total == 5


def test_scalar_and_empty_denominators(pp):
    M = pp.metrics
    s = M.Scalar()
    assert np.isnan(s.value())
    assert np.isnan(s.update(0.0)) and s.count == 0                  # exactly 0 is skipped
    assert s.update(2.0) == 2.0 and s.update(0.0) == 2.0 and s.update(4.0) == 3.0
    tm = M.TrainMetrics()
    r = tm.result()
    assert np.isnan(r["cls_loss"]) and np.isnan(r["rpn_acc"]) and np.isnan(r["cls_loss_rt"])
    assert all(r[k] == 0.0 for pk in M.threshold_keys() for k in pk)  # 0 / clip(0, 1)
    # a step without positives adds nothing to recall; thresholds nobody passes add nothing to precision
    counts = np.zeros(32, np.int64)
    counts[2] = 10
    counts[10:13] = 4
    tm.update(counts, 0.5, 0.0)
    assert not tm.pr.rec_count.any() and tm.pr.prec_count.tolist() == [4, 4, 4, 0, 0, 0, 0]
    assert tm.result()["loc_loss_rt"] == 0.0 and np.isnan(tm.result()["loc_loss"])
    tm.reset()
    assert tm.steps == 0 and tm.acc.count == 0 and not tm.pr.prec_count.any()


_WORKER = r"""
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
import torch.distributed as dist
import pp_amd as pp
dist.init_process_group(backend="gloo")
r, n = dist.get_rank(), dist.get_world_size()
M = pp.metrics
with np.load(os.path.join("tests", "golden", "ref_train_metrics.npz")) as z:
    logits, labels, cl, ll = (z["b3c2/" + k] for k in ("logits", "labels", "cls_loss", "loc_loss"))
mine, whole = M.TrainMetrics(), M.TrainMetrics()
for s in range(6):
    c = M.head_metrics_np(labels[s], logits[s])
    whole.update(c, cl[s], ll[s])
    if s % n == r:
        mine.update(c, cl[s], ll[s])
tot = mine.allreduce(dist)
a, b = tot._pack(), whole._pack()
assert np.array_equal(a[0], b[0]), (a[0], b[0])
assert np.allclose(a[1], b[1], rtol=1e-12, atol=0)
ra, rb = tot.result(), whole.result()
for k in rb:
    if not k.endswith("_rt"):
        assert abs(ra[k] - rb[k]) <= 1e-12 * abs(rb[k]), (k, ra[k], rb[k])
assert ra["cls_loss_rt"] == mine.cls_loss_rt and mine.steps == 3 and tot.steps == 6
print("rank", r, "ok")
dist.destroy_process_group()
"""


def test_allreduce_two_ranks_gloo_equals_one_process(pp, tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29547", str(script)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert r.stdout.count("ok") == 2
    # no communicator: a copy
    tm = pp.metrics.TrainMetrics()
    tm.update(np.arange(32), 1.0, 2.0)
    cp = tm.allreduce(None)
    assert cp is not tm and cp.result() == tm.result()


def test_gpu_problem_keeps_clear_of_the_thresholds(pp):
    """The detect problem of tests/test_gpu_train_metrics.py on the CPU oracle's forward pass: the restatement alone
    stays under that test's cap of 0.1 % of the anchors within 4 * 2**-24 of a threshold."""
    import util_ref
    import test_gpu_train_metrics as g
    cfg, d, w, frames, labels = g._detect_problem(pp)
    rect, trv, p2 = pp.synth.default_calib()
    ref = util_ref.oracle_detect(d, w, frames, rect, trv, p2)
    cls = np.asarray(ref["preds"]["cls_preds"], np.float32).reshape(2, d.num_anchors, 1)
    near = pp.metrics.near_threshold(cls)
    assert near.sum() <= 1e-3 * near.size
    s = 1 / (1 + np.exp(-cls.astype(np.float64)))
    assert 0.02 < (s > 0.5).mean() < 0.98                      # the classifier fires on some anchors and not on others
    assert (labels > 0).sum() > 100 and (labels == 0).sum() > 100 and (labels == -1).sum() > 100


def test_header_declares_the_metrics_surface():
    with open(os.path.join(ROOT, "include", "pp_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+PP_METRICS_COUNTS\s+32\b", h)
    assert re.search(r"int\s+pp_head_metrics\s*\(\s*pp_handle\s+h\s*,\s*const\s+int32_t\s*\*\s*labels\s*,\s*int32_t\s+batch\s*,"
                     r"\s*const\s+float\s*\*\s*cls_preds\s*,\s*int64_t\s*\*\s*counts\s*\)", h)
    assert re.search(r"int\s+pp_set_train_metrics\s*\(\s*pp_handle\s+h\s*,\s*int32_t\s+on\s*\)", h)
    assert re.search(r"int\s+pp_get_train_metrics_enabled\s*\(\s*pp_handle\s+h\s*,\s*int32_t\s*\*\s*on\s*\)", h)
    assert re.search(r"int\s+pp_get_train_metrics\s*\(\s*pp_handle\s+h\s*,\s*int64_t\s*\*\s*counts\s*\)", h)
    added = h[h.index("later additions within"):h.index("#define PP_ABI_VERSION")]
    for name in NEW:
        assert name in added
    assert added.index("pp_get_detection_rows") < added.index("pp_head_metrics")      # appended, nothing before them changed


def test_binding_and_argument_errors(pp, hip_lib):
    for name in NEW:
        assert name in pp._lib.EXPORTS and hasattr(hip_lib, name)
    assert pp._lib.EXPORTS.index("pp_get_detection_rows") < pp._lib.EXPORTS.index("pp_head_metrics")
    assert "metrics.hip" in pp._lib.SOURCES and "api_metrics.hip" in pp._lib.SOURCES
    assert pp._lib.PP_METRICS_COUNTS == pp.metrics.NCOUNTS == 32
    for name in ("head_metrics", "set_train_metrics", "train_metrics", "train_metrics_counts"):
        assert hasattr(pp.Engine, name)
    for name in ("metrics", "reset_metrics"):
        assert hasattr(pp.Trainer, name)
    # a NULL handle is an argument error on every entry point (nothing is dereferenced)
    import ctypes
    counts = np.zeros(32, np.int64)
    lab = np.zeros(4, np.int32)
    on = ctypes.c_int32(7)
    PP_ERR_ARG = 1
    assert hip_lib.pp_head_metrics(None, lab.ctypes.data, 1, None, counts.ctypes.data) == PP_ERR_ARG
    assert hip_lib.pp_set_train_metrics(None, 1) == PP_ERR_ARG
    assert hip_lib.pp_get_train_metrics_enabled(None, ctypes.byref(on)) == PP_ERR_ARG and on.value == 7
    assert hip_lib.pp_get_train_metrics(None, counts.ctypes.data) == PP_ERR_ARG
    assert not counts.any()
    with pytest.raises(ValueError, match="training option"):
        pp.VoxelNet(pp.config.tiny_config(1), training=False, metrics=True)
