"""The training step on the backbone layouts of tests/stride_layouts.py -- first block at stride 2 (block1.0 reads the
scatter canvas and takes the two-pass depthwise backward), transposed convolutions with kernel == stride 1, 2, 4 and 8
(map_row's shift branches and its generic division branch), k = 1 behind a stride-1 block, a block without in-block layers
(its stride layer feeds the deconv), three frames (every map's rows end inside a 64- and a 128-row tile) -- against torch
autograd over the restated network, the float64 oracle's batch statistics and the oracle's head maps on the trained
weights.  Every bar is the one of the test named next to it; the weight seeds are fixed in the table
(tests/test_stride_layouts_host.py holds them to the kink margin on the CPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import stride_layouts as SL
import util_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = SL.B
HEAD_KEYS = ("box_preds", "cls_preds", "dir_cls_preds")
LOSS_KEYS = ("loss", "loc_loss_reduced", "cls_loss_reduced", "dir_loss_reduced", "cls_pos_loss", "cls_neg_loss")


def _trainer(pp, p, w=None, **kw):
    return pp.Trainer(p.cfg, p.w if w is None else w, max_batch=B, max_points_per_frame=4096, **kw)


# ------------------------------------------------------------------ 1. the step against autograd
@pytest.mark.parametrize("name", SL.NAMES)
def test_step_matches_autograd(pp, hip_lib, name):
    """The bars of test_gradients_match_autograd_small_grids: loss keys within 1e-5 * max(1, |v|), num_positives equal,
    every trainable tensor's gradient within 1e-4 of the tensor's largest against the float32 graph and against the
    float64 graph under the step's own decisions, a second pass bit-identical."""
    from test_gpu_train import _rel_errors
    p = SL.layout_problem(pp, name)
    d = p.d
    vals, grads = p.ref32[0], p.ref32[1]
    print(f"{name}: weight seed {p.weight_seed}, kink margin {p.margin:.2e} (tests/test_stride_layouts_host.py asserts it)")
    tr = _trainer(pp, p)
    out = tr.forward_backward(p.frames, p.labels, p.reg)
    g1 = tr.grads.cpu().numpy().copy()
    for k in LOSS_KEYS:
        assert abs(out[k] - vals[k]) <= 1e-5 * max(1.0, abs(vals[k])), (k, out[k], vals[k])
    assert out["num_positives"] == vals["num_positives"] == p.num_positives
    got = tr.gradients()
    assert set(got) == set(grads)
    (wn, wmax), _ = _rel_errors(got, grads)
    print(f"{name}: {tr.params.numel()} trainable parameters, worst relative gradient error {wmax:.2e} ({wn})")
    assert wmax <= SL.GRAD_BAR, (wn, wmax)
    (fn_, fmax), _ = _rel_errors(got, p.grads64(util_ref.forced_decisions(tr, p.ex)))
    print(f"{name}: against float64 with the step's decisions {fmax:.2e} ({fn_})")
    assert fmax <= SL.GRAD_BAR, (fn_, fmax)
    # the decision masks of the transposed convolutions: [B, input pixels, k, k, C]
    dec = tr.decisions()
    maps = SL.MAPS[name][0]
    for b in range(3):
        k, (h, w) = d.upsample_strides[b], maps[b]
        assert dec[f"rpn/deconv{b + 1}/bn"].shape == (B, h * w, k, k, d.num_upsample_filters[b]), (b, k)
    out2 = tr.forward_backward(p.frames, p.labels, p.reg)
    assert out2["loss"] == out["loss"] and np.array_equal(tr.grads.cpu().numpy(), g1), "bit-identical second pass"
    tr.close()


# ------------------------------------------------------------------ 2. moving statistics
@pytest.mark.parametrize("name", SL.NAMES)
def test_moving_statistics_after_one_step(pp, hip_lib, name):
    """One step from moving statistics 0 / 0 against the float64 oracle's batch statistics, every BatchNorm layer, with
    the bars and the row counts of test_gpu_train_regime.batch_statistics_errors: mean within 1e-6 |m64| + 1e-5 sqrt(v64),
    biased variance within 1e-4 v64 + 1e-9 (each + 3x the float32 restatement's own error).  The transposed convolutions'
    rows are B * h * w * k * k and the moving variance carries their Bessel factor: a count without k * k, or k for k * k,
    is off by 1 / n and more."""
    from test_gpu_train_regime import _check_statistics, _rows, _zero_moving
    p = SL.layout_problem(pp, name)
    d = p.d
    rows = _rows(d, B)
    want_rows, _ = SL.layer_rows(d)
    assert rows == want_rows
    s64, s32 = p.stats64, p.ref32[2]
    w = _zero_moving(d, {k: np.array(v, copy=True) for k, v in p.w.items()})
    tr = _trainer(pp, p, w=w)
    tr.forward_backward(p.frames, p.labels, p.reg)
    after = tr.weights()
    tr.close()
    errs = {}
    for bn, (m64, v64) in s64.items():
        mom = 0.01 if bn == "pfn/bn" else 0.99
        keep = np.float64(np.float32(1.0) - np.float32(mom))
        m = after[bn + "/moving_mean"].astype(np.float64) / keep
        v = after[bn + "/moving_variance"].astype(np.float64) / keep
        if bn != "pfn/bn":
            n = rows[bn]
            v = v * (n - 1.0) / n
        mbar = 1e-6 * np.abs(m64) + 1e-5 * np.sqrt(v64)
        e32 = float((np.abs(s32[bn][0].astype(np.float64) - m64) / mbar).max())
        em = float((np.abs(m - m64) / mbar).max()) / (1.0 + 3.0 * e32)
        vbar = 1e-4 * v64 + 1e-9
        e32v = float((np.abs(s32[bn][1].astype(np.float64) - v64) / vbar).max())
        ev = float((np.abs(v - v64) / vbar).max()) / (1.0 + 3.0 * e32v)
        errs[bn] = (em, ev)
    assert set(errs) == set(rows) | {"pfn/bn"}
    _check_statistics(errs, name)


# ------------------------------------------------------------------ 3. which kernels ran
@pytest.mark.parametrize("name", SL.NAMES)
def test_depthwise_backward_paths(pp, hip_lib, name):
    """A block's first layer reads a tensor (the canvas, the block before's activation): two passes, k_tr_dw_bwd_w and
    k_tr_dw_bwd_in, at stride 1 and at stride 2.  An in-block layer reads the layer before's pre-BatchNorm map at stride 1:
    the one-pass k_tr_dw_bwd."""
    p = SL.layout_problem(pp, name)
    d = p.d
    tr = _trainer(pp, p)
    tr.engine.set_profiling(True)
    tr.forward_backward(p.frames, p.labels, p.reg)
    names = [n.split(":")[0] for n, _ in tr.engine.kernel_times()]
    tr.close()
    print(name, "layer_strides", d.layer_strides, {k: names.count(k) for k in ("k_tr_dw_bwd_in", "k_tr_dw_bwd_w", "k_tr_dw_bwd")})
    if d.layer_strides[0] == 2:
        assert "k_tr_dw_bwd_in" in names and "k_tr_dw_bwd_w" in names
    else:
        assert "k_tr_dw_bwd" in names
    # and exactly: one two-pass backward per block, one one-pass backward per in-block layer
    assert names.count("k_tr_dw_bwd_w") == 3 and names.count("k_tr_dw_bwd_in") == 3
    assert names.count("k_tr_dw_bwd") == sum(d.layer_nums)
    assert names.count("k_tr_bn_relu") >= 6      # the three block-final activations and the three deconvs' pixel shuffles


# ------------------------------------------------------------------ 4. inference on the trained weights
@pytest.mark.parametrize("name", SL.NAMES)
def test_inference_on_trained_weights(pp, hip_lib, name):
    """Two optimizer steps, then Trainer.detect (the weight publish) and a fresh Engine loaded from Trainer.weights(): both
    give the head maps of the oracle on those weights within test_gpu_parity's TOL (the pattern of
    test_trained_weights_round_trip) -- the inference deconv kernels at B = 3 and, for s222-u248, at k = 8."""
    from test_gpu_parity import TOL
    p = SL.layout_problem(pp, name)
    d = p.d
    tr = _trainer(pp, p, learning_rate=2e-3, weight_decay=1e-4)
    for _ in range(2):
        tr.step(p.frames, p.labels, p.reg)
    w2 = tr.weights()
    pp.weights.check_weights(d, w2)
    assert np.abs(w2["rpn/conv_cls/kernel"] - p.w["rpn/conv_cls/kernel"]).max() > 1e-4, "the steps moved the heads"
    rect, trv, p2 = p.calib
    ref2 = util_ref.oracle_detect(d, w2, p.frames, rect, trv, p2)
    rects, trvs = np.stack([rect] * B), np.stack([trv] * B)

    def check(eng, what):
        im = eng.intermediates()
        for b in range(B):
            fr = ref2["frames"][b]
            P = fr["coordinates"].shape[0]
            assert im["n_pillars"][b] == P and np.array_equal(im["coors"][b, :P], fr["coordinates"])
            assert np.array_equal(im["anchors_mask"][b].astype(bool), fr["anchors_mask"])
        for k in HEAD_KEYS:
            assert im[k].shape == ref2["preds"][k].shape, k
            print(f"{name} {what} {k}: max |diff| {np.abs(im[k] - ref2['preds'][k]).max():.2e}")
            np.testing.assert_allclose(im[k], ref2["preds"][k], rtol=0, atol=TOL, err_msg=f"{what} {k}")

    tr.detect(p.frames, rects, trvs)
    check(tr.engine, "published")
    tr.close()
    eng = pp.Engine(p.cfg, max_batch=B, max_points_per_frame=4096)
    eng.load_weights(w2)
    eng.detect(p.frames, rects, trvs)
    tags = eng.layer_tags()
    print(name, tags)
    deconvs = [t for t in tags if ":deconv" in t]
    assert len(deconvs) == 3
    check(eng, "fresh engine")
    eng.close()


# ------------------------------------------------------------------ 5. the other kernel generations
@pytest.mark.parametrize("env", [{"PP_TRAIN_FUSED_MIN": "0"}, {"PP_TRAIN_ARENA_FLOATS": "4096"}], ids=["fused", "arena"])
def test_step_matches_autograd_other_generations(hip_lib, env):
    """The fused training-forward launches at every size (k_sep_u<..., TR = 1> at stride 2 on the canvas; TR = 2 for the
    transposed convolutions) and the training arena exhausted: test 1 for every layout in a child process each (the
    switches are read once per process)."""
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_train_layouts.py"), "-k", "test_step_matches_autograd and not other"],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{len(SL.NAMES)} passed" in r.stdout, r.stdout[-1000:]
