"""Buffer reuse the shipped configurations do not reach (all `-m gpu`, through the C-ABI): the frame sub-range walk of
run_backbone over a block that writes more bytes per frame than it reads (stride 1 with more channels, or stride 2 with
cout > 4 cin), whose ping-pong activation buffers would otherwise be overwritten before they are read.
"""
import numpy as np
import pytest

import util_ref

pytestmark = pytest.mark.gpu

TOL = 1e-4


# ------------------------------------------------------------------ frame sub-ranges over a widening block
def _widening_config(pp, B, strides, filters, upsample):
    cfg = pp.config.kitti_shaped_config(B)
    cfg["model"]["second"]["rpn"].update(layer_strides=strides, num_filters=filters, upsample_strides=upsample)
    return cfg


def _launches(eng, frames, layer):
    eng.set_profiling(True)
    d, n = eng.detect(frames)
    k = sum(1 for name, _ in eng.kernel_times() if name.endswith(":" + layer))
    eng.set_profiling(False)
    return k, d.copy(), n.copy()


def _heads(eng):
    im = eng.intermediates()
    return [im[k] for k in ("box_preds", "cls_preds", "dir_cls_preds")]


@pytest.mark.parametrize("case", [
    # block2 opens with stride 1 and twice the channels: its second layer writes 2x what its first reads per frame
    dict(B=8, strides=[2, 1, 2], filters=[64, 128, 256], upsample=[1, 1, 2], walked="block2.1"),
    # block2 opens with stride 2 and cout = 5 cin: a quarter of the pixels at five times the channels
    dict(B=32, strides=[2, 2, 2], filters=[32, 160, 256], upsample=[1, 2, 4], walked="block2.1"),
])
def test_subrange_walk_over_a_widening_block(pp, hip_lib, case):
    """Frame sub-ranges (pp_set_cache_budget) on a KITTI-sized grid whose block2 writes more bytes per frame than it
    reads: the run that is walked sub-batch by sub-batch must not overwrite input frames it has yet to read.  At the
    default budget (and at 1 MB) some of block2 is still walked in sub-ranges; head maps and detections are the bits of
    the unsplit launches (budget 0), and one frame matches the float64 oracle."""
    B, N = case["B"], 12000
    eng = pp.Engine(_widening_config(pp, B, case["strides"], case["filters"], case["upsample"]), max_batch=B,
                    max_points_per_frame=N)
    d = eng.d
    w = pp.weights.init_weights(d, seed=11)
    eng.load_weights(w)
    frames = [pp.synth.kitti_cloud(700 + i, N - 97 * i) for i in range(B)]
    eng.set_cache_budget(0)
    k0, d0, n0 = _launches(eng, frames, case["walked"])
    assert k0 == 1
    eng.detect(frames)
    h0 = _heads(eng)
    assert int(n0.sum()) > 0, "the frames must produce detections"
    for mb in (256, 1):
        eng.set_cache_budget(mb)
        k, d1, n1 = _launches(eng, frames, case["walked"])
        assert k > 1, f"budget {mb} MB: {case['walked']} must still be walked in sub-ranges ({k} launch)"
        assert np.array_equal(n1, n0) and d1.tobytes() == d0.tobytes(), f"budget {mb} MB: detections"
        d2, n2 = eng.detect(frames)                  # the graph path, too
        assert np.array_equal(n2, n0) and d2.tobytes() == d0.tobytes(), f"budget {mb} MB: detections (graph)"
        for a, b_ in zip(_heads(eng), h0):
            assert np.array_equal(a, b_), f"budget {mb} MB: head maps"
    eng.set_cache_budget(256)
    eng.detect(frames)
    im = eng.intermediates()
    b = 1
    ref = util_ref.oracle_detect(d, w, [frames[b]], *pp.synth.default_calib())
    fr = ref["frames"][0]
    P = fr["coordinates"].shape[0]
    assert im["n_pillars"][b] == P and np.array_equal(im["coors"][b, :P], fr["coordinates"])
    for k in ("box_preds", "cls_preds", "dir_cls_preds"):
        np.testing.assert_allclose(im[k][b], ref["preds"][k][0], rtol=0, atol=TOL, err_msg=k)
    eng.close()
