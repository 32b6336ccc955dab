"""Feeds that cross between the streams back to back (all `-m gpu`, through the C-ABI).

The voxeliser's scratch (cells, keys, sorted indices) exists once per handle, while a pass voxelises on the main stream
(zero-copy feed of <= 4 frames, synchronous and device uploads) or on the copy stream right behind its upload (copy feed
of more frames): batches that cross that boundary with no sync in between must give the bits of the same frames fed one
batch at a time.  torch is imported first, so that -- as in a training process, and in the whole suite -- the library
runs on the HIP runtime torch brings: there, replayed zero-copy passes over frames of more than 16 384 points went wrong
while the voxeliser's clear was a memset node of the graph (k_fill_first in voxelize.hip).
"""
import ctypes as C

import torch  # noqa: F401  (before the library is loaded: see above)
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ZC_MAX = 4          # ZC_MAX_BATCH (pp_api.hip): larger batches take the copy feed


def _snapshot(eng):
    """detections + the intermediates of the pass the handle last ran (waits for it)"""
    d, n = eng.detections()
    im = eng.intermediates()
    return d.copy(), n.copy(), im


def _assert_same(got, want, what):
    d, n, im = got
    wd, wn, wim = want
    B = len(wn)
    assert np.array_equal(n[:B], wn), (what, n[:B], wn)
    for b in range(B):                              # rows past a frame's count are not defined
        assert d[b, :n[b]].tobytes() == wd[b, :wn[b]].tobytes(), (what, "detections", b)
    assert np.array_equal(im["n_pillars"][:B], wim["n_pillars"]), (what, "n_pillars")
    for b in range(B):
        P = int(wim["n_pillars"][b])
        assert np.array_equal(im["coors"][b, :P], wim["coors"][b, :P]), (what, "coors", b)
        assert np.array_equal(im["num_points"][b, :P], wim["num_points"][b, :P]), (what, "num_points", b)
    for k in ("box_preds", "cls_preds", "dir_cls_preds"):
        assert np.array_equal(im[k][:B], wim[k]), (what, k)


def _mixed_feed_engine(pp):
    B = 8
    eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=32768)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    # zero-copy batches of large frames (a long voxeliser on the main stream) and copy-feed batches of small frames (a
    # short DMA ahead of the voxeliser on the copy stream)
    shapes = [(3, 32000), (6, 1500), (4, 30000), (8, 1200), (2, 32768), (5, 2000)]
    sets = [[pp.synth.d435i_cloud(500 + 10 * k + i, npts - 37 * i) for i in range(nb)] for k, (nb, npts) in enumerate(shapes)]
    assert [len(s) <= ZC_MAX for s in sets] == [True, False] * 3
    want = []
    for fr in sets:                                  # one batch at a time, synchronous feed
        eng.detect(fr)
        want.append(_snapshot(eng))
    return eng, sets, want


def test_mixed_zero_copy_and_copy_feeds_back_to_back(pp, hip_lib):
    """upload_async alternating between batches of <= 4 frames (zero-copy feed: voxelised on the main stream) and of
    5..8 frames (copy feed: voxelised on the copy stream right behind the DMA), on an engine with max_batch = 8.  The
    copy-stream voxeliser of pass k+1 must wait for the main-stream voxeliser of pass k (the scratch exists once), and
    the main-stream one of k+1 for the copy-stream one of k."""
    eng, sets, want = _mixed_feed_engine(pp)
    stg = [eng.staging(fr) for fr in sets]
    for k in range(len(stg)):                        # capture every graph key once (an LRU eviction syncs the stream)
        eng.upload_async(stg[k])
        eng.detect_async()
    eng.sync()
    # 1. pipelined: upload k+1 is queued before pass k is read, so every pass is checked -- the zero-copy passes are
    # the ones a copy-stream voxeliser could overwrite, the copy-feed passes the ones a main-stream voxeliser could
    order = [k % len(stg) for k in range(4 * len(stg))]
    eng.upload_async(stg[order[0]])
    eng.detect_async()
    for i in range(1, len(order)):
        eng.upload_async(stg[order[i]])
        _assert_same(_snapshot(eng), want[order[i - 1]], ("pipelined", i - 1, order[i - 1]))
        eng.detect_async()
    _assert_same(_snapshot(eng), want[order[-1]], ("pipelined", len(order) - 1, order[-1]))
    # 2. back to back with no read in between; the last pass is checked, ending once on each feed
    for last in (len(stg) - 1, len(stg) - 2):        # a copy-feed batch last, then a zero-copy one
        run = [k % len(stg) for k in range(last + 1 + 3 * len(stg))]
        assert len(run) >= 20 and run[-1] == last
        for k in run:
            eng.upload_async(stg[k])
            eng.detect_async()
        _assert_same(_snapshot(eng), want[last], ("back to back", last))
    eng.sync()
    for s_ in stg:
        s_.close()
    eng.close()


def test_synchronous_and_device_feeds_then_copy_feed(pp, hip_lib):
    """upload (synchronous) or upload_device -> detect_async -> upload_async of other frames (copy feed) -> read the
    first pass -> detect_async -> read the second, with no sync before the copy-stream voxeliser is queued."""
    hip = C.CDLL("libamdhip64.so")            # the process's one HIP runtime (pp_amd._lib._one_hip_runtime)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def ok(rc):
        assert rc == 0, f"hip error {rc}"
    eng, sets, want = _mixed_feed_engine(pp)
    big = [k for k, s in enumerate(sets) if len(s) <= ZC_MAX]
    small = [k for k, s in enumerate(sets) if len(s) > ZC_MAX]
    stg = {k: eng.staging(sets[k]) for k in small}
    devs = {}
    for k in big:
        pts = np.ascontiguousarray(np.concatenate(sets[k], axis=0), np.float32)
        offs = np.concatenate([[0], np.cumsum([f.shape[0] for f in sets[k]])]).astype(np.int32)
        p = C.c_void_p()
        ok(hip.hipMalloc(C.byref(p), pts.nbytes))
        ok(hip.hipMemcpy(p, pts.ctypes.data_as(C.c_void_p), pts.nbytes, 1))
        devs[k] = (p, offs)
    try:
        for rep in range(4):
            for i, (kb, ks) in enumerate(zip(big, small)):
                if (rep + i) % 2 == 0:
                    eng.upload(sets[kb])
                else:
                    eng.upload_device(devs[kb][0].value, devs[kb][1])
                eng.detect_async()
                eng.upload_async(stg[ks])
                _assert_same(_snapshot(eng), want[kb], ("sync/device feed", rep, kb))
                eng.detect_async()
                _assert_same(_snapshot(eng), want[ks], ("copy feed after it", rep, ks))
    finally:
        eng.sync()
        for s_ in stg.values():
            s_.close()
        eng.close()
        for p, _ in devs.values():
            ok(hip.hipFree(p))
