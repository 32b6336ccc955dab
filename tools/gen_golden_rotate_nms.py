"""Golden vectors of the rotated NMS from the reference's numba-CUDA kernel itself, run by the CUDA-model emulator of
tools/ref_shim.py (one Python thread per CUDA thread, a barrier for syncthreads, per-block shared arrays):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_rotate_nms.py      -> tests/golden/ref_rotate_nms.npz

  rotate_nms_gpu -> rotate_nms_kernel -> nms_postprocess   second/core/non_max_suppression/nms_gpu.py:419-490, :111-128
            (score sort, 64 x 64 block / thread indexing, shared-memory staging, bit masks, the host sweep)

The reference is imported at run time; only arrays are written.  Per case `<name>`: `<name>_dets` [n,6] float32
(x, y, x size, y size, angle, score), `<name>_args` float64 (threshold, pre_max_size or -1, post_max_size or -1) and
`<name>_keep` int64; `names` lists the cases.

Plain Python and real numba can differ in the last ulp of an IoU (the trig is evaluated at different widths), so every
random case is redrawn until no pair's rotated IoU lies within 1e-4 of its threshold -- the margin gen_golden_kernels.py
uses for the stand-up NMS -- and the hand-made ones are asserted to keep it: the fixture pins indexing and decisions,
not rounding.  The margins are taken on the project's C restatement of the IoU (oracle/c_oracle.py), in both argument
orders.  Scores are a shuffled permutation: no ties.

The caps have no rotated counterpart in the reference (its nms(), libraries/eval_helper_functions.py:463-492, wraps the
stand-up kernel only): the cap cases apply that function's steps -- the min(n, pre) best by score in, at most post out,
indices mapped back -- around rotate_nms_gpu.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402
from oracle import c_oracle  # noqa: E402

_, ng = ref_shim.load_reference_eval()
assert type(ng.rotate_nms_kernel).__name__ == "_CudaKernel"

MARGIN = 1e-4


def margin_ok(boxes, thr):
    """No pair's IoU, in either argument order, within MARGIN of thr (NaN: zero-area pairs decide nothing)."""
    if boxes.shape[0] < 2:
        return True
    iou = c_oracle.rotate_iou_eval(boxes[:, :5], boxes[:, :5], -1).astype(np.float64)
    off = ~np.eye(boxes.shape[0], dtype=bool)
    d = np.abs(iou[off] - thr)
    return bool(np.all(d[np.isfinite(d)] > MARGIN))


def scores_perm(rng, n):
    return ((rng.permutation(n).astype(np.float32) + 0.5) / max(n, 1)).astype(np.float32)


def random_boxes(rng, n):
    """Centres dense enough to overlap; a third of the boxes are jittered copies of another one (so that the high
    thresholds suppress too)."""
    side = 1.6 * np.sqrt(max(n, 1))
    b = np.concatenate([rng.uniform(0, side, (n, 2)), rng.uniform(0.5, 2.5, (n, 2)), rng.uniform(-3.5, 3.5, (n, 1))], axis=1)
    for i in range(n):
        if n > 2 and rng.random() < 0.33:
            j = int(rng.integers(0, n))
            if j != i:
                b[i] = b[j] + np.concatenate([rng.normal(0, 0.06, 2), rng.normal(0, 0.04, 2), rng.normal(0, 0.03, 1)])
    return b.astype(np.float32)


def run_reference(dets, thr, pre=None, post=None):
    """nms()'s steps around rotate_nms_gpu."""
    n = dets.shape[0]
    indices = np.arange(n)
    if pre is not None:
        m = min(n, pre)
        indices = np.argsort(-dets[:, 5], kind="stable")[:m]      # np.argpartition(scores, -m)[-m:] as a set; no ties
    sub = dets[indices]
    if len(sub) == 0:
        return np.zeros((0,), np.int64)
    keep = np.array(ng.rotate_nms_gpu(sub.copy(), np.float32(thr)), dtype=np.int64)
    if post is not None:
        keep = keep[:post]
    return indices[keep].astype(np.int64)


def line_fillers(n, x0=10.0):
    """n disjoint boxes on a line, far from the origin."""
    return np.array([[x0 + 3.0 * k, 20.0, 1.0, 1.0, 0.2 * k] for k in range(n)], dtype=np.float32).reshape(n, 5)


def hand_cases():
    c = {}
    A = [0.0, 0.0, 2.0, 1.0, 0.3]
    c["identical"] = (np.array([[0, 0, 2, 1, 0.0]] * 2, np.float32), [0.9, 0.8], 0.5)
    # the same turned by 0.3 rad: the float32 corner tests of the reference miss every corner and parallel edges do not
    # cross, so its IoU is 0 and both boxes stay -- pinned as the reference decides it
    c["identical_turned"] = (np.array([A, A], np.float32), [0.9, 0.8], 0.5)
    c["contained"] = (np.array([[0, 0, 4, 2, 0.4], [0.2, 0.1, 1, 0.5, 0.4]], np.float32), [0.9, 0.8], 0.1)
    c["contained_big_last"] = (np.array([[0.2, 0.1, 3, 1.5, 0.4], [0, 0, 4, 2, 0.4]], np.float32), [0.9, 0.8], 0.5)
    c["touching"] = (np.array([[0, 0, 2, 1, 0.0], [2, 0, 2, 1, 0.0]], np.float32), [0.9, 0.8], 0.1)
    c["octagon"] = (np.array([[0, 0, 2, 2, 0.0], [0, 0, 2, 2, np.pi / 4]], np.float32), [0.9, 0.8], 0.5)
    c["octagon_kept"] = (np.array([[0, 0, 2, 2, 0.0], [0, 0, 2, 2, np.pi / 4]], np.float32), [0.9, 0.8], 0.75)
    c["disjoint"] = (np.array([[0, 0, 2, 1, 0.3], [5, 5, 2, 1, 1.0], [-6, 2, 1, 1, 2.0]], np.float32), [0.5, 0.9, 0.7], 0.1)
    # chain: A removes B, C survives although IoU(B, C) > thr
    c["chain"] = (np.array([[0, 0, 2, 1, 0.0], [0.5, 0, 2, 1, 0.0], [1.0, 0, 2, 1, 0.0]], np.float32), [0.9, 0.8, 0.7], 0.4)
    # a suppressor at sorted position 0 whose victim sits two column blocks further
    n = 140
    b = np.concatenate([np.array([A], np.float32), line_fillers(n - 2), np.array([[0.05, 0.02, 2.0, 1.0, 0.3]], np.float32)])
    s = np.concatenate([[1.0], 0.9 - 0.005 * np.arange(n - 2), [0.9 - 0.005 * 130 - 0.0025]])   # victim at sorted position 131
    c["far_victim"] = (b, s, 0.5)
    # victims at sorted positions 63 and 64
    n = 70
    b = np.concatenate([np.array([A], np.float32), line_fillers(n - 3),
                        np.array([[0.05, 0.02, 2.0, 1.0, 0.3], [-0.04, 0.03, 2.0, 1.0, 0.28]], np.float32)])
    fs = 0.9 - 0.005 * np.arange(n - 3)
    s = np.concatenate([[1.0], fs, [fs[61] - 0.001, fs[61] - 0.002]])     # fillers 0..61 at positions 1..62, then the two
    c["victims_63_64"] = (b, s, 0.5)
    return c


def main():
    rng = np.random.default_rng(419)
    out, names = {}, []

    def store(name, dets, thr, pre, post, keep):
        out[name + "_dets"] = dets
        out[name + "_args"] = np.array([thr, -1 if pre is None else pre, -1 if post is None else post], dtype=np.float64)
        out[name + "_keep"] = keep
        names.append(name)
        print(f"{name}: n {dets.shape[0]} thr {thr} pre {pre} post {post}: {len(keep)} kept", flush=True)

    for thr in (0.1, 0.3, 0.5, 0.7):
        for n in (1, 2, 63, 64, 65, 100, 129, 200):
            while True:
                dets = np.concatenate([random_boxes(rng, n), scores_perm(rng, n)[:, None]], axis=1)
                if margin_ok(dets, thr):
                    break
            keep = run_reference(dets, thr)
            if n >= 63:
                assert 0 < len(keep) < n, (thr, n, len(keep))
            store(f"rand_t{thr}_n{n}", dets, thr, None, None, keep)

    for name, (boxes, scores, thr) in hand_cases().items():
        dets = np.concatenate([np.asarray(boxes, np.float32), np.asarray(scores, np.float32)[:, None]], axis=1)
        assert len(set(dets[:, 5].tolist())) == len(dets), name + ": score ties"
        assert margin_ok(dets, thr), name + ": an IoU within the margin of the threshold"
        store("hand_" + name, dets, thr, None, None, run_reference(dets, thr))
    srt = lambda nm: np.argsort(-out[nm + "_dets"][:, 5], kind="stable")
    assert len(out["hand_identical_keep"]) == 1 and len(out["hand_identical_turned_keep"]) == 2 and len(out["hand_touching_keep"]) == 2 and len(out["hand_octagon_keep"]) == 1
    assert len(out["hand_octagon_kept_keep"]) == 2 and len(out["hand_disjoint_keep"]) == 3
    assert out["hand_chain_keep"].tolist() == [0, 2]
    assert int(np.where(srt("hand_far_victim") == 139)[0][0]) >= 128 and 139 not in out["hand_far_victim_keep"]
    assert len(out["hand_far_victim_keep"]) == 139
    o = srt("hand_victims_63_64")
    assert sorted(o[[63, 64]].tolist()) == [68, 69] and len(out["hand_victims_63_64_keep"]) == 68

    for k, (n, pre, post, thr) in enumerate(((300, 100, 50, 0.5), (200, 1000, 100, 0.5), (90, 100, 300, 0.1), (150, 64, 5, 0.7),
                                             (40, None, 10, 0.5), (0, 100, 50, 0.5))):
        while True:
            dets = np.concatenate([random_boxes(rng, n), scores_perm(rng, n)[:, None]], axis=1).astype(np.float32).reshape(n, 6)
            if margin_ok(dets, thr):
                break
        store(f"cap_{k}", dets, thr, pre, post, run_reference(dets, thr, pre, post))
    store("empty", np.zeros((0, 6), np.float32), 0.5, None, None, np.zeros((0,), np.int64))
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ref_rotate_nms.npz"), **out)


if __name__ == "__main__":
    main()
