"""Golden vectors of Soft-NMS from the reference's soft_nms_jit itself (second/core/non_max_suppression/nms_cpu.py:79-169),
imported at run time through tools/ref_shim.py (numba's decorators as identities) and run unmodified:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_soft_nms.py      -> tests/golden/ref_soft_nms.npz

Only arrays are written.  Per case `<name>`: `<name>_dets` [n,5] float32 (x1, y1, x2, y2, score), `<name>_args` float64
(method, sigma, Nt, threshold, pre_max_size or -1, post_max_size or -1) and `<name>_kept` [N,5] float32, the rows the
reference leaves in boxes[:N] -- selection order, final scores; `names` lists the cases.  The reference's keep list is
range(N) and its in-place swaps lose the original indices, so rows are identified by their coordinates (every case has
pairwise distinct boxes, except the hand-made identical pair).

Plain Python under NumPy 2 keeps float32 + 1 in float32 where numba widens to float64 (the caveat ref_shim.py documents), so
the reference's scores here differ from numba's -- and from pp_amd.soft_nms.soft_nms_np, which follows numba's typing -- in
the last float32 bits.  The fixture therefore pins decisions, order and row identity exactly and scores to a recorded
tolerance: `max_rel_score_diff` is the largest relative difference between the two over all cases, asserted below 2.5e-6.
No decision may hang on that: random cases are redrawn (at most 200 times) until soft_nms_np's decision_margins give every
selection gap > 1e-5, every |ov - Nt| > 1e-4 (the margin of the sibling generators) and every |re-scored value - floor|
> 1e-6; the hand-made cases are asserted to keep the same margins.

The caps have no counterpart in soft_nms_jit: the cap cases apply the steps of nms() (libraries/eval_helper_functions.py:
463-492) around it, as gen_golden_rotate_nms.py does -- the min(n, pre) best by score in, at most post out.
"""
import importlib
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

ref_shim.install()
nms_cpu = importlib.import_module("second.core.non_max_suppression.nms_cpu")
import pp_amd  # noqa: E402

sn = pp_amd.soft_nms
GAP, IOU, FLOOR, MAX_DRAWS, MAX_REL = 1e-5, 1e-4, 1e-6, 200, 2.5e-6
DEFAULT = (0.5, 0.3, 0.001)      # sigma, Nt, threshold: soft_nms_jit's defaults


def random_dets(rng, n):
    """Pixel-scale boxes dense enough to overlap; a third are jittered copies of another one; distinct scores."""
    side = 45.0 * np.sqrt(max(n, 1))
    xy = rng.uniform(0, side, (n, 2))
    wh = rng.uniform(10.0, 60.0, (n, 2))
    b = np.concatenate([xy, xy + wh], axis=1)
    for i in range(n):
        if n > 2 and rng.random() < 0.33:
            j = int(rng.integers(0, n))
            if j != i:
                b[i] = b[j] + rng.normal(0, 4.0, 4)
    s = rng.uniform(0.02, 1.0, n)
    return np.concatenate([b, s[:, None]], axis=1).astype(np.float32).reshape(n, 5)


def margins_ok(dets, method, sigma, nt, thr, pre=None, post=None):
    if len(set(map(tuple, dets[:, :4].tolist()))) != len(dets) or len(set(dets[:, 4].tolist())) != len(dets):
        return False
    m = sn.decision_margins(dets, method, sigma, nt, thr, pre, post)
    return m["gap"] > GAP and m["iou"] > IOU and m["floor"] > FLOOR


def run_reference(dets, method, sigma, nt, thr, pre=None, post=None):
    """nms()'s steps around soft_nms_jit: the kept rows [N,5]."""
    sub = dets
    if pre is not None and pre < len(dets):
        sub = dets[np.sort(np.argsort(-dets[:, 4], kind="stable")[:pre])]      # np.argpartition(...) as a set; no ties
    boxes = np.ascontiguousarray(sub, dtype=np.float32).copy()
    keep = nms_cpu.soft_nms_jit(boxes, np.float32(sigma), np.float32(nt), np.float32(thr), np.uint32(method))
    assert list(keep) == list(range(len(keep)))
    kept = boxes[:len(keep)]
    return kept[:post].copy() if post is not None else kept.copy()


def hand_cases():
    """name -> (boxes, scores, method, sigma, Nt, threshold)."""
    c = {}
    for m in (0, 1, 2):
        c[f"identical_m{m}"] = ([[5, 5, 40, 30]] * 2, [0.9, 0.8], m, *DEFAULT)
    # more than 1 apart in x: iw = 10 - 11.5 + 1 <= 0, nothing is re-scored; likewise in y
    c["apart_x"] = ([[0, 0, 10, 10], [11.5, 0, 20, 10]], [0.9, 0.8], 2, *DEFAULT)
    c["apart_y"] = ([[0, 0, 10, 10], [0, 11.5, 10, 20]], [0.9, 0.8], 2, *DEFAULT)
    # exactly touching under the +1 convention: iw = 10 - 10.5 + 1 = 0.5 > 0, so the neighbour is re-scored
    c["half_apart_x"] = ([[0, 0, 10, 10], [10.5, 0, 20, 10]], [0.9, 0.8], 2, *DEFAULT)
    # starts below the floor and overlaps the selected box a little (linear, ov <= Nt: weight 1): dropped all the same
    c["below_floor_overlapping"] = ([[0, 0, 30, 30], [25, 25, 60, 60]], [0.9, 0.0005], 1, *DEFAULT)
    # starts below the floor and overlaps nothing: never re-scored, kept
    c["below_floor_alone"] = ([[0, 0, 30, 30], [100, 100, 130, 130]], [0.9, 0.0005], 1, *DEFAULT)
    # D is decayed by A, B and C in turn (Gaussian, ov = 0.512 each): 0.2 -> 0.118 -> 0.070 -> 0.041 < floor 0.05
    D = [20, 20, 50, 50]
    c["accumulated_decay"] = ([[10, 20, 40, 50], [30, 20, 60, 50], [20, 30, 50, 60], D], [0.9, 0.8, 0.7, 0.2], 2, 0.5, 0.3, 0.05)
    c["accumulated_decay_two"] = ([[10, 20, 40, 50], [30, 20, 60, 50], D], [0.9, 0.8, 0.2], 2, 0.5, 0.3, 0.05)
    return c


def main():
    rng = np.random.default_rng(79)
    out, names = {}, []
    worst = 0.0

    def store(name, dets, method, sigma, nt, thr, pre=None, post=None):
        nonlocal worst
        kept = run_reference(dets, method, sigma, nt, thr, pre, post)
        keep, scores = sn.soft_nms_np(dets, method, sigma, nt, thr, pre, post)
        assert len(keep) == len(kept) and np.array_equal(dets[keep, :4], kept[:, :4]), name + ": the restatement disagrees"
        if len(keep):
            rel = float(np.max(np.abs(scores.astype(np.float64) - kept[:, 4]) / np.abs(kept[:, 4].astype(np.float64))))
            worst = max(worst, rel)
        out[name + "_dets"] = dets
        out[name + "_args"] = np.array([method, sigma, nt, thr, -1 if pre is None else pre, -1 if post is None else post], np.float64)
        out[name + "_kept"] = kept
        names.append(name)
        print(f"{name}: n {len(dets)} method {method} sigma {sigma} Nt {nt} floor {thr} pre {pre} post {post}: {len(kept)} kept", flush=True)

    def draw(n, method, sigma, nt, thr, pre=None, post=None):
        for k in range(MAX_DRAWS):
            dets = random_dets(rng, n)
            if margins_ok(dets, method, sigma, nt, thr, pre, post):
                return dets
        raise AssertionError(f"n {n} method {method}: no draw with the margins in {MAX_DRAWS}")

    for method in (0, 1, 2):
        for n in (0, 1, 2, 7, 33, 64, 65, 100, 300):
            store(f"rand_m{method}_n{n}", draw(n, method, *DEFAULT), method, *DEFAULT)
        for n in (33, 100):
            store(f"sig03_nt05_m{method}_n{n}", draw(n, method, 0.3, 0.5, 0.001), method, 0.3, 0.5, 0.001)
            store(f"floor005_m{method}_n{n}", draw(n, method, 0.5, 0.3, 0.05), method, 0.5, 0.3, 0.05)
    for name, (boxes, scores, method, sigma, nt, thr) in hand_cases().items():
        dets = np.concatenate([np.asarray(boxes, np.float32), np.asarray(scores, np.float32)[:, None]], axis=1)
        m = sn.decision_margins(dets, method, sigma, nt, thr)
        assert m["gap"] > GAP and m["iou"] > IOU and m["floor"] > FLOOR, (name, m)
        store("hand_" + name, dets, method, sigma, nt, thr)
    k = lambda nm: len(out["hand_" + nm + "_kept"])
    assert k("identical_m0") == 1 and k("identical_m1") == 1 and k("identical_m2") == 2
    assert k("apart_x") == 2 and k("apart_y") == 2 and out["hand_apart_x_kept"][1, 4] == np.float32(0.8)
    assert k("half_apart_x") == 2 and out["hand_half_apart_x_kept"][1, 4] < np.float32(0.8)
    assert k("below_floor_overlapping") == 1 and k("below_floor_alone") == 2
    assert k("accumulated_decay") == 3 and k("accumulated_decay_two") == 3
    assert out["hand_accumulated_decay_two_kept"][2, 4] > 0.05

    for i, (n, method, pre, post) in enumerate(((150, 2, 64, None), (90, 1, None, 10), (300, 2, 100, 50), (40, 0, 100, 100))):
        dets = draw(n, method, *DEFAULT, pre, post)
        store(f"cap_{i}", dets, method, *DEFAULT, pre, post)
        free = sn.soft_nms_np(dets, method, *DEFAULT)[0]
        if post is not None and post < n:
            assert len(out[f"cap_{i}_kept"]) == post < len(free), "the post cap must bind"
        if pre is not None and pre < n:
            capped = sn.soft_nms_np(dets, method, *DEFAULT, pre, None)[0]
            assert len(capped) < len(free) or not np.array_equal(capped, free[:len(capped)]), "the pre cap must bind"

    assert worst < MAX_REL, worst
    print(f"max_rel_score_diff {worst:.3e}")
    out["max_rel_score_diff"] = np.array(worst, np.float64)
    out["names"] = np.array(names)
    # np.savez_compressed stamps every member with the time of day; fixed stamps make a rerun give the committed bytes
    with zipfile.ZipFile(os.path.join(ROOT, "tests", "golden", "ref_soft_nms.npz"), "w", zipfile.ZIP_DEFLATED) as z:
        for key, value in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    main()
