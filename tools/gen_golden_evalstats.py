"""Golden vectors for the AP evaluator's matching statistics, produced by RUNNING the
reference's own compute_statistics_jit and fused_compute_statistics (second/utils/eval.py:166-345) as plain
Python (build container only; numba decorators are identity stubs, tools/ref_shim.py).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_evalstats.py
      -> tests/golden/ref_eval_stats.npz

Synthetic frames built to hit the rules of the greedy matching: detection counts around the 64-lane chunk (0, 1,
63, 64, 65, 130), overlaps from a small set (ties, values equal to min_overlap), scores from 8 values that are also
the thresholds (score ties, score == thresh), one score at the NO_DETECTION sentinel, ignore flags from {-1, 0, 1},
DontCare boxes covering detections by exactly / more than / less than min_overlap.

Stored: the inputs (flat, with per-frame counts), per (case, frame, min_overlap, thresh) tp / fp / fn / similarity
as compute_statistics_jit returns them (similarity -1 included), fused_compute_statistics' totals over all frames,
and the true-positive scores of the pass without thresholds.  The generator also asserts that the project's host
compute_statistics returns the same values on every case.
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

ev, _ = ref_shim.load_reference_eval()
host = importlib.import_module("pp_amd").kitti_eval

rng = np.random.default_rng(4117)
OVERLAP_SET = np.array([0.0, 0.3, 0.5, 0.55, 0.7, 0.9])
OVERLAP_P = np.array([0.55, 0.09, 0.09, 0.09, 0.09, 0.09])
SCORE_SET = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8])
MIN_OVERLAPS = np.array([0.5, 0.7])
THRESHOLDS = SCORE_SET.copy()
CASES = [(0, False), (0, True), (1, False), (1, True)]       # (metric, compute_aos)
SENTINEL = -10000000.0

# (detections, ground truths) per frame: the chunk edges, the empty corners, then seeded small frames
SHAPES = [(0, 0), (0, 3), (5, 0), (1, 1), (63, 7), (64, 9), (65, 11), (130, 40), (128, 1), (1, 40), (64, 40), (66, 2)]
while len(SHAPES) < 40:
    SHAPES.append((int(rng.integers(0, 24)), int(rng.integers(0, 12))))


def make_frame(f, D, G):
    ov = rng.choice(OVERLAP_SET, size=(D, G), p=OVERLAP_P)
    scores = rng.choice(SCORE_SET, size=D)
    if f == 7 and D:
        scores[3] = SENTINEL                                   # overlaps ground truths, can never win pass 1
        ov[3, :] = 0.9
    ign_gt = rng.choice([-1, 0, 1], size=G, p=[0.15, 0.6, 0.25]).astype(np.int64)
    ign_dt = rng.choice([-1, 0, 1], size=D, p=[0.15, 0.6, 0.25]).astype(np.int64)
    x1 = rng.integers(0, 60, D).astype(np.float64) * 10
    y1 = rng.integers(0, 20, D).astype(np.float64) * 10
    w = rng.choice([10.0, 20.0, 40.0], D)
    h = rng.choice([10.0, 20.0], D)
    dt_box = np.stack([x1, y1, x1 + w, y1 + h], 1).reshape(D, 4)
    dcs = []
    if D and f % 3 != 1:                                       # DontCare regions over some detections
        for j in rng.choice(D, size=min(D, 1 + f % 4), replace=False):
            frac = rng.choice([0.5, 0.7, 0.8, 1.0, 0.3])       # exactly min_overlap, above, below
            b = dt_box[j].copy()
            b[2] = b[0] + frac * (b[2] - b[0])
            dcs.append(b)
    dc = np.stack(dcs, 0) if dcs else np.zeros((0, 4))
    gt = np.concatenate([rng.uniform(0, 600, (G, 4)), rng.uniform(-np.pi, np.pi, (G, 1))], 1)
    dt = np.concatenate([dt_box, rng.uniform(-np.pi, np.pi, (D, 1)), scores.reshape(D, 1)], 1)
    return ov, gt, dt, ign_gt, ign_dt, dc


frames = [make_frame(f, D, G) for f, (D, G) in enumerate(SHAPES)]
N, K, T = len(frames), len(MIN_OVERLAPS), len(THRESHOLDS)
maxg = max(G for _, G in SHAPES)
stats = np.zeros((len(CASES), N, K, T, 4))
tp_scores = np.full((N, K, maxg), np.nan)
tp_count = np.zeros((N, K), dtype=np.int64)
fused = np.zeros((len(CASES), K, T, 4))


def same(a, b, what):
    assert a[:3] == b[:3] and float(a[3]) == float(b[3]) and np.array_equal(a[4], b[4]), (what, a, b)


for f, (ov, gt, dt, ig, idt, dc) in enumerate(frames):
    for k, mo in enumerate(MIN_OVERLAPS):
        for metric in (0, 1):
            ref = ev.compute_statistics_jit(ov, gt, dt, ig, idt, dc, metric, mo, 0.0, False)
            mine = host.compute_statistics(ov, gt, dt, ig, idt, dc, metric, mo, 0.0, False)
            same(ref, mine, ("pass 1", f, mo, metric))
        tp_count[f, k] = len(ref[4])
        tp_scores[f, k, :len(ref[4])] = ref[4]
        for c, (metric, aos) in enumerate(CASES):
            for t, th in enumerate(THRESHOLDS):
                ref = ev.compute_statistics_jit(ov, gt, dt, ig, idt, dc, metric, mo, th, True, aos)
                mine = host.compute_statistics(ov, gt, dt, ig, idt, dc, metric, mo, th, True, aos)
                same(ref, mine, ("pass 2", f, mo, th, metric, aos))
                stats[c, f, k, t] = ref[:4]

# fused_compute_statistics over all frames at once (overlaps as the block-diagonal "part" it slices)
nd = np.array([D for D, _ in SHAPES], dtype=np.int64)
ng = np.array([G for _, G in SHAPES], dtype=np.int64)
nc = np.array([fr[5].shape[0] for fr in frames], dtype=np.int64)
big = np.zeros((nd.sum(), ng.sum()))
di = gi = 0
for (ov, *_), D, G in zip(frames, nd, ng):
    big[di:di + D, gi:gi + G] = ov
    di, gi = di + D, gi + G
cat = lambda i, w: np.concatenate([fr[i].reshape(-1, w) if w else fr[i] for fr in frames], 0)  # noqa: E731
gt_all, dt_all, dc_all = cat(1, 5), cat(2, 6), cat(5, 4)
ig_all, idt_all = cat(3, 0), cat(4, 0)
for c, (metric, aos) in enumerate(CASES):
    for k, mo in enumerate(MIN_OVERLAPS):
        pr = np.zeros((T, 4))
        ev.fused_compute_statistics(big, pr, ng, nd, nc, gt_all, dt_all, dc_all, ig_all, idt_all, metric,
                                    min_overlap=mo, thresholds=THRESHOLDS, compute_aos=aos)
        fused[c, k] = pr

out = os.path.join(ROOT, "tests", "golden", "ref_eval_stats.npz")
np.savez_compressed(
    out, num_dt=nd, num_gt=ng, num_dc=nc, gt_datas=gt_all, dt_datas=dt_all, dc_bboxes=dc_all, ignored_gt=ig_all,
    ignored_det=idt_all, overlaps=np.concatenate([fr[0].reshape(-1) for fr in frames]), min_overlaps=MIN_OVERLAPS,
    thresholds=THRESHOLDS, case_metric=np.array([m for m, _ in CASES]), case_aos=np.array([a for _, a in CASES]),
    stats=stats, fused=fused, tp_scores=tp_scores, tp_count=tp_count)
print(out, os.path.getsize(out), "bytes;", N, "frames; tp total", stats[0, :, :, :, 0].sum(), "fp", stats[0, :, :, :, 1].sum(),
      "stuff removed", (stats[2, ..., 1] - stats[0, ..., 1]).sum(), "similarity -1 cases", int((stats[1, ..., 3] == -1).sum()))
