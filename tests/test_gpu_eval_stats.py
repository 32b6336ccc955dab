"""AP-evaluator statistics on the GPU (csrc/eval_stats.hip through pp_eval_match / pp_eval_pr) against the
reference's compute_statistics_jit / fused_compute_statistics (tests/golden/ref_eval_stats.npz) and against the
host loop over `compute_statistics` on the 57 frames of ref_kitti_eval.npz.

Counts and matched indices are compared exactly.  The similarity sum is float64 on both sides; with n the number
of terms summed, the bound is n * 2^-51 + n^2 * 2^-52: the device's cos and the host's may each be an ulp off on a
value in [-1, 1] (2 * 2^-53 per term after the halving, doubled for slack on both sides), and adding n non-negative
terms of at most 1 in another order moves the sum by at most (n - 1) * n * 2^-53.
"""
import numpy as np
import pytest

from conftest import load_golden

from test_eval_stats_host import fixture_frames
from test_kitti_eval import ORACLE_FNS, _annos

pytestmark = pytest.mark.gpu

NO_DETECTION = -10000000


def sim_tol(n):
    n = np.asarray(n, dtype=np.float64)
    return n * 2.0 ** -51 + n * n * 2.0 ** -52


def match_indices(ov, scores, ign_gt, ign_dt, mo):
    """Pass 1 as a scalar double loop: per ground truth the detection counted as a true positive, or -1."""
    D, G = ov.shape
    assigned = [False] * D
    out = []
    for i in range(G):
        if ign_gt[i] == -1:
            out.append(-1)
            continue
        det, best = -1, NO_DETECTION
        for j in range(D):
            if ign_dt[j] != -1 and not assigned[j] and ov[j, i] > mo and scores[j] > best:
                det, best = j, scores[j]
        if det >= 0:
            assigned[det] = True
        out.append(det if det >= 0 and ign_gt[i] == 0 and ign_dt[det] == 0 else -1)
    return out


@pytest.fixture(scope="module")
def golden():
    g = load_golden("ref_eval_stats.npz")
    fr = fixture_frames(g)
    return g, fr


def _pack(ke, fr, sel=None):
    idx = range(len(fr["gt"])) if sel is None else sel
    return ke.pack_frames(*[[fr[k][i] for i in idx] for k in ("overlaps", "gt", "dt", "ign_gt", "ign_dt", "dc")])


def _thresholds(g):
    K, T = len(g["min_overlaps"]), len(g["thresholds"])
    th = np.zeros((K, 41))
    th[:, :T] = g["thresholds"]
    return th, np.full(K, T, dtype=np.int32)


def test_match_against_reference_fixture(pp, hip_lib, golden):
    g, fr = golden
    ke = pp.kitti_eval
    packed = _pack(ke, fr)
    m = ke.match_frames_gpu(packed, g["min_overlaps"])
    assert m.dtype == np.int32 and m.shape == (2, g["num_gt"].sum())
    for k, mo in enumerate(g["min_overlaps"]):
        for f in range(packed["nframes"]):
            row = m[k, packed["gt_off"][f]:packed["gt_off"][f + 1]]
            want = match_indices(fr["overlaps"][f], fr["dt"][f][:, 5], fr["ign_gt"][f], fr["ign_dt"][f], mo)
            assert row.tolist() == want, (k, f)
            got_scores = fr["dt"][f][row[row >= 0], 5]
            assert np.array_equal(got_scores, g["tp_scores"][f, k, :g["tp_count"][f, k]]), (k, f)
        assert np.array_equal(ke.matched_scores(packed, m[k]),
                              np.concatenate([g["tp_scores"][f, k, :g["tp_count"][f, k]] for f in range(packed["nframes"])]))
    assert np.array_equal(m, ke.match_frames_gpu(packed, g["min_overlaps"]))


def test_pr_against_reference_fixture(pp, hip_lib, golden):
    g, fr = golden
    ke = pp.kitti_eval
    th, nt = _thresholds(g)
    T = int(nt[0])
    packed = _pack(ke, fr)
    singles = [_pack(ke, fr, [f]) for f in range(packed["nframes"])]
    for c, (metric, aos) in enumerate(zip(g["case_metric"], g["case_aos"])):
        want = g["stats"][c].copy()                        # [frame, tier, threshold, 4]
        want[..., 3] = np.where(want[..., 3] == -1, 0.0, want[..., 3])
        pr = ke.pr_frames_gpu(packed, g["min_overlaps"], th, nt, int(metric), bool(aos))
        assert pr.shape == (2, 41, 4) and not pr[:, T:].any()
        assert np.array_equal(pr[:, :T, :3], g["fused"][c][..., :3]), c
        assert np.array_equal(pr[:, :T, :3], want[..., :3].sum(0)), c
        err = np.abs(pr[:, :T, 3] - g["fused"][c][..., 3])
        print(f"case {c}: similarity |delta| max {err.max():.3e}, bound min {sim_tol(pr[:, :T, 0]).min():.3e}")
        assert (err <= sim_tol(pr[:, :T, 0])).all(), c
        if not aos:
            assert not pr[..., 3].any()
        for f, one in enumerate(singles):                  # and frame by frame
            prf = ke.pr_frames_gpu(one, g["min_overlaps"], th, nt, int(metric), bool(aos))
            assert np.array_equal(prf[:, :T, :3], want[f][..., :3]), (c, f)
            assert (np.abs(prf[:, :T, 3] - want[f][..., 3]) <= sim_tol(prf[:, :T, 0])).all(), (c, f)


def test_partial_threshold_counts_leave_zero_slots(pp, hip_lib, golden):
    g, fr = golden
    ke = pp.kitti_eval
    th, nt = _thresholds(g)
    full = ke.pr_frames_gpu(_pack(ke, fr), g["min_overlaps"], th, nt, 0, True)
    nt2 = np.array([3, 0], dtype=np.int32)
    part = ke.pr_frames_gpu(_pack(ke, fr), g["min_overlaps"], th, nt2, 0, True)
    assert np.array_equal(part[0, :3], full[0, :3]) and not part[0, 3:].any() and not part[1].any()


@pytest.fixture(scope="module")
def kitti(pp):
    g = load_golden("ref_kitti_eval.npz")
    gts, dts = _annos(g)
    return g, gts, dts


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_against_the_host_loop(pp, hip_lib, kitti, metric):
    _, gts, dts = kitti
    ke = pp.kitti_eval
    overlaps, _, _, _ = ke.calculate_iou_partly(dts, gts, metric, overlap_fns=ORACLE_FNS)
    tiers = ke.official_min_overlaps()[[0, 1, 3], metric, 1]
    for difficulty in (0, 2):
        gt_list, dt_list, ign_gt, ign_dt, dcs, total_valid = ke._prepare_data(gts, dts, 1, difficulty)
        packed = ke.pack_frames(overlaps, gt_list, dt_list, ign_gt, ign_dt, dcs)
        m = ke.match_frames_gpu(packed, tiers)
        th, nt = np.zeros((3, 41)), np.zeros(3, dtype=np.int32)
        for k, mo in enumerate(tiers):
            host_scores, want = [], []
            for i in range(len(gts)):
                host_scores += ke.compute_statistics(overlaps[i], gt_list[i], dt_list[i], ign_gt[i], ign_dt[i], dcs[i],
                                                     metric, mo, 0.0, False)[4].tolist()
                want += match_indices(overlaps[i], dt_list[i][:, 5], ign_gt[i], ign_dt[i], mo)
            assert m[k].tolist() == want, (difficulty, k)
            assert ke.matched_scores(packed, m[k]).tolist() == host_scores, (difficulty, k)
            t = ke.get_thresholds(np.array(host_scores), total_valid)
            nt[k] = len(t)
            th[k, :len(t)] = t
        assert nt.max() > 5
        pr = ke.pr_frames_gpu(packed, tiers, th, nt, metric, True)
        for k, mo in enumerate(tiers):
            want = np.zeros((41, 4))
            for i in range(len(gts)):
                for t in range(nt[k]):
                    tp, fp, fn, sim, _ = ke.compute_statistics(overlaps[i], gt_list[i], dt_list[i], ign_gt[i], ign_dt[i],
                                                               dcs[i], metric, mo, th[k, t], True, True)
                    want[t] += (tp, fp, fn, sim if sim != -1 else 0.0)
            assert np.array_equal(pr[k, :, :3], want[:, :3]), (difficulty, k)
            assert (np.abs(pr[k, :, 3] - want[:, 3]) <= sim_tol(want[:, 0])).all(), (difficulty, k)


@pytest.fixture(scope="module")
def gpu_reports(pp, hip_lib, kitti):
    _, gts, dts = kitti
    ke = pp.kitti_eval
    one = ke.get_official_eval_result(gts, dts, ["Pedestrian"], compute_bbox=False, statistics="gpu", overlap_fns=ORACLE_FNS)
    two = ke.get_official_eval_result(gts, dts, ["Pedestrian", "Cyclist"], difficultys=[0, 1, 2], compute_bbox=True,
                                      statistics="gpu", overlap_fns=ORACLE_FNS)
    return one, two


def test_reports_equal_the_reference(kitti, gpu_reports):
    g = kitti[0]
    (text, mbbox, mbev, m3d, maos), (text2, b2, bev2, d32, aos2) = gpu_reports
    assert mbbox is None and text == str(g["official_text"])
    for got, key in ((mbev, "official_bev"), (m3d, "official_3d"), (maos, "official_aos")):
        np.testing.assert_allclose(got, g[key], rtol=0, atol=1e-9)
    assert text2 == str(g["official2_text"])
    for got, key in ((b2, "official2_bbox"), (bev2, "official2_bev"), (d32, "official2_3d"), (aos2, "official2_aos")):
        np.testing.assert_allclose(got, g[key], rtol=0, atol=1e-9, equal_nan=True)


def test_count_metrics_are_bit_identical_to_the_host_path(pp, kitti, gpu_reports):
    """bbox / bev / 3d come from integer counts alone.  One host evaluation serves both reports: the single-class
    report is the first class of the two-class one."""
    _, gts, dts = kitti
    (_, _, mbev, m3d, _), (_, b2, bev2, d32, _) = gpu_reports
    _, hb2, hbev2, hd32, _ = pp.kitti_eval.get_official_eval_result(gts, dts, ["Pedestrian", "Cyclist"], difficultys=[0, 1, 2],
                                                                    compute_bbox=True, overlap_fns=ORACLE_FNS)
    assert b2.tobytes() == hb2.tobytes() and bev2.tobytes() == hbev2.tobytes() and d32.tobytes() == hd32.tobytes()
    assert mbev.tobytes() == hbev2[:1].tobytes() and m3d.tobytes() == hd32[:1].tobytes()


def test_coco_report_equals_the_reference(pp, hip_lib, kitti):
    g, gts, dts = kitti
    assert pp.kitti_eval.get_coco_eval_result(gts, dts, ["Pedestrian"], overlap_fns=ORACLE_FNS,
                                              statistics="gpu") == str(g["coco_text"])


def test_two_calls_return_the_same_bytes(pp, hip_lib, golden):
    g, fr = golden
    ke = pp.kitti_eval
    th, nt = _thresholds(g)
    packed = _pack(ke, fr)
    a = ke.pr_frames_gpu(packed, g["min_overlaps"], th, nt, 0, True)
    b = ke.pr_frames_gpu(packed, g["min_overlaps"], th, nt, 0, True)
    assert a.tobytes() == b.tobytes() and a[..., 3].any()
    ms = []
    ke.match_frames_gpu(packed, g["min_overlaps"], kernel_ms=ms)
    ke.pr_frames_gpu(packed, g["min_overlaps"], th, nt, 0, True, kernel_ms=ms)
    assert len(ms) == 2 and all(0.0 < x < 1000.0 for x in ms)


def test_edges(pp, hip_lib):
    ke = pp.kitti_eval
    th, nt = np.zeros((2, 41)), np.array([4, 4], dtype=np.int32)
    tiers = [0.5, 0.7]
    none = ke.pack_frames([], [], [], [], [], [])
    assert ke.match_frames_gpu(none, tiers).shape == (2, 0)
    assert not ke.pr_frames_gpu(none, tiers, th, nt, 0, True).any()
    e = lambda *s: np.zeros(s)  # noqa: E731
    empty = ke.pack_frames([e(0, 0)] * 3, [e(0, 5)] * 3, [e(0, 6)] * 3, [[]] * 3, [[]] * 3, [e(0, 4)] * 3)
    assert ke.match_frames_gpu(empty, tiers).shape == (2, 0)
    assert not ke.pr_frames_gpu(empty, tiers, th, nt, 0, True).any()
    # ground truths without any detection are all misses; detections without ground truth are all false positives
    only_gt = ke.pack_frames([e(0, 3)], [e(3, 5)], [e(0, 6)], [[0, 1, 0]], [[]], [e(0, 4)])
    assert ke.match_frames_gpu(only_gt, tiers).tolist() == [[-1] * 3] * 2
    pr = ke.pr_frames_gpu(only_gt, tiers, th, nt, 1, False)
    assert pr[:, :4].tolist() == [[[0.0, 0.0, 2.0, 0.0]] * 4] * 2
    dt = e(70, 6)
    dt[:, 5] = 0.5
    only_dt = ke.pack_frames([e(70, 0)], [e(0, 5)], [dt], [[]], [[0] * 69 + [1]], [e(0, 4)])
    pr = ke.pr_frames_gpu(only_dt, tiers, th, nt, 1, False)
    assert pr[:, :4].tolist() == [[[0.0, 69.0, 0.0, 0.0]] * 4] * 2
    big = ke.pack_frames([e(1025, 1)], [e(1, 5)], [e(1025, 6)], [[0]], [[0] * 1025], [e(0, 4)])
    with pytest.raises(RuntimeError, match="1024"):
        ke.match_frames_gpu(big, tiers)
    with pytest.raises(RuntimeError, match="1024"):
        ke.pr_frames_gpu(big, tiers, th, nt, 1, False)
    full = ke.pack_frames([e(1024, 2)], [e(2, 5)], [e(1024, 6)], [[0, 0]], [[0] * 1024], [e(0, 4)])
    assert ke.match_frames_gpu(full, tiers).tolist() == [[-1, -1]] * 2       # the limit itself is served
    with pytest.raises(ValueError, match="statistics"):
        ke.get_official_eval_result([], [], ["Pedestrian"], statistics="bogus")
