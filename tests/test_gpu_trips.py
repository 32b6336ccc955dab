"""The data-path stages past one trip of their scan, carry and strided loops (tests/trip_cases.py lists the loops): the
frustum crop over more than 16 frames and more than 64 chunks a frame, the sweep accumulation over segments of more than
16 chunks, more than 64 and more than 1024 streams, history 1 and 8 and full poses, the evaluator over more than 256 and
512 frames, the augmentation with more boxes than selection threads, the GT sampler over more than 256 frames, Soft-NMS
ranking more than 256 rows under its pre cap and rotated NMS with more than 4096 entering boxes -- each bit for bit
against the stage's host restatement (augmentation: as test_gpu_augment.py compares with it, exact decisions and 1 ulp on
coordinates, since the device's sin / cos are not numpy's; the evaluator's similarity sum: its sim_tol; rotated NMS: the
keep list its construction dictates)."""
import numpy as np
import pytest

from conftest import load_golden

import trip_cases as tc
from test_eval_stats_host import fixture_frames
from test_gpu_augment import _near_face, _within_ulp
from test_gpu_eval_stats import _pack, _thresholds, match_indices, sim_tol
from test_gpu_sweeps import _same
from test_kitti_eval import ORACLE_FNS, _annos

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------ frustum crop
@pytest.fixture(scope="module", params=[3, 4], ids=["F3", "F4"])
def crop_engine(request, pp, hip_lib):
    eng = pp.Engine(tc.config(tc.CROP_MAX_BATCH, request.param), max_batch=tc.CROP_MAX_BATCH, max_points_per_frame=tc.CROP_NMAX)
    assert eng.d.num_point_features == request.param
    yield eng
    eng.close()


def _crop_equals(eng, frames, planes, want, back, tag):
    eng.upload(frames)
    kept, pts = eng.crop_to_image(planes, back=back, return_points=True)
    assert kept.dtype == np.int32 and kept.tolist() == [len(w) for w in want], (tag, kept.tolist())
    assert eng._offsets.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist(), tag
    assert np.array_equal(eng.crop_info(), kept), tag
    for b, (p, w) in enumerate(zip(pts, want)):
        assert p.dtype == np.float32 and p.shape == w.shape and p.tobytes() == w.tobytes(), (tag, b)
    return kept, pts


@pytest.mark.parametrize("back", [False, True], ids=["front", "back"])
@pytest.mark.parametrize("B", [17, 33])
def test_crop_past_sixteen_frames_and_one_round_of_chunks(crop_engine, B, back):
    frames, planes, want = tc.crop_case(B, crop_engine.d.num_point_features, back)
    first = _crop_equals(crop_engine, frames, planes, want, back, "first")
    # the same engine, the frames in another order: short frames where the long ones were (stale chunk tables would show)
    perm = tc.crop_permutation(B)
    _crop_equals(crop_engine, [frames[i] for i in perm], planes, [want[i] for i in perm], back, "permuted")
    again = _crop_equals(crop_engine, frames, planes, want, back, "again")
    assert np.array_equal(again[0], first[0]) and all(a.tobytes() == b.tobytes() for a, b in zip(again[1], first[1]))


# ------------------------------------------------------------------------------------------------ sweep accumulation
def _sweep_engine(pp, B, F, nmax, cfg):
    eng = pp.Engine(tc.config(B, F), max_batch=B, max_points_per_frame=nmax)
    eng.set_sweeps(cfg)
    return eng


def _sweeps_equal(pp, eng, cfg, calls, F, nmax, streams, feed=None):
    ref = pp.sweeps.SweepAccumulator(cfg, streams, F, nmax)
    assert eng.sweeps().to_dict() == ref.cfg.to_dict()
    infos = []
    for i, (frames, poses, stamps) in enumerate(calls):
        want, winfo = ref.accumulate(frames, poses, stamps)
        (feed or eng.upload)(frames)
        counts, pts = eng.accumulate_sweeps(poses, stamps, return_points=True)
        _same(pts, counts, eng.sweeps_info(), want, winfo, i)
        infos.append(winfo)
    return infos


@pytest.mark.parametrize("F,dec,cap,tf", tc.LONG_SETUPS)
def test_sweep_segments_past_sixteen_chunks(pp, hip_lib, F, dec, cap, tf):
    cfg = tc.long_cfg(dec, cap, tf)
    eng = _sweep_engine(pp, 2, F, tc.LONG_NMAX, cfg)
    infos = _sweeps_equal(pp, eng, cfg, tc.long_calls(F), F, tc.LONG_NMAX, 2)
    if dec == 1:
        assert infos[3]["truncated"].tolist() == [4, 0]
    else:
        assert infos[3]["push_truncated"][0] > 0
    eng.close()


def test_sweep_segments_past_sixteen_chunks_ingested(pp, hip_lib):
    """The long-segment sequence through ingest_pointcloud2: the frames' sizes are device values and the move grid is the
    host's bound, as in test_gpu_sweeps.py's test_ingested_frames_sizes_on_the_device_only."""
    from pp_amd import ingest
    F, dec, cap, tf = tc.LONG_SETUPS[0]
    cfg = tc.long_cfg(dec, cap, tf)
    eng = _sweep_engine(pp, 2, F, tc.LONG_NMAX, cfg)
    fields = [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1), ("intensity", 12, 7, 1)]
    mount = ingest.Mount(np.eye(3), np.eye(3), 0.0)

    def feed(frames):
        msgs = [(f.tobytes(), f.shape[0], 1, 4 * F, 4 * F * f.shape[0], fields) for f in frames]
        eng.ingest_pointcloud2(msgs, first=0, decimate=1, features=[ingest.FeatureField("intensity")], mount=mount)
        assert eng._offsets is None                                    # nothing on the host knows the sizes

    infos = _sweeps_equal(pp, eng, cfg, tc.long_calls(F), F, tc.LONG_NMAX, 2, feed)
    assert infos[3]["truncated"].tolist() == [4, 0]
    eng.close()


@pytest.mark.parametrize("B", [65, 129])
def test_sweep_offsets_past_sixty_four_streams(pp, hip_lib, B):
    eng = _sweep_engine(pp, B, 3, tc.MANY_NMAX, tc.MANY_CFG)
    infos = _sweeps_equal(pp, eng, tc.MANY_CFG, tc.many_calls(B), 3, tc.MANY_NMAX, B)
    assert infos[2]["used"].tolist() == [1] * B
    eng.close()


@pytest.mark.parametrize("history", [1, 8])
def test_sweep_history_limits(pp, hip_lib, history):
    cfg = tc.limit_cfg(history)
    eng = _sweep_engine(pp, tc.LIMIT_STREAMS, 4, tc.LIMIT_NMAX, cfg)
    infos = _sweeps_equal(pp, eng, cfg, tc.limit_calls(history), 4, tc.LIMIT_NMAX, tc.LIMIT_STREAMS)
    late = np.array([i["used"] for i in infos[history + 1:]])
    assert (late == history).any()
    if history > 1:
        assert ((late > 0) & (late < history)).any()
    else:
        assert (late == 0).any()                                       # (no integer lies strictly between 0 and 1)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- evaluator
@pytest.fixture(scope="module")
def golden():
    g = load_golden("ref_eval_stats.npz")
    return g, fixture_frames(g)


@pytest.mark.parametrize("reps", [8, 14], ids=["320", "560"])
def test_pr_and_match_over_the_repeated_reference_fixture(pp, hip_lib, golden, reps):
    """ref_eval_stats.npz's 40 frames, repeated: the expectation is the sum of the fixture's per-frame `stats`."""
    g, fr = golden
    ke = pp.kitti_eval
    idx = tc.long_order(len(fr["gt"]), reps)
    packed = _pack(ke, fr, idx)
    assert packed["nframes"] == len(idx) > 256
    th, nt = _thresholds(g)
    T = int(nt[0])
    per_frame = [[match_indices(fr["overlaps"][f], fr["dt"][f][:, 5], fr["ign_gt"][f], fr["ign_dt"][f], mo)
                  for f in range(len(fr["gt"]))] for mo in g["min_overlaps"]]
    m = ke.match_frames_gpu(packed, g["min_overlaps"])
    for k in range(len(g["min_overlaps"])):
        assert m[k].tolist() == [j for f in idx for j in per_frame[k][f]], k
    assert np.array_equal(m, ke.match_frames_gpu(packed, g["min_overlaps"]))
    for c, (metric, aos) in enumerate(zip(g["case_metric"], g["case_aos"])):
        stats = g["stats"][c].copy()                                   # [frame, tier, threshold, 4]
        stats[..., 3] = np.where(stats[..., 3] == -1, 0.0, stats[..., 3])
        want = stats[idx].sum(0)
        pr = ke.pr_frames_gpu(packed, g["min_overlaps"], th, nt, int(metric), bool(aos))
        assert np.array_equal(pr[:, :T, :3], want[..., :3]) and not pr[:, T:].any(), c
        err = np.abs(pr[:, :T, 3] - want[..., 3])
        print(f"case {c}, {len(idx)} frames: similarity |delta| max {err.max():.3e}, bound min {sim_tol(want[..., 0]).min():.3e}")
        assert (err <= sim_tol(want[..., 0])).all(), c
        again = ke.pr_frames_gpu(packed, g["min_overlaps"], th, nt, int(metric), bool(aos))
        assert again.tobytes() == pr.tobytes(), c


@pytest.fixture(scope="module")
def kitti():
    g = load_golden("ref_kitti_eval.npz")
    return _annos(g)


@pytest.mark.parametrize("reps", [5, 10], ids=["285", "570"])
@pytest.mark.parametrize("metric", [0, 1])
def test_pr_and_match_over_the_repeated_kitti_frames(pp, hip_lib, kitti, metric, reps):
    """ref_kitti_eval.npz's 57 frames, repeated: the expectation is the host loop over `compute_statistics`, run once per
    distinct frame and summed over the list -- never a GPU call."""
    gts, dts = kitti
    ke = pp.kitti_eval
    idx = tc.long_order(len(gts), reps)
    assert len(idx) == 57 * reps
    overlaps, _, _, _ = ke.calculate_iou_partly(dts, gts, metric, overlap_fns=ORACLE_FNS)
    tiers = ke.official_min_overlaps()[[0, 1, 3], metric, 1]
    gt_list, dt_list, ign_gt, ign_dt, dcs, total_valid = ke._prepare_data(gts, dts, 1, 2)
    pick = lambda lst: [lst[i] for i in idx]  # noqa: E731
    packed = ke.pack_frames(pick(overlaps), pick(gt_list), pick(dt_list), pick(ign_gt), pick(ign_dt), pick(dcs))
    assert packed["nframes"] == len(idx)
    frame_args = [(overlaps[i], gt_list[i], dt_list[i], ign_gt[i], ign_dt[i], dcs[i]) for i in range(len(gts))]
    m = ke.match_frames_gpu(packed, tiers)
    th, nt = np.zeros((3, 41)), np.zeros(3, dtype=np.int32)
    for k, mo in enumerate(tiers):
        scores = [ke.compute_statistics(*a, metric, mo, 0.0, False)[4].tolist() for a in frame_args]
        want = [match_indices(a[0], a[2][:, 5], a[3], a[4], mo) for a in frame_args]
        assert m[k].tolist() == [j for f in idx for j in want[f]], k
        host_scores = [s for f in idx for s in scores[f]]
        assert ke.matched_scores(packed, m[k]).tolist() == host_scores, k
        t = ke.get_thresholds(np.array(host_scores), total_valid * reps)
        nt[k] = len(t)
        th[k, :len(t)] = t
    assert nt.max() > 5
    assert np.array_equal(m, ke.match_frames_gpu(packed, tiers))
    pr = ke.pr_frames_gpu(packed, tiers, th, nt, metric, True)
    for k, mo in enumerate(tiers):
        per = np.zeros((len(gts), 41, 4))
        for i, a in enumerate(frame_args):
            for t in range(nt[k]):
                tp, fp, fn, sim, _ = ke.compute_statistics(*a, metric, mo, th[k, t], True, True)
                per[i, t] = (tp, fp, fn, sim if sim != -1 else 0.0)
        want = per[idx].sum(0)
        assert np.array_equal(pr[k, :, :3], want[:, :3]), k
        err = np.abs(pr[k, :, 3] - want[:, 3])
        print(f"metric {metric}, tier {k}, {len(idx)} frames: similarity |delta| max {err.max():.3e}")
        assert (err <= sim_tol(want[:, 0])).all(), k
    assert pr[..., 3].any()
    assert ke.pr_frames_gpu(packed, tiers, th, nt, metric, True).tobytes() == pr.tobytes()


def _on_equal_bytes(fn):
    """fn, evaluated once per distinct argument bytes: the host evaluator calls compute_statistics again for every
    repetition of a frame, with arrays of the same content."""
    by_id, canon, results = {}, {}, {}

    def content(a):
        if not isinstance(a, np.ndarray):
            return a
        hit = by_id.get(id(a))
        if hit is None or hit[0] is not a:
            raw = (a.dtype.str, a.shape, a.tobytes())
            hit = by_id[id(a)] = (a, canon.setdefault(raw, len(canon)))
        return hit[1]

    def cached(*args):
        key = tuple(content(a) for a in args)
        if key not in results:
            results[key] = fn(*args)
        return results[key]

    return cached


def test_reports_over_285_frames_equal_the_host_path(pp, hip_lib, kitti, monkeypatch):
    gts, dts = kitti
    ke = pp.kitti_eval
    idx = tc.long_order(len(gts), 5)
    G, D = [gts[i] for i in idx], [dts[i] for i in idx]
    assert len(G) == 285
    gpu = ke.get_official_eval_result(G, D, ["Pedestrian"], compute_bbox=False, statistics="gpu", overlap_fns=ORACLE_FNS)
    monkeypatch.setattr(ke, "compute_statistics", _on_equal_bytes(ke.compute_statistics))
    host = ke.get_official_eval_result(G, D, ["Pedestrian"], compute_bbox=False, overlap_fns=ORACLE_FNS)
    assert gpu[0] == host[0] and gpu[1] is None and host[1] is None
    assert gpu[2].tobytes() == host[2].tobytes() and gpu[3].tobytes() == host[3].tobytes()     # bev, 3d: counts alone
    np.testing.assert_allclose(gpu[4], host[4], rtol=0, atol=1e-9)                               # aos
    assert gpu[2].any() and gpu[4].any()


# ------------------------------------------------------------------------------------------------------ augmentation
@pytest.mark.parametrize("name", ["over", "exact"])
def test_augment_with_more_boxes_than_selection_threads(pp, hip_lib, name):
    frames, gts, valids = tc.augment_case(name)
    B = len(frames)
    cfg = pp.config.pedestrian_d435i_config(B)
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=tc.AUG_NMAX)
    acfg = tc.augment_config()
    draws = tc.augment_draws(gts, acfg)
    ref = tc.augment_reference(frames, gts, valids, draws, acfg, eng.d.pc_range)
    eng.upload(frames)
    got = eng.augment(gts, None, valids, draws, acfg)
    sel = eng.augment_selected()
    assert sel.tolist() == [int(s) for r in ref for s in r[3]["selected"]]
    for b, ((gp, gb, gc), (pts, bx, cl, info)) in enumerate(zip(got, ref)):
        assert _near_face(pp, frames[b], gts[b]) == 0
        assert len(gb) == len(bx) == int(info["keep"].sum()), (b, len(gb), len(bx))    # the keep flags: the same boxes stay
        _within_ulp(gb, bx)
        np.testing.assert_array_equal(gc, cl)
        assert gp.shape == pts.shape and gp[:, 3:].tobytes() == pts[:, 3:].tobytes()
        _within_ulp(gp, pts)
        assert (info["owner"] >= 0).sum() >= 2 * int(valids[b].sum())                  # every valid box moves its points
    eng.upload(frames)
    again = eng.augment(gts, None, valids, draws, acfg)
    for a, g in zip(again, got):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, g))
    assert np.array_equal(eng.augment_selected(), sel)
    eng.close()


# ---------------------------------------------------------------------------------------------- the two standalone NMS
def test_rotate_nms_removed_set_past_the_first_word(pp, hip_lib):
    """More than 4096 boxes enter: a lane of k_rnms_sweep holds a second, third and fourth word of the removed set."""
    dets, want = tc.rotate_nms_case()
    assert len(dets) <= pp.rotate_nms.MAX_BOXES
    got = pp.rotate_nms.rotate_nms(dets, 0.5)
    assert got.dtype == np.int64 and np.array_equal(got, want), np.setxor1d(got, want)
    assert got.tobytes() == pp.rotate_nms.rotate_nms(dets, 0.5).tobytes()
    capped = pp.rotate_nms.rotate_nms(dets, 0.5, post_max_size=8196)           # the walk stops inside the third word
    assert np.array_equal(capped, want[:8196])


def test_soft_nms_pre_cap_ranks_past_256_rows(pp, hip_lib):
    """k_snms_enter ranks every row against all rows, 256 at a time, when the pre cap binds."""
    sn = pp.soft_nms
    dets, _ = tc.soft_nms_case()
    rkeep, rscores = sn.soft_nms_np(dets, "hard", pre_max_size=tc.SNMS_PRE, **tc.SNMS_PARAMS)
    keep, scores = sn.soft_nms(dets, "hard", pre_max_size=tc.SNMS_PRE, **tc.SNMS_PARAMS)
    assert np.array_equal(keep, rkeep) and np.array_equal(scores, rscores)
    again = sn.soft_nms(dets, "hard", pre_max_size=tc.SNMS_PRE, **tc.SNMS_PARAMS)
    assert keep.tobytes() == again[0].tobytes() and scores.tobytes() == again[1].tobytes()


# ------------------------------------------------------------------------- loops over the batch, one thread per frame
def test_sweep_plan_past_1024_streams(pp, hip_lib):
    """k_sweep_plan's thread-per-frame loops take a second trip at the 1025th stream."""
    B = 1025
    eng = _sweep_engine(pp, B, 3, tc.MANY_NMAX, tc.MANY_CFG)
    infos = _sweeps_equal(pp, eng, tc.MANY_CFG, tc.many_calls(B), 3, tc.MANY_NMAX, B)
    assert infos[2]["used"].tolist() == [1] * B and infos[2]["count"][1024] > 0
    eng.close()


def test_gt_sample_decides_past_256_frames(pp, hip_lib):
    """k_gts_decide's thread-per-frame loop takes a second trip at the 257th frame; the comparison is
    test_gpu_gt_sample.py's: decisions equal, clouds bit-identical."""
    import random

    from test_gpu_gt_sample import _compare, _ped_db, _random_batch
    gts = pp.gt_sampler
    B = 257
    db = _ped_db(pp)
    eng = pp.Engine(tc.config(B), max_batch=B, max_points_per_frame=2048)
    eng.load_gt_database(db)
    rng = np.random.default_rng(31)
    frames, gt, classes, valids = _random_batch(pp, rng, db, B, 3, 300, (0.05, 6.35, -2.5, 2.5))
    cand = gts.draw_candidates(db, classes, random.Random(31))
    got, tap = _compare(pp, eng, db, frames, gt, classes, valids, cand, db.config)
    assert (tap["status"][256] == gts.ACCEPTED).any() and len(got[256][0]) > len(frames[256])
    eng.close()
