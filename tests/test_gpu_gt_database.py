"""The object-database build on the GPU (csrc/gt_database.hip): pp_gtdb_build / pp_gtdb_count against the reference
fixture and the float64 host restatement (gt_database.build_objects_np) -- counts equal, points bit-identical, order
included --, run-to-run identity over the feeds, the streamed dataset build, the database it makes for the sampler, the
frames left as they were, and argument refusal."""
import random

import numpy as np
import pytest

from test_gt_database_host import check_database, fixture_dataset

pytestmark = pytest.mark.gpu


def _near_face(pp, pts, boxes):
    """Points within 1e-9 m of a face of any box (test_gpu_gt_sample._near_face)."""
    if len(boxes) == 0 or len(pts) == 0:
        return 0
    near = 0
    n, d = pp.augment.box_planes(np.asarray(boxes, np.float64))
    norm = np.linalg.norm(n, axis=-1)[None]
    slab = max(64, 1000000 // len(boxes))
    for s in range(0, len(pts), slab):
        sg = pp.augment.face_sign(np.asarray(pts[s:s + slab], np.float64)[:, :3], n, d)
        near += int(((np.abs(sg) / norm).min(axis=(1, 2)) < 1e-9).sum())
    return near


def random_batch(seed, B, F, n_max, span):
    """B frames of up to n_max points over span (x0, x1, y0, y1) with 0-256 lidar boxes each: frame 0 has no points,
    frame 1 no boxes, frame 2 a full-size cloud and 256 boxes; boxes of pedestrian to van size, free to overlap; some far
    outside the cloud (no points)."""
    rng = np.random.default_rng(seed)
    frames, boxes = [], []
    for b in range(B):
        n = 0 if b == 0 else n_max if b == 2 else int(rng.integers(1, n_max + 1))
        p = np.stack([rng.uniform(span[0], span[1], n), rng.uniform(span[2], span[3], n), rng.uniform(-1.4, 1.4, n)] +
                     [rng.uniform(0, 1, n) for _ in range(F - 3)], 1).astype(np.float32)
        g = 0 if b == 1 else 256 if b == 2 else int(rng.choice([1, 3, 17, 64, 65, 130, 256]))
        bx = np.stack([rng.uniform(span[0] - 1.0, span[1] + 1.0, g), rng.uniform(span[2] - 1.0, span[3] + 1.0, g),
                       rng.uniform(-1.2, 0.2, g), rng.uniform(0.4, 2.2, g), rng.uniform(0.4, 4.5, g), rng.uniform(0.8, 2.2, g),
                       rng.uniform(-3.2, 3.2, g)], 1)
        frames.append(p)
        boxes.append(bx)
    return frames, boxes


def _compare(pp, eng, frames, boxes):
    """One batch against the host restatement; nothing is excluded.  Returns (points cut out, near-face points)."""
    gdb = pp.gt_database
    eng.upload(frames)
    counts, objs = eng.build_gt_objects(boxes, return_counts=True)
    only = eng.count_points_in_gt(boxes)
    total = near = 0
    for b, (p, bx) in enumerate(zip(frames, boxes)):
        want_c, want_o = gdb.build_objects_np(p, bx)
        near += _near_face(pp, p, bx)
        assert counts[b].dtype == np.int32 and np.array_equal(counts[b], want_c), b
        assert np.array_equal(only[b], want_c), b
        assert len(objs[b]) == len(want_o)
        for i, (g, w) in enumerate(zip(objs[b], want_o)):
            assert g.dtype == np.float32 and g.shape == w.shape and g.tobytes() == w.tobytes(), (b, i)
        total += int(want_c.sum())
    print(f"near-face points (< 1e-9 m): {near}; points cut out: {total}")
    assert near == 0
    return total, counts


def test_fixture_frames_equal_reference(pp, hip_lib):
    gdb = pp.gt_database
    G, infos, clouds = fixture_dataset()
    B = len(clouds)
    eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=4096)
    lidar = [G[f"f{k}__rbbox_lidar"] for k in range(B)]
    eng.upload(clouds)
    counts = eng.count_points_in_gt(lidar)
    objs = eng.build_gt_objects(lidar)
    for k in range(B):
        assert np.array_equal(counts[k], G[f"f{k}__num_points_in_gt"][:len(lidar[k])])
        assert [len(o) for o in objs[k]] == counts[k].tolist()
    db_infos, db_points = gdb.create_groundtruth_database(eng, infos, clouds, used_classes=list(G["used_classes"]))
    assert check_database(G, db_infos, db_points) == 29                      # the reference's files, bit for bit
    gdb.calculate_num_points_in_gt(eng, infos, clouds)
    for k, info in enumerate(infos):
        got = info["annos"]["num_points_in_gt"]
        assert got.dtype == np.int32 and np.array_equal(got, G[f"f{k}__num_points_in_gt"])
    eng.close()


@pytest.mark.parametrize("seed", [61, 62])
def test_random_batches_cfg_a(pp, hip_lib, seed):
    B = 32
    eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=8192)
    frames, boxes = random_batch(seed, B, 3, 8192, (0.05, 6.35, -2.5, 2.5))
    total, counts = _compare(pp, eng, frames, boxes)
    assert total > sum(len(f) for f in frames)                                # points shared between boxes
    assert any((c == 0).any() for c in counts) and max(len(c) for c in counts) == 256
    eng.close()


def test_random_batch_cfg_k_four_features(pp, hip_lib):
    B = 8
    cfg = pp.config.kitti_shaped_config(B)
    assert pp.config.Derived(cfg).num_point_features == 4
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=32768)
    frames, boxes = random_batch(63, B, 4, 32768, (0.05, 40.0, -20.0, 20.0))
    boxes[2][:, 3:6] *= 4.0                                                   # objects of thousands of points
    total, counts = _compare(pp, eng, frames, boxes)
    assert max(int(c.max()) for c in counts if len(c)) > 1000
    eng.close()


def test_runs_and_feeds_identical(pp, hip_lib):
    B = 4
    eng = pp.Engine(pp.config.pedestrian_d435i_config(8), max_batch=8, max_points_per_frame=8192)
    frames, boxes = random_batch(64, B, 3, 6000, (0.05, 6.35, -2.5, 2.5))

    def flat(res):
        counts, objs = res
        return [c.tobytes() for c in counts] + [o.tobytes() for f in objs for o in f]

    eng.upload(frames)
    first = flat(eng.build_gt_objects(boxes, return_counts=True))
    assert flat(eng.build_gt_objects(boxes, return_counts=True)) == first        # the same resident frames again
    eng.upload(frames)
    assert flat(eng.build_gt_objects(boxes, return_counts=True)) == first
    st = eng.staging(frames)                                                      # zero-copy (<= 4 frames)
    eng.upload_async(st)
    assert flat(eng.build_gt_objects(boxes, return_counts=True)) == first
    frames8, boxes8 = frames + frames, boxes + boxes                              # the copy engine's feed
    st8 = eng.staging(frames8)
    eng.upload_async(st8)
    assert flat(eng.build_gt_objects(boxes8, return_counts=True)) == [c for c in first[:B]] * 2 + first[B:] * 2
    eng.close()


def test_streamed_dataset_build_with_partial_last_batch(pp, hip_lib):
    gdb = pp.gt_database
    G, infos, clouds = fixture_dataset()
    eng = pp.Engine(pp.config.pedestrian_d435i_config(5), max_batch=5, max_points_per_frame=4096)     # 12 frames: 5 + 5 + 2
    db_infos, db_points = gdb.create_groundtruth_database(eng, infos, iter(clouds), used_classes=list(G["used_classes"]))
    assert check_database(G, db_infos, db_points) == 29
    host_infos, host_points = gdb.create_groundtruth_database(None, infos, clouds, used_classes=list(G["used_classes"]))
    for name in host_infos:
        assert [o["path"] for o in db_infos[name]] == [o["path"] for o in host_infos[name]]
        assert [p.tobytes() for p in db_points[name]] == [p.tobytes() for p in host_points[name]]
    with pytest.raises(ValueError, match="float32"):
        gdb.create_groundtruth_database(eng, infos, [c.astype(np.float64) for c in clouds])
    eng.close()


def test_database_from_frames_feeds_the_sampler(pp, hip_lib, tmp_path):
    gdb, gts = pp.gt_database, pp.gt_sampler
    G, infos, clouds = fixture_dataset()
    B = 4
    cfg = pp.config.pedestrian_d435i_config(B)
    cfg["model"]["second"]["num_class"] = 2
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=8192)
    scfg = gts.SamplerConfig.from_input_reader({"sample_classes": ["Pedestrian", "Cyclist"], "sample_max_nums": [5, 3]})
    used = list(G["used_classes"])
    db = gts.GtDatabase.from_frames(eng, infos, clouds, scfg, np.random.RandomState(9), random.Random(9), 3, used_classes=used)
    db_infos, db_points = gdb.create_groundtruth_database(eng, infos, clouds, used_classes=used)
    pkl = gdb.write_reference_files(db_infos, db_points, tmp_path)
    db2 = gts.GtDatabase.from_reference_files(pkl, tmp_path, True, scfg, np.random.RandomState(9), random.Random(9), 3)
    assert len(db) == len(db2) > 10
    for key in ("boxes", "points", "offsets", "classes"):
        assert getattr(db, key).tobytes() == getattr(db2, key).tobytes(), key
    frames = [clouds[3], clouds[7], clouds[3][:900], clouds[7][:500]]         # frames without objects of their own
    gt = [np.zeros((0, 7), np.float32)] * B
    classes = [np.zeros(0, np.int32)] * B
    out = []
    for d in (db, db2):
        eng.load_gt_database(d)
        cand = gts.draw_candidates(d, classes, random.Random(4))
        eng.upload(frames)
        out.append(eng.gt_sample(gt, classes, None, cand))
    assert any(len(o[0]) > len(f) for o, f in zip(out[0], frames))            # something was pasted
    for a, b in zip(out[0], out[1]):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    eng.close()


def test_detect_after_a_build_sees_the_same_frames(pp, hip_lib):
    B = 4
    eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=8192)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    frames = [pp.synth.d435i_cloud(700 + i, 4096) for i in range(B)]
    _, boxes = random_batch(65, B, 3, 100, (0.05, 6.35, -2.5, 2.5))
    rect, trv, _ = pp.synth.default_calib()
    R, T = np.stack([rect] * B), np.stack([trv] * B)

    def run(build, feed):
        if feed == "copy":
            eng.upload(frames, R, T)
        else:
            eng.upload_async(eng.staging(frames))
            eng.set_calib(R, T, B)
        if build:
            assert sum(int(c.sum()) for c in eng.count_points_in_gt(boxes)) > 0
            eng.build_gt_objects(boxes)
        eng.detect_async()
        eng.sync()
        dets, n = eng.detections()
        kept = [np.asarray(dets[b][:int(n[b])]).tobytes() for b in range(B)]
        return kept, n.tobytes(), eng.intermediates()["n_pillars"].tobytes()

    for feed in ("copy", "zero-copy"):
        assert run(True, feed) == run(False, feed)
    eng.close()


def test_refusals_leave_the_handle_usable(pp, hip_lib):
    B = 2
    eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=4096)
    frames, boxes = random_batch(66, B, 3, 3000, (0.05, 6.35, -2.5, 2.5))
    boxes = [boxes[0][:0], np.array([[3.0, 0.0, -0.7, 2.0, 2.0, 2.0, 0.3], [3.2, 0.1, -0.7, 1.0, 1.0, 1.0, 0.0]])]
    eng.upload(frames)
    good = eng.build_gt_objects(boxes, return_counts=True)
    need = int(sum(c.sum() for c in good[0]))
    assert need > 1
    with pytest.raises(RuntimeError, match=f"PP_ERR_ARG.*holds {need - 1} points, {need} are written"):
        eng.build_gt_objects(boxes, capacity=need - 1)
    again = eng.build_gt_objects(boxes, return_counts=True, capacity=need)       # succeeds at the reported size
    assert [o.tobytes() for f in again[1] for o in f] == [o.tobytes() for f in good[1] for o in f]
    eng._gdb_cap = 0                                                             # ... and the engine's own retry finds it
    eng._offsets = np.zeros(B + 1, np.int64)
    assert [o.tobytes() for f in eng.build_gt_objects(boxes) for o in f] == [o.tobytes() for f in good[1] for o in f]
    for bad, what in (([boxes[0], boxes[1] * np.array([1, 1, 1, 1, 1, 1, np.nan])], "not finite"),
                      ([boxes[0], boxes[1] * np.array([1, 1, 1, 0, 1, 1, 1.0])], "size <= 0"),
                      ([boxes[0], np.repeat(boxes[1][:1], 257, 0)], r"257 boxes \(0\.\.256\)"),
                      ([boxes[1]], "frames are resident")):
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*" + what):
            eng.build_gt_objects(bad)
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*" + what):
            eng.count_points_in_gt(bad)
        assert [o.tobytes() for f in eng.build_gt_objects(boxes) for o in f] == [o.tobytes() for f in good[1] for o in f]
    # frames ingested from camera messages: their sizes are device values
    msg = pp.synth.pointcloud2_message(1, 64, 48)
    eng.ingest_pointcloud2([msg, msg])
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*ingested from camera messages"):
        eng.build_gt_objects(boxes)
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*ingested from camera messages"):
        eng.count_points_in_gt(boxes)
    eng.upload(frames)
    assert [o.tobytes() for f in eng.build_gt_objects(boxes) for o in f] == [o.tobytes() for f in good[1] for o in f]
    eng.close()

