"""Inputs that take the data-path stages past ONE trip of their scan, carry and strided loops, shared by
tests/test_trip_cases_host.py (which asserts, on the host restatements alone, that every input does what it is built for)
and tests/test_gpu_trips.py (which runs them on the GPU, bit for bit against the stage's restatement).

The audit behind them: every `for (x = tid | lane | wave; x < n; x += step)` loop and every round-with-carry loop of the
data-path kernels.  An entry reads: the loop | the size at which it takes a second trip | whether the C API admits that
size; under it, the test that reaches it.  T = tests/test_gpu_trips.py.  "refused": the size cannot pass the API's
argument checks, so there is nothing to test.

csrc/frustum_crop.hip
  k_crop_scan  b += 16 (a wave per frame) | batch > 16 | admitted
      T::test_crop_past_sixteen_frames_and_one_round_of_chunks (17 frames: two trips, 33: three)
  k_crop_scan  c0 += PP_WAVE, `carry` | a frame > 16 384 rows | admitted
      the same test (16 385, 32 767 and 32 768 rows; 16 384: exactly one trip)
  k_crop_count, k_crop_scatter: a chunk per wave, CROP_ITER fixed steps; `run` is carried inside a chunk only
csrc/sweeps.hip (k_sweep_plan; k_sweep_move is a chunk per workgroup and has no loop)
  b += PLAN_THREADS (counts; segments) | batch > 1024 | admitted (*)
      T::test_sweep_plan_past_1024_streams (1025)
  b0 += PP_WAVE, carries `off` and `c` | batch > 64 | admitted
      T::test_sweep_offsets_past_sixty_four_streams (65: two trips, 129: three)
  g += PLAN_THREADS / 16 (16 lanes per segment) | batch x (history + 2) > 64 | admitted
      the same test (195 and 387 segments)
  c += 16 (a lane per chunk of a segment) | a segment > 4096 rows | admitted
      T::test_sweep_segments_past_sixteen_chunks, T::..._ingested (33 chunks: three trips, 17: two)
  sweep_select  k < PP_SWEEP_MAX under the guard k < history | history 1 and 8 | admitted
      T::test_sweep_history_limits (at 8 the guard is always true and the ring has 9 slots)
csrc/ingest.hip, csrc/ingest_dev.h
  ing_scan_chunks  c0 += PP_WAVE, `carry` | a message > 32 768 records | admitted
      test_gpu_rig_ingest.py::test_chunk_and_scan_boundaries (260 x 128: 65 chunks);
      the plain path: test_gpu_ingest.py::test_vga_messages_at_max_batch (640 x 480: 600 chunks)
  ingest_scan_frames  b += 16 | batch > 16 | admitted
      test_gpu_depth_ingest.py::test_a_batch_of_18_one_chunk_frames
  k_rig_scan  s += 16 | sources > 16 | admitted
      test_gpu_rig_ingest.py::test_more_sources_than_the_scan_has_waves (3 frames x 6 sources)
csrc/eval_stats.hip
  k_es_reduce  f += 256 | frames > 256 | admitted
      T::test_pr_and_match_over_the_repeated_kitti_frames, T::..._reference_fixture (285, 320: two trips; 560, 570:
      three), T::test_reports_over_285_frames_equal_the_host_path
  k_es_match, k_es_count  c < nch (64 detections a round, a state bit per round) | detections > 64 | admitted (<= 1024)
      test_gpu_eval_stats.py::test_pr_against_reference_fixture (65 and 130), ::test_edges (1024)
csrc/augment.hip
  k_aug_select  g += kSelThreads (corners; box stages) | boxes of a frame > 128 | admitted (<= 256)
      T::test_augment_with_more_boxes_than_selection_threads (129 and 256; 128: exactly one trip)
  k_aug_select  a lane per try | num_try > 128 | refused (PP_AUG_MAX_TRY)
  k_aug_compact  g += 256 | boxes of a frame > 256 | refused (PP_MAX_GT_PER_FRAME)
csrc/gt_sample.hip
  k_gts_select  g += kSelThreads (256) | boxes of a frame > 256 | refused
  k_gts_select  t += kSelThreads (pairs) | candidates x (boxes + candidates) > 256 | admitted
      test_gpu_gt_sample.py::test_random_batches_cfg_a (a frame without boxes draws 4 rounds x 8 candidates: 1024 pairs;
      test_trip_cases_host.py checks that the batches hold such a frame)
  k_gts_decide  b += 256 | batch > 256 | admitted (*)
      T::test_gt_sample_decides_past_256_frames (257)
  k_gts_paste  t += 256 | boxes + accepted > 256 | refused (boxes + a round's candidates <= 256)
csrc/gt_database.hip
  k_gdb_members  t0 += kTile | boxes of a frame > 64 | admitted
  k_gdb_members  k += kChunk (staging a tile) | a tile of > 10 boxes | admitted
  k_gdb_chunks  c < nch, `run` | a frame > 256 points | admitted
  k_gdb_offsets  a run of boxes per thread | boxes of the batch > 256 | admitted
      all four: test_gpu_gt_database.py::test_random_batches_cfg_a (frame 2: 256 boxes on a full cloud)
csrc/targets.hip
  stage_boxes  g += blockDim.x (256) | boxes of a frame > 256 | refused
csrc/soft_nms.hip
  k_snms_enter  j0 += 256 | rows > 256 under a binding pre cap | admitted
      T::test_soft_nms_pre_cap_ranks_past_256_rows (600 rows, 300 enter); before it only the all-equal rows of
      test_gpu_soft_nms.py::test_caps_empty_input_and_refusals
  k_soft_nms  i += SNMS_T, SNMS_PER rows a thread | entering rows > 1024 | admitted (<= 4096)
      test_gpu_soft_nms.py::test_seeded_sets_equal_the_restatement[4096]
csrc/rotate_nms.hip
  k_rnms_rank  j0 += 256 | boxes > 256 | admitted
  k_rnms_mask  q += RNMS_TILE * RNMS_Q (staging) | a column tile > 28 boxes | admitted
      both: test_gpu_rotate_nms.py::test_thousand_boxes_equal_the_host_restatement
  k_rnms_sweep  a lane's removed-set words l, l + 64, ... | entering boxes > 4096 | admitted (<= 16 384)
      T::test_rotate_nms_removed_set_past_the_first_word (12 350 boxes: words 1, 2 and 3)
csrc/grad_clip.hip (k_grad_norm_finish; k_grad_sumsq takes PP_GNORM_CHUNK / 256 fixed steps)
  gi += 16 (a wave per group) | groups > 16 | admitted
  i += 64 (partial sums) | partial sums > 64 | admitted
  base += 64, gi += 64 (groups, 64 at a time) | groups > 64 | admitted
      all: test_gpu_grad_clip.py::test_trainer_frozen_norm_covers_the_trainable_tensors (a norm per tensor: 82 groups once
      set_trainable(True) has rebuilt them); the standalone table of that file has 70 segments in 10 groups

(*) max_batch is the only bound on the batch, so the API admits these sizes although no use of the project comes near them
(the benchmark's batch is 64); on tiny_config an engine that wide costs a fraction of a second, and the cases are here.
"""
import copy

import numpy as np

import pp_amd as pp

F32 = np.float32


def config(B, F=3):
    """tiny_config with F point features (the 4-feature variant is pc2_feature_cases.config4's)."""
    cfg = copy.deepcopy(pp.config.tiny_config(B))
    if F != 3:
        cfg["model"]["second"]["num_point_features"] = F
        for reader in ("eval_input_reader", "train_input_reader"):
            if reader in cfg:
                cfg[reader]["num_point_features"] = F
    return cfg


# ------------------------------------------------------------------------------------------------------ frustum crop
CROP_CHUNK, CROP_ROUND = 256, 64 * 256          # rows of a chunk; rows one round of k_crop_scan's 64 lanes covers
CROP_NMAX, CROP_MAX_BATCH = 32768, 33
CROP_SMALL = (0, 1, 255, 256, 257, 4096)
CROP_IMAGE_SHAPE = (375, 1242)
# frame -> rows, the frames the case is about; every other frame draws from CROP_SMALL
CROP_FIXED = {17: {0: 16385, 16: 257},
              33: {0: 16384, 8: 0, 16: 32768, 24: 0, 32: 32767}}
CROP_SEED = {17: 5, 33: 6}


def crop_planes(B):
    rect, trv2c, p2 = pp.synth.default_calib()
    return np.stack([pp.frustum.frustum_planes(rect, trv2c, p2, CROP_IMAGE_SHAPE)] * B)


def crop_sizes(B):
    rng = np.random.default_rng(100 + B)
    sizes = [int(CROP_FIXED[B].get(b, CROP_SMALL[int(rng.integers(len(CROP_SMALL)))])) for b in range(B)]
    return sizes


def crop_case(B, F, back):
    """(frames, planes [B, 6, 4], expected kept frames) of the B-frame case.  The clouds of the `back` run are the
    forward run's with column 0 negated: the restatement then keeps the same rows under either flag, so the conditions
    test_trip_cases_host.py asserts (a kept row on either side of chunk 64) hold for both."""
    rng = np.random.default_rng(CROP_SEED[B])
    frames = []
    for n in crop_sizes(B):
        f = np.stack([rng.uniform(-10, 70, n), rng.uniform(-30, 30, n), rng.uniform(-3, 2, n)], 1).astype(F32)
        if F > 3:
            f = np.concatenate([f, rng.random((n, F - 3), dtype=F32)], axis=1)
        if back:
            f[:, 0] = -f[:, 0]
        frames.append(np.ascontiguousarray(f))
    planes = crop_planes(B)
    want = [pp.frustum.crop_np(f, planes[b], back=back) for b, f in enumerate(frames)]
    return frames, planes, want


def crop_permutation(B):
    """The order of the second call: the frames reversed and turned by 5, so that small frames land on the slots whose
    chunk tables the long frames of the first call filled."""
    return [(B - 1 - b + 5) % B for b in range(B)]


# ------------------------------------------------------------------------------------------------ sweep accumulation
SWEEP_CHUNK = 256


def full_pose(rng, call, stream):
    """A pose as an odometry frame far from its origin gives it: roll, pitch and yaw all non-zero, a translation of the
    order of 1e3 m that moves about a metre per call; through sweeps.pose_from_matrix."""
    roll = 0.05 + 0.004 * call + 0.002 * stream + abs(rng.normal()) * 0.005
    pitch = -0.08 - 0.004 * call - 0.002 * stream - abs(rng.normal()) * 0.005
    yaw = 0.3 + (0.2 * call + 0.37 * stream) % 2.5 + rng.normal() * 0.02
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = [1234.5 + 1.1 * call + 3.0 * stream + rng.normal() * 0.1, -2345.25 + 0.7 * call + rng.normal() * 0.1,
                87.125 + 0.05 * call + rng.normal() * 0.02]
    return pp.sweeps.pose_from_matrix(T)


def pose_angles(P):
    """(roll, pitch, yaw) of a [3, 4] pose built as Rz Ry Rx."""
    R = P[:, :3]
    return np.arctan2(R[2, 1], R[2, 2]), -np.arcsin(R[2, 0]), np.arctan2(R[1, 0], R[0, 0])


STAMP0 = 1.7e9


def _sweep_frame(rng, n, F):
    f = rng.uniform([-40.0, -40.0, -2.0], [40.0, 40.0, 3.0], size=(n, 3)).astype(F32)
    if F > 3:
        f = np.concatenate([f, rng.random((n, F - 3), dtype=F32)], axis=1)
    return np.ascontiguousarray(f)


def sweep_calls(sizes, F, stamps, seed):
    """[(frames, poses [B, 3, 4], stamps [B])]: sizes[call][stream] rows, stamps[call][stream] seconds after STAMP0."""
    rng = np.random.default_rng(seed)
    calls = []
    for i, row in enumerate(sizes):
        frames = [_sweep_frame(rng, n, F) for n in row]
        poses = np.stack([full_pose(rng, i, b) for b in range(len(row))])
        calls.append((frames, poses, STAMP0 + np.asarray(stamps[i], np.float64)))
    return calls


# long segments: 8193 rows are 33 chunks (k_sweep_plan's 16 lanes take three trips), 4097 rows are 17 (two)
LONG_NMAX, LONG_ROWS, LONG_CALLS = 32768, (8193, 4097), 4
# (point features, history_decimate, capacity, time_feature)
LONG_SETUPS = [(4, 1, 9000, 3), (3, 1, 9000, -1), (4, 3, 2000, 3)]


def long_cfg(dec, cap, tf):
    return {"history": 8, "capacity": cap, "history_decimate": dec, "max_age": 1000.0, "time_feature": tf}


def long_calls(F):
    return sweep_calls([LONG_ROWS] * LONG_CALLS, F, [[0.1 * i + b for b in range(2)] for i in range(LONG_CALLS)], 21)


# many streams: the offset scan of k_sweep_plan walks the batch 64 frames at a time
MANY_NMAX, MANY_CALLS = 64, 3
MANY_CFG = {"history": 1, "capacity": 8, "history_decimate": 1, "max_age": 1000.0, "time_feature": -1}


def many_calls(B):
    sizes = [[(b + i) % 4 for b in range(B)] for i in range(MANY_CALLS)]
    return sweep_calls(sizes, 3, [[0.1 * i + 0.001 * b for b in range(B)] for i in range(MANY_CALLS)], 22 + B)


# history limits: three streams, tiny frames, the ring wraps; stream 0 steps 0.1 s (max_age 0.35 s: three sweeps are
# young enough), stream 1 steps 0.01 s (every stored sweep is), stream 2 steps 0.1 s and pauses before two of the calls
LIMIT_NMAX, LIMIT_STREAMS, LIMIT_MAX_AGE = 64, 3, 0.35


def limit_cfg(history):
    return {"history": history, "capacity": 4, "history_decimate": 1, "max_age": LIMIT_MAX_AGE, "time_feature": 3}


def limit_calls(history):
    n = history + 3
    sizes = [[(2 * i + 3 * b) % 6 for b in range(LIMIT_STREAMS)] for i in range(n)]
    pause = np.cumsum([0.5 if i in (n - 3, n - 1) else 0.0 for i in range(n)])
    return sweep_calls(sizes, 4, [[0.1 * i, 0.01 * i, 0.1 * i + pause[i]] for i in range(n)], 23 + history)


def run_restatement(cfg, calls, F, nmax):
    """[(output frames, info)] of the calls through a fresh sweeps.SweepAccumulator."""
    return pp.sweeps.accumulate_np(cfg, calls, F, nmax)


# ---------------------------------------------------------------------------------------------------------- evaluator
def long_order(n, reps):
    """Indices into a list of n frames, `reps` repetitions, each turned by another amount: the first turn, counted up
    from 11 r, that no earlier repetition has and that leaves the frames 256 and 512 positions apart different (thread i of
    k_es_reduce adds frames i, i + 256, i + 512)."""
    idx, turns = np.zeros(0, np.int64), []
    for r in range(reps):
        for s in range(11 * r, 11 * r + n):
            rep = np.roll(np.arange(n), -(s % n))
            cand = np.concatenate([idx, rep])
            ok = s % n not in turns or len(turns) >= n
            for gap in (256, 512):
                if len(cand) > gap:
                    ok = ok and (cand[gap:] != cand[:-gap])[max(len(idx) - gap, 0):].all()
            if ok:
                break
        else:
            raise ValueError(f"long_order({n}, {reps}): no turn for repetition {r}")
        idx = cand
        turns.append(s % n)
    return idx


# ------------------------------------------------------------------------------------------------------ augmentation
AUG_SEL_THREADS = 128                    # kSelThreads of csrc/augment.hip and csrc/gt_sample.hip
AUG_COUNTS = {"over": [129, 256], "exact": [128]}
AUG_NMAX = 4096


def _grid_boxes(rng, G):
    """G small boxes on a 16 x 16 grid inside cfg-A's range, 0.36 m x 0.3 m apart, in a shuffled order; the last four
    are two pairs of twins: the same centre, the yaws 45 degrees apart, so that every try of either still crosses the
    other's edges and neither finds a place (selected -1)."""
    cells = rng.permutation(256)[:G]
    gx, gy = cells // 16, cells % 16
    g = np.stack([0.45 + 0.36 * gx + rng.uniform(-0.02, 0.02, G), -2.25 + 0.3 * gy + rng.uniform(-0.02, 0.02, G),
                  rng.uniform(-1.0, -0.6, G), rng.uniform(0.05, 0.08, G), rng.uniform(0.05, 0.08, G),
                  rng.uniform(0.3, 0.5, G), rng.uniform(-np.pi, np.pi, G)], 1)
    for a in (G - 4, G - 2):
        g[a, 3:5] = g[a + 1, 3:5] = (1.2, 1.3)
        g[a + 1, :3] = g[a, :3]
        g[a + 1, 6] = g[a, 6] + np.pi / 4
    return g.astype(F32)


def augment_case(name):
    """(frames, gt boxes, valid flags) of a batch with AUG_COUNTS[name] boxes per frame.  Every box holds two points; the
    frames are d435i clouds besides."""
    rng = np.random.default_rng(31 + len(name))
    frames, gts, valids = [], [], []
    for b, G in enumerate(AUG_COUNTS[name]):
        g = _grid_boxes(rng, G)
        inside = np.repeat(g[:, :3], 2, axis=0).astype(np.float64)
        inside[:, 2] += np.tile([0.1, 0.2], G)
        inside[:, :2] += rng.uniform(-0.01, 0.01, (2 * G, 2))
        frames.append(np.ascontiguousarray(np.concatenate([pp.synth.d435i_cloud(900 + b, 2000), inside.astype(F32)])))
        gts.append(g)
        v = rng.uniform(size=G) < 0.9
        v[-4:] = True
        valids.append(v)
    return frames, gts, valids


def augment_config():
    return pp.augment.AugmentConfig.from_input_reader({})


def augment_draws(gts, cfg):
    """The draws test_gpu_augment.py's _check_batch makes."""
    return pp.augment.draw(np.random.RandomState(1), gts, cfg)


def augment_reference(frames, gts, valids, draws, cfg, pc_range):
    """Per frame augment_np's (points, boxes, classes, info)."""
    pc = np.asarray(pc_range, np.float64)
    return [pp.augment.augment_np(frames[b], gts[b], None, valids[b], draws.frame(b), cfg, pc, return_info=True)
            for b in range(len(frames))]


# ---------------------------------------------------------------------------------------------- the two standalone NMS
RNMS_N = 12350
# sorted position suppressed -> the position that suppresses it: the removed bits sit in words 1, 1, 2 and 3 of
# k_rnms_sweep's removed set (a lane holds the words l, l + 64, ... of 64 positions each)
RNMS_PAIRS = {4130: 4120, 4159: 10, 8200: 4200, 12300: 8300}


def rotate_nms_case():
    """(dets [RNMS_N, 6], expected keep): unit squares 5 apart on a line, scores falling with the index, so sorted
    position = index; the boxes of RNMS_PAIRS lie on top of their suppressors.  The expectation is the construction's."""
    n = RNMS_N
    d = np.zeros((n, 6), F32)
    d[:, 0] = 5.0 * np.arange(n)
    d[:, 2:4] = 1.0
    d[:, 5] = 1.0 - np.arange(n) / n
    for gone, by in RNMS_PAIRS.items():
        d[gone, 0] = d[by, 0]
    return d, np.array([i for i in range(n) if i not in RNMS_PAIRS], np.int64)


SNMS_N, SNMS_PRE = 600, 300
SNMS_PARAMS = dict(sigma=0.5, iou_threshold=0.3, score_floor=0.001)


def soft_nms_case():
    """(dets [SNMS_N, 5], margins) for method "hard" under pre_max_size = SNMS_PRE: disjoint boxes on a grid and 200
    jittered copies of some, scores a permuted grid (no ties), drawn again until every decision of the restatement under
    the cap keeps test_gpu_soft_nms.py's margins."""
    rng = np.random.default_rng(7)
    n, copies = SNMS_N, 200
    for _ in range(200):
        m = n - copies
        side = int(np.ceil(np.sqrt(m)))
        cell = rng.permutation(side * side)[:m]
        xy = np.stack([cell % side, cell // side], axis=1) * 45.0 + rng.uniform(0, 4.0, (m, 2))
        b = np.concatenate([xy, xy + rng.uniform(10.0, 40.0, (m, 2))], axis=1)
        b = np.concatenate([b, b[rng.choice(m, copies, replace=False)] + rng.normal(0, 2.0, (copies, 4))])[rng.permutation(n)]
        dets = np.concatenate([b, ((rng.permutation(n) + 0.5) / n)[:, None]], axis=1).astype(F32)
        margins = pp.soft_nms.decision_margins(dets, "hard", pre_max_size=SNMS_PRE, **SNMS_PARAMS)
        if margins["gap"] > 1e-5 and margins["iou"] > 1e-4 and margins["floor"] > 1e-6:
            return dets, margins
    raise AssertionError("soft_nms_case: no draw with the margins")
