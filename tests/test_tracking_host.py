"""tracking.py, the host restatement of the per-stream tracking step (the GPU step is held to it bit for bit in
tests/test_gpu_tracking.py).  The reference has no tracker, so the restatement is held to independent formulations written
here (a generic 2x2 matrix Kalman filter, a sort-based greedy matching) and to hand-made cases."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T(pp):
    return pp.tracking


def _dets(pp, rows_per_stream, rows=None):
    """rows_per_stream: per stream a list of (x, y, z, score, label) -> (dets [S, rows], n [S])."""
    from pp_amd.engine import DET_DTYPE
    R = rows or max(1, max(len(r) for r in rows_per_stream))
    d = np.zeros((len(rows_per_stream), R), DET_DTYPE)
    n = np.zeros(len(rows_per_stream), np.int32)
    for s, rr in enumerate(rows_per_stream):
        n[s] = len(rr)
        for i, (x, y, z, sc, lb) in enumerate(rr):
            d["box3d_lidar"][s, i] = [x, y, z, 0.6, 0.8, 1.7, 0.25]
            d["score"][s, i] = sc
            d["label"][s, i] = lb
    return d, n


def _cfg(T, **kw):
    base = dict(gate=1.25, birth_score=0.3, max_misses=2, min_hits=2)
    base.update(kw)
    return T.TrackConfig(**base)


# ---- 1. independent formulation ----
def test_scalar_filter_equals_a_generic_matrix_filter(T):
    """predict / update on the three scalars against F P F' + Q, K = P H' (H P H' + R)^-1, (I - K H) P with numpy matrices,
    200 seeded steps of varying dt.  1e-12 relative is what two float64 orderings of a well-conditioned 2x2 allow."""
    rng = np.random.default_rng(20240611)
    q, r = 4.0, 0.01
    x = np.array([1.5, 0.0])
    P = np.diag([0.01, 4.0])
    sx, sv, p00, p01, p11 = 1.5, 0.0, 0.01, 0.0, 4.0
    H = np.array([[1.0, 0.0]])
    worst = 0.0
    truth = 1.5
    for step in range(200):
        dt = float(rng.uniform(0.01, 0.08))
        truth += 0.9 * dt
        z = truth + float(rng.uniform(-0.02, 0.02))
        F = np.array([[1.0, dt], [0.0, 1.0]])
        Q = q * np.array([[dt ** 4 / 4, dt ** 3 / 2], [dt ** 3 / 2, dt ** 2]])
        x = F @ x
        P = F @ P @ F.T + Q
        if step % 7 != 3:                      # some steps are misses: predict only
            S = H @ P @ H.T + r
            K = P @ H.T @ np.linalg.inv(S)
            x = x + (K @ (np.array([z]) - H @ x))
            P = (np.eye(2) - K @ H) @ P
        sx = T.Tracker.predict_axis(sx, sv, dt)
        p00, p01, p11 = T.Tracker.predict_cov(p00, p01, p11, dt, q)
        if step % 7 != 3:
            k0, k1 = T.Tracker.gains(p00, p01, r)
            sx, sv = T.Tracker.update_axis(sx, sv, z, k0, k1)
            p00, p01, p11 = T.Tracker.update_cov(p00, p01, p11, k0, k1)
        for got, want in ((sx, x[0]), (sv, x[1]), (p00, P[0, 0]), (p01, P[0, 1]), (p01, P[1, 0]), (p11, P[1, 1])):
            worst = max(worst, abs(got - want) / max(abs(want), 1e-300))
    print(f"worst relative difference over 200 steps: {worst:.3e}")
    assert worst <= 1e-12


# ---- 2. greedy rule ----
@pytest.mark.parametrize("seed,M,n,class_aware", [(0, 64, 100, False), (1, 64, 100, True), (2, 17, 5, True), (3, 3, 40, False),
                                                  (4, 64, 64, False), (5, 1, 1, False)])
def test_greedy_matching_equals_sorted_pairs(T, seed, M, n, class_aware):
    rng = np.random.default_rng(seed)
    # a coarse lattice (float32-exact) makes equal distances common
    tx, ty = rng.integers(0, 12, M) * 0.25, rng.integers(0, 12, M) * 0.25
    dx, dy = rng.integers(0, 12, n) * 0.25, rng.integers(0, 12, n) * 0.25
    tl, dl = rng.integers(0, 2, M).astype(np.int32), rng.integers(0, 2, n).astype(np.int32)
    live = rng.random(M) < 0.8
    gate = 0.75
    got = T.Tracker.associate(tx, ty, tl, live, dx, dy, dl, np.float64(gate), class_aware)
    pairs = []
    for s in range(M):
        for r in range(n):
            ex, ey = tx[s] - dx[r], ty[s] - dy[r]
            d2 = ex * ex + ey * ey
            if live[s] and d2 <= gate * gate and (not class_aware or tl[s] == dl[r]):
                pairs.append((d2, s, r))
    want = np.full(M, -1, np.int64)
    used = set()
    for d2, s, r in sorted(pairs):
        if want[s] < 0 and r not in used:
            want[s] = r
            used.add(r)
    assert np.array_equal(got, want)
    assert len(pairs) == 0 or (want >= 0).any()


# ---- 3. hand-made cases (float32-exact coordinates) ----
def test_gate_is_inclusive_and_one_ulp_beyond_is_not(pp, T):
    t = T.Tracker(_cfg(T), 2)
    t.step(*_dets(pp, [[(2.0, 1.0, 0.0, 0.9, 0)], [(2.0, 1.0, 0.0, 0.9, 0)]]), dt=[1e-3, 1e-3])
    beyond = float(np.nextafter(np.float32(2.0), np.float32(3.0)))
    # stream 0: offsets 0.75, 1.0 -> d2 = 1.5625 = 1.25^2 exactly; stream 1: one float32 ulp further in y
    tr, n, _ = t.step(*_dets(pp, [[(2.75, 2.0, 0.0, 0.9, 0)], [(2.75, beyond, 0.0, 0.9, 0)]]), dt=[1e-3, 1e-3])
    assert n[0] == 1 and tr[0, 0]["id"] == 1 and tr[0, 0]["hits"] == 2 and tr[0, 0]["det_row"] == 0
    assert n[1] == 2 and tr[1, 0]["hits"] == 1 and tr[1, 0]["misses"] == 1 and tr[1, 0]["det_row"] == -1
    assert tr[1, 1]["id"] == 2 and tr[1, 1]["det_row"] == 0


def test_equal_distances_take_the_lowest_slot_then_the_lowest_row(pp, T):
    t = T.Tracker(_cfg(T), 1)
    # two tracks (slots 0, 1) at x = 1 and x = 2
    t.step(*_dets(pp, [[(1.0, 0.0, 0.0, 0.9, 0), (2.0, 0.0, 0.0, 0.9, 0)]]), dt=[1e-3])
    # one row halfway: equally far from both -> slot 0
    tr, n, _ = t.step(*_dets(pp, [[(1.5, 0.0, 0.0, 0.9, 0)]]), dt=[1e-3])
    assert n[0] == 2 and tr[0, 0]["det_row"] == 0 and tr[0, 1]["det_row"] == -1
    # two rows equally far from track slot 0 alone (slot 1 is out of the gate): the lower row
    t2 = T.Tracker(_cfg(T, gate=0.5), 1)
    t2.step(*_dets(pp, [[(1.0, 0.0, 0.0, 0.9, 0)]]), dt=[1e-3])
    tr, n, _ = t2.step(*_dets(pp, [[(1.25, 0.0, 0.0, 0.9, 0), (0.75, 0.0, 0.0, 0.9, 0)]]), dt=[1e-3])
    assert tr[0, 0]["id"] == 1 and tr[0, 0]["det_row"] == 0
    assert n[0] == 2 and tr[0, 1]["id"] == 2 and tr[0, 1]["det_row"] == 1


def test_class_aware_on_and_off(pp, T):
    for aware, ids in ((True, [1, 2]), (False, [1])):
        t = T.Tracker(_cfg(T, class_aware=aware), 1)
        t.step(*_dets(pp, [[(1.0, 0.0, 0.0, 0.9, 0)]]))
        tr, n, _ = t.step(*_dets(pp, [[(1.0, 0.0, 0.0, 0.9, 1)]]))
        assert tr[0]["id"][:n[0]].tolist() == ids
        if not aware:
            assert tr[0, 0]["label"] == 1 and tr[0, 0]["hits"] == 2


def test_no_birth_below_birth_score(pp, T):
    t = T.Tracker(_cfg(T, birth_score=0.5), 1)
    tr, n, _ = t.step(*_dets(pp, [[(1.0, 0.0, 0.0, 0.49, 0), (3.0, 0.0, 0.0, 0.5, 0)]]))
    assert n[0] == 1 and tr[0, 0]["det_row"] == 1 and tr[0, 0]["id"] == 1
    # ... but a low-score row still updates an existing track
    tr, n, _ = t.step(*_dets(pp, [[(3.0, 0.0, 0.0, 0.1, 0)]]))
    assert n[0] == 1 and tr[0, 0]["hits"] == 2 and tr[0, 0]["score"] == np.float32(0.1)


def test_freed_slot_is_reused_in_the_same_step_lowest_first_and_ids_are_not(pp, T):
    t = T.Tracker(_cfg(T, max_misses=0), 1)
    t.step(*_dets(pp, [[(0.0, 0.0, 0.0, 0.9, 0), (5.0, 0.0, 0.0, 0.9, 0), (10.0, 0.0, 0.0, 0.9, 0)]]))
    # slots 0 and 2 get no row (max_misses = 0: freed at once); two far rows are born into slots 0 and 2, in row order
    tr, n, _ = t.step(*_dets(pp, [[(5.0, 0.0, 0.0, 0.9, 0), (20.0, 0.0, 0.0, 0.9, 0), (30.0, 0.0, 0.0, 0.9, 0)]]))
    assert n[0] == 3
    assert tr[0]["id"][:3].tolist() == [4, 2, 5]            # slot order; ids 1 and 3 are gone and not reused
    assert tr[0]["det_row"][:3].tolist() == [1, 0, 2]
    assert tr[0]["state"][:3, 0].tolist() == [20.0, 5.0, 30.0]
    assert t.info()["next_id"][0] == 6


def test_overflow_at_65_candidates(pp, T):
    t = T.Tracker(_cfg(T), 1)
    rows = [(2.0 * i, 0.0, 0.0, 0.9, 0) for i in range(65)]
    tr, n, ov = t.step(*_dets(pp, [rows]))
    assert n[0] == 64 and ov[0] == 1 and tr[0]["id"][:64].tolist() == list(range(1, 65))
    assert t.info()["next_id"][0] == 65
    tr, n, ov = t.step(*_dets(pp, [rows]))
    assert n[0] == 64 and ov[0] == 2 and (tr[0]["hits"][:64] == 2).all()


def test_min_hits_and_max_misses_boundaries(pp, T):
    t = T.Tracker(_cfg(T, min_hits=3, max_misses=2), 1)
    one = _dets(pp, [[(1.0, 0.0, 0.0, 0.9, 0)]])
    none = _dets(pp, [[]])
    conf = [int(t.step(*one)[0][0, 0]["confirmed"]) for _ in range(4)]
    assert conf == [0, 0, 1, 1]                               # confirmed exactly at the third hit
    counts = []
    for _ in range(4):
        tr, n, _ = t.step(*none)
        counts.append((int(n[0]), int(tr[0, 0]["misses"])))
    assert counts == [(1, 1), (1, 2), (0, 0), (0, 0)]         # freed exactly at miss max_misses + 1 = 3
    # confirmed stays through misses
    t.reset()
    for _ in range(3):
        t.step(*one)
    assert t.step(*none)[0][0, 0]["confirmed"] == 1


def test_flagged_frame_leaves_its_stream_untouched(pp, T):
    t = T.Tracker(_cfg(T), 2)
    d, n = _dets(pp, [[(1.0, 0.0, 0.0, 0.9, 0)], [(2.0, 0.0, 0.0, 0.9, 0)]])
    t.step(d, n)
    before = (t.x.copy(), t.p.copy(), t.hits.copy())
    n2 = n.copy()
    n2[1] |= 1 << 30
    t.step(d, n2)
    assert np.array_equal(t.x[1], before[0][1]) and np.array_equal(t.p[1], before[1][1]) and np.array_equal(t.hits[1], before[2][1])
    assert t.hits[0, 0] == 2


# ---- 4. behaviour ----
def _walk(pp, T, cfg, seed, steps=60, dropout=()):
    rng = np.random.default_rng(seed)
    t = T.Tracker(cfg, 1)
    v = np.array([0.9, -0.4, 0.0])
    out = None
    for i in range(steps):
        pos = np.array([2.0, 1.0, -0.6]) + v * (i / 30.0) + rng.uniform(-0.02, 0.02, 3)
        rows = [] if i in dropout else [(pos[0], pos[1], pos[2], 0.8, 0)]
        out = t.step(*_dets(pp, [rows]))
    return out


def test_constant_velocity_target(pp, T):
    """(0.9, -0.4, 0) m/s, +-2 cm uniform noise, 30 Hz, 60 steps, the default configuration: within 0.1 m/s of the truth.
    Seeds 0..4 show a worst component error of 0.024 m/s (printed): a margin of four."""
    worst = 0.0
    for seed in range(5):
        tr, n, _ = _walk(pp, T, T.TrackConfig(), seed)
        assert n[0] == 1 and tr[0, 0]["id"] == 1 and tr[0, 0]["hits"] == 60
        err = np.abs(tr[0, 0]["state"][3:] - np.array([0.9, -0.4, 0.0])).max()
        worst = max(worst, err)
        assert err <= 0.1, (seed, err)
    print(f"worst velocity error over seeds 0..4: {worst:.4f} m/s")


def test_crossing_targets_keep_their_ids(pp, T):
    """Two pedestrians walking in opposite directions along x on lanes 1 m apart in y, passing each other at step 30: the
    smallest centre distance is the 1 m lane separation, the predicted tracks stay within a few cm of their own rows."""
    rng = np.random.default_rng(11)
    t = T.Tracker(T.TrackConfig(), 1)
    for i in range(60):
        a = np.array([2.0 + 0.9 * i / 30.0, 0.0, -0.6]) + rng.uniform(-0.02, 0.02, 3)
        b = np.array([3.8 - 0.9 * i / 30.0, 1.0, -0.6]) + rng.uniform(-0.02, 0.02, 3)
        rows = [(a[0], a[1], a[2], 0.8, 0), (b[0], b[1], b[2], 0.7, 0)]
        if i % 2:
            rows.reverse()                    # the detector's row order follows the scores, not the identities
        tr, n, _ = t.step(*_dets(pp, [rows]))
        assert n[0] == 2
    by_id = {int(r["id"]): r for r in tr[0, :2]}
    assert set(by_id) == {1, 2}
    assert by_id[1]["state"][3] > 0.7 and by_id[2]["state"][3] < -0.7       # each kept its own direction
    assert abs(by_id[1]["state"][1]) < 0.1 and abs(by_id[2]["state"][1] - 1.0) < 0.1


def test_dropout_of_five_frames(pp, T):
    """Steps 30..34 carry no detection.  max_misses = 5: the track coasts on its velocity (5 frames at 1 m/s and a velocity
    good to 0.03 m/s leave it within a centimetre of the next detection, against a gate of 0.6 m) and keeps id 1 with 55
    hits; max_misses = 4: it is freed at the fifth miss and the target comes back as id 2 with the 25 hits that follow."""
    gap = range(30, 35)
    tr, n, _ = _walk(pp, T, T.TrackConfig(max_misses=5), 3, dropout=gap)
    assert n[0] == 1 and tr[0, 0]["id"] == 1 and tr[0, 0]["hits"] == 55
    tr, n, _ = _walk(pp, T, T.TrackConfig(max_misses=4), 3, dropout=gap)
    assert n[0] == 1 and tr[0, 0]["id"] == 2 and tr[0, 0]["hits"] == 25


# ---- 5. plumbing ----
def test_config_key_parses_and_echoes(pp, T):
    cfg = pp.config.tiny_config(1)
    assert pp.config.Derived(cfg).tracking is None
    cfg["model"]["second"]["tracking"] = False
    assert pp.config.Derived(cfg).tracking is None
    cfg["model"]["second"]["tracking"] = True
    assert pp.config.Derived(cfg).tracking == T.TrackConfig().to_dict()
    cfg["model"]["second"]["tracking"] = {"gate": 0.8, "max_misses": 3}
    d = pp.config.Derived(cfg).tracking
    assert d == dict(T.TrackConfig().to_dict(), gate=0.8, max_misses=3)
    assert T.TrackConfig().period == 1.0 / 30.0 and T.TrackConfig().gate == 0.6
    assert T.TrackConfig().max_misses == 5 and T.TrackConfig().min_hits == 3


@pytest.mark.parametrize("field,value", [("gate", 0.0), ("gate", float("nan")), ("q_acc", -1.0), ("r_pos", 0.0), ("p0_pos", 0.0),
                                         ("p0_vel", float("inf")), ("size_alpha", 1.5), ("size_alpha", -0.1),
                                         ("birth_score", float("nan")), ("period", 0.0), ("max_misses", -1), ("min_hits", 0),
                                         ("min_hits", 1.5), ("gate", "wide")])
def test_bad_fields_raise_naming_the_field(pp, T, field, value):
    with pytest.raises(ValueError, match=field):
        T.TrackConfig(**{field: value})
    cfg = pp.config.tiny_config(1)
    cfg["model"]["second"]["tracking"] = {field: value}
    with pytest.raises(ValueError, match=field):
        pp.config.Derived(cfg)


def test_unknown_key_and_wrong_type_raise(pp, T):
    cfg = pp.config.tiny_config(1)
    cfg["model"]["second"]["tracking"] = {"gait": 1.0}
    with pytest.raises(ValueError, match="gait"):
        pp.config.Derived(cfg)
    cfg["model"]["second"]["tracking"] = 3
    with pytest.raises(ValueError, match="tracking"):
        pp.config.Derived(cfg)


def test_stamps_to_dt(T):
    last = np.array([np.nan, 10.0, 5.0])
    dt, new = T.stamps_to_dt(last, [1.0, 10.25, 5.5], 3, 1.0 / 30.0)
    assert dt.tolist() == [1.0 / 30.0, 0.25, 0.5] and new.tolist() == [1.0, 10.25, 5.5]
    assert np.isnan(last[0])                                   # not changed in place
    with pytest.raises(ValueError, match="stream 1"):
        T.stamps_to_dt(last, [1.0, 10.0, 6.0], 3, 1.0 / 30.0)  # equal: does not increase
    with pytest.raises(ValueError, match="stream 2"):
        T.stamps_to_dt(last, [1.0, 11.0, 4.0], 3, 1.0 / 30.0)
    with pytest.raises(ValueError, match="stream 0"):
        T.stamps_to_dt(last, [np.inf, 11.0, 6.0], 3, 1.0 / 30.0)
    with pytest.raises(ValueError, match="2 values for 3"):
        T.stamps_to_dt(last, [1.0, 11.0], 3, 1.0 / 30.0)


NEW = ["pp_set_tracking", "pp_get_tracking", "pp_set_track_dt", "pp_get_tracks", "pp_track_update", "pp_track_reset",
       "pp_track_info"]


def test_header_exports_and_sources(pp):
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    assert "#define PP_ABI_VERSION 4" in hdr
    head = hdr[:hdr.index("#define PP_ABI_VERSION")]
    later = head[head.index("later additions within 4"):]
    at = later.index("pp_soft_nms.")
    for name in ["PP_TRACK_MAX", "pp_track_config", "pp_track"] + NEW:
        assert re.search(r"\b%s\b" % name, later[at:]), name
    ex = pp._lib.EXPORTS
    assert ex[ex.index("pp_soft_nms") + 1:] == NEW
    assert pp._lib.SOURCES[-2:] == ["api_track.hip", "track.hip"]
    for src in pp._lib.SOURCES[-2:]:
        assert os.path.exists(os.path.join(os.path.dirname(pp._lib.__file__), "csrc", src))


def _c_struct_size(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = 0
    for ctype, names in re.findall(r"(double|float|int32_t)\s+([^;]+);", body):
        w = {"double": 8, "float": 4, "int32_t": 4}[ctype]
        for nm in names.split(","):
            m = re.search(r"\[(\d+)\]", nm)
            assert size % w == 0, (name, nm)                   # no padding inside
            size += w * (int(m.group(1)) if m else 1)
    return size


def test_struct_sizes_match_the_header(pp, T):
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    assert _c_struct_size(hdr, "pp_track_config") == ctypes.sizeof(pp._lib.PPTrackConfig) == 80
    assert _c_struct_size(hdr, "pp_track") == ctypes.sizeof(pp._lib.PPTrack) == T.TRACK_DTYPE.itemsize == 112
    # field by field: the numpy rows are the C rows
    for f, _ in pp._lib.PPTrack._fields_:
        assert T.TRACK_DTYPE.fields[f][1] == getattr(pp._lib.PPTrack, f).offset, f
    src = open(os.path.join(os.path.dirname(pp._lib.__file__), "csrc", "api_track.hip")).read()
    assert "static_assert(sizeof(pp_track_config) == 80" in src and "static_assert(sizeof(pp_track) == 112" in src
    assert re.search(r"#define PP_TRACK_MAX 64\b", hdr) and pp._lib.PP_TRACK_MAX == T.PP_TRACK_MAX == 64


def test_det_track_ids_and_velocity(T):
    tr = np.zeros(64, T.TRACK_DTYPE)
    tr["id"][:3] = [7, 8, 9]
    tr["det_row"][:3] = [2, -1, 0]
    tr["state"][:3, 3:] = [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
    assert T.det_track_ids(tr, 3, 4).tolist() == [9, -1, 7, -1]
    assert T.det_track_velocity(tr, 3, 4).tolist() == [[7, 8, 9], [0, 0, 0], [1, 2, 3], [0, 0, 0]]
    assert T.det_track_ids(tr, 0, 2).tolist() == [-1, -1]


def test_track_np_is_the_tracker(pp, T):
    frames = [_dets(pp, [[(1.0 + 0.03 * i, 0.0, 0.0, 0.9, 0)]]) for i in range(5)]
    outs = T.track_np(_cfg(T), frames, dts=[[0.04]] * 5)
    t = T.Tracker(_cfg(T), 1)
    for (d, n), got in zip(frames, outs):
        want = t.step(d, n, [0.04])
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert outs[-1][0][0, 0]["hits"] == 5
