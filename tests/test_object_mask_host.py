"""The per-point object mask on the host (object_mask.py: the rule the GPU stage mirrors).  `object_mask_np` is held to a
second, loop-based statement; the boundary, the NaN rows and the non-finite footprints are hand-made; the carry and the
predict of the tracks' copies are held to tracking.Tracker bit for bit; the three readers' restatements are unchanged
without a mask; and the room a square object crosses shows what the stage is for.  No GPU."""
import copy
import math

import numpy as np
import pytest

import object_mask_cases as oc


def _loop_mask(points, footprints):
    """The rule once more, a row and a footprint at a time in Python floats."""
    out = []
    for r in np.asarray(points):
        x, y = float(r[0]), float(r[1])
        inside = False
        for ox, oy, c, s, hx, hy in np.asarray(footprints, np.float64).reshape(-1, 6).tolist():
            dx, dy = x - ox, y - oy
            u, v = (dx * c) - (dy * s), (dx * s) + (dy * c)
            inside = inside or (abs(u) <= hx and abs(v) <= hy)
        out.append(inside)
    return np.array(out, bool)


@pytest.mark.parametrize("seed", oc.SEEDS)
def test_restatement_against_the_loop(pp, seed):
    om = pp.object_mask
    frames, rects, pad = oc.seeded_case(seed)
    some = 0
    for f, r in zip(frames, rects):
        fp = om.rect_footprints_np(r, pad)
        assert len(fp) == max(len(r) - (3 if len(r) > 4 else 0), 0)          # the non-finite rectangles are left out
        got = om.object_mask_np(f, fp)
        assert got.dtype == bool and got.shape == (len(f),)
        assert np.array_equal(got, _loop_mask(f, fp))
        m = om.point_margins_np(f, fp)
        assert not (m < oc.MARGIN).any(), (seed, float(np.nanmin(m)))       # no row of a seeded case is undecided
        bad = ~np.isfinite(f[:, :2]).all(1)
        assert not got[bad].any()
        some += int(got.sum())
        assert np.array_equal(om.unpack_words(om.pack_words(got), len(f)), got)
    assert some > 0


def test_sizes_cover_the_issue():
    rows = {r for r, _ in oc.size_cases()}
    fps = {k for _, k in oc.size_cases()}
    assert rows == set(oc.ROWS) and fps == set(oc.FOOTPRINTS)
    for seed in oc.SEEDS:
        frames, _, _ = oc.seeded_case(seed)
        assert len({len(f) for f in frames}) > 1 and any(sum(len(g) for g in frames[:j]) % 64 for j in (1, 2))


def test_boundary_nan_and_non_finite_footprints(pp):
    om = pp.object_mask
    rows, inside = oc.boundary_rows()
    fp = om.rect_footprints_np(oc.BOUNDARY_RECT)
    assert fp.tolist() == [[1.0, 2.0, 1.0, 0.0, 0.5, 0.25]]
    assert np.array_equal(om.object_mask_np(rows, fp), inside)
    assert np.array_equal(_loop_mask(rows, fp), inside)
    assert (om.point_margins_np(rows, fp)[[0, 2, 4, 6]] == 0.0).all()        # ON the edge: inside, by <=
    # a NaN row, in either coordinate, and an infinite one
    bad = np.array([[np.nan, 2.0, 0], [1.0, np.nan, 0], [np.inf, 2.0, 0], [1.0, -np.inf, 0]], np.float32)
    assert not om.object_mask_np(bad, fp).any()
    # a footprint with a non-finite field covers nothing, whichever field it is
    for k in range(5):
        r = oc.BOUNDARY_RECT.copy()
        r[0, k] = (np.nan, np.inf, -np.inf, np.nan, np.inf)[k]
        assert len(om.rect_footprints_np(r)) == 0
        assert not om.object_mask_np(rows, om.rect_footprints_np(r)).any()
    # a negative half extent (w + 2 pad < 0) covers nothing; pad widens
    assert not om.object_mask_np(rows, om.rect_footprints_np([[1.0, 2.0, -1.0, 0.5, 0.0]])).any()
    wide = om.object_mask_np(rows, om.rect_footprints_np(oc.BOUNDARY_RECT, pad=0.5))
    assert wide[:11].all() and not wide[11]
    # the empty table and the empty frame
    assert not om.object_mask_np(rows, np.zeros((0, 6))).any() and np.isinf(om.point_margins_np(rows, np.zeros((0, 6)))).all()
    assert om.object_mask_np(np.zeros((0, 3), np.float32), fp).shape == (0,)
    with pytest.raises(ValueError, match="float32"):
        om.object_mask_np(rows.astype(np.float64), fp)


def _tracker(pp):
    t = pp.tracking.Tracker(oc.TRACK, oc.TRACK_STREAMS)
    for dets, n, dt, poses in oc.track_steps(pp):
        t.step(dets, n, dt, poses)
    return t


def test_carry_and_predict_against_the_tracker(pp):
    om = pp.object_mask
    t = _tracker(pp)
    assert t.has_prev.all()
    before = copy.deepcopy(t.__dict__)
    tr, nt, _ = t.tracks()
    assert nt.tolist() == [3, 1]
    poses, dt = oc.peek_pose(pp)
    cfg = dict(objects="tracks", pad=0.1)
    fps = [om.footprints_np(cfg, tracks=tr[s], n_tracks=nt[s], pose=poses[s], prev=(t.prev_pose[s], t.prev_psi[s]), dt=dt[s])
           for s in range(2)]
    # a copy of the tracker stepped with the same poses and dt and no detections: its predicted state is the footprints' centres
    t2 = copy.deepcopy(t)
    empty = np.zeros((2, 1), pp.Engine.det_dtype())
    tr2, nt2, _ = t2.step(empty, [0, 0], dt, poses)
    assert nt2.tolist() == nt.tolist()
    for s in range(2):
        assert fps[s].shape == (nt[s], 6)
        assert fps[s][:, :2].tobytes() == tr2["state"][s, :nt[s], :2].tobytes()              # bit for bit
        cs = np.array([(math.cos(y), math.sin(y)) for y in tr2["yaw"][s, :nt[s]]])
        assert fps[s][:, 2:4].tobytes() == cs.tobytes()                                       # yaw + (psi_c - prev_psi)
        assert np.array_equal(fps[s][:, 4], tr["size"][s, :nt[s], 0] * 0.5 + 0.1)
        st, _ = om.peek_tracks_np(tr[s], nt[s], poses[s], (t.prev_pose[s], t.prev_psi[s]), dt[s])
        assert st[:, 3:5].tobytes() == tr2["state"][s, :nt[s], 3:5].tobytes()                 # the carried velocity
    # the original tracker is untouched: a peek, not a step
    for k, v in before.items():
        w = t.__dict__[k]
        assert (v.tobytes() == w.tobytes()) if isinstance(v, np.ndarray) else (v == w), k
    # without a previous pose the carry is skipped; without dt nothing is predicted
    plain = om.footprints_np(cfg, tracks=tr[0], n_tracks=nt[0])
    assert plain[:, :2].tobytes() == tr["state"][0, :3, :2].tobytes()
    assert om.footprints_np(cfg, tracks=tr[0], n_tracks=nt[0], pose=poses[0], prev=None).tobytes() == plain.tobytes()
    only_dt = om.footprints_np(cfg, tracks=tr[0], n_tracks=nt[0], dt=0.5)
    x = tr["state"][0, :3]
    assert only_dt[:, 0].tobytes() == (x[:, 0] + x[:, 3] * 0.5).tobytes() and only_dt[:, 1].tobytes() == (x[:, 1] + x[:, 4] * 0.5).tobytes()


def test_min_speed_confirmed_only_min_score_boundaries(pp):
    om = pp.object_mask
    t = _tracker(pp)
    tr, nt, _ = t.tracks()
    v2 = tr["state"][0, :3, 3] ** 2 + tr["state"][0, :3, 4] ** 2
    walker = int(np.argmax(v2))
    assert tr["confirmed"][0, :3].tolist() == [1, 1, 0] and v2[walker] > 0
    n_fp = lambda **kw: len(om.footprints_np(dict(objects="tracks", **kw), tracks=tr[0], n_tracks=nt[0]))    # noqa: E731
    assert n_fp() == 3 and n_fp(confirmed_only=True) == 2
    # (vx * vx + vy * vy) >= min_speed * min_speed, inclusive: a threshold whose square IS v2 keeps the track
    s = math.sqrt(v2[walker])
    lo, hi = (s, np.nextafter(s, np.inf)) if s * s <= v2[walker] else (np.nextafter(s, -np.inf), s)
    assert lo * lo <= v2[walker] < hi * hi
    slower = int((v2 >= lo * lo).sum())
    assert n_fp(min_speed=lo) == slower >= 1 and n_fp(min_speed=hi) == int((v2 >= hi * hi).sum()) < slower
    assert n_fp(min_speed=0.0) == 3                                                             # a parked object masks at 0
    # detections: score >= min_score, inclusive; a flagged frame has none
    dets, n = oc.det_rows(pp, [[(0.5, 0.5, 0.4, 0.6, 0.2, 0.5), (1.5, 0.5, 0.4, 0.6, 0.2, 0.25), (2.5, 0.5, 0.4, 0.6, 0.2, 0.75)]])
    d_fp = lambda ms, nn=int(n[0]): om.footprints_np(dict(objects="detections", min_score=ms), dets=dets[0], n_dets=nn)    # noqa: E731
    assert len(d_fp(0.5)) == 2 and len(d_fp(np.nextafter(np.float32(0.5), np.float32(1)))) == 1 and len(d_fp(0.0)) == 3
    assert d_fp(0.5)[:, 0].tolist() == [0.5, 2.5]                                               # in row order
    assert len(d_fp(0.0, 3 | (1 << 30))) == 0
    # the configuration's own checks
    C = om.ObjectMaskConfig
    assert C(objects="detections", consumers="costmap").to_dict()["consumers"] == 4 and C(consumers=3).consumers == ("occupancy", "scan_match")
    for bad, what in ((dict(pad=-0.1), "pad"), (dict(min_speed=-1.0), "min_speed"), (dict(objects="none"), "objects"),
                      (dict(consumers=("maps",)), "consumers"), (dict(min_score=math.nan), "min_score"), (dict(objects=0), "objects")):
        with pytest.raises(ValueError, match=what):
            C(**bad)
    with pytest.raises(ValueError, match="unknown keys"):
        C.from_any(dict(padding=1.0))


def test_readers_without_a_mask_are_what_they_were(pp):
    """mask=None is the call without the argument, and a mask that names no row gives the same results: on the recovery
    room of the scan match and on a frame of the navigation cycle."""
    import nav_cycle_cases as nc
    import scan_match_cases as sc
    m, pts, prior, _ = sc.room_case(pp, 3)
    none = np.zeros(len(pts), bool)
    w0, s0 = pp.scan_match.match_np(m, pts, prior, sc.ROOM_SCAN)
    for mask in (None, none):
        w, s = pp.scan_match.match_np(m, pts, prior, sc.ROOM_SCAN, mask=mask)
        assert w.tobytes() == w0.tobytes() and s.tobytes() == s0.tobytes()
        c1, t1 = pp.scan_match.scan_cells_np(sc.ROOM_OCC, pts, prior, mask)
        c0, t0 = pp.scan_match.scan_cells_np(sc.ROOM_OCC, pts, prior)
        assert c1.tobytes() == c0.tobytes() and t1 == t0
    a, b, c = (pp.occupancy.OccupancyMap(sc.ROOM_OCC) for _ in range(3))
    ia, ib, ic = a.update(pts, prior), b.update(pts, prior, mask=None), c.update(pts, prior, mask=none)
    assert ia == ib and list(ia) == list(nc.OCC_INFO) and ic == dict(ia, masked=0)
    assert a.logodds().tobytes() == b.logodds().tobytes() == c.logodds().tobytes() and a.grid().tobytes() == c.grid().tobytes()
    rng = np.random.default_rng(9)
    f = rng.uniform([-0.7, -1.2, -1.4], [2.3, 1.3, 1.4], (700, 3)).astype(np.float32)
    g0, k0 = pp.costmap.costmap_np(f, nc.GRID)
    for mask in (None, np.zeros(700, bool)):
        g, k = pp.costmap.costmap_np(f, nc.GRID, mask=mask)
        assert g.tobytes() == g0.tobytes() and k.tobytes() == k0.tobytes()
    for fn in (lambda: pp.costmap.costmap_np(f, nc.GRID, mask=np.zeros(3, bool)), lambda: a.update(pts, prior, mask=np.zeros(3, bool)),
               lambda: pp.scan_match.scan_cells_np(sc.ROOM_OCC, pts, prior, np.zeros(3, bool))):
        with pytest.raises(ValueError, match="mask must be bool"):
            fn()


def test_what_a_masked_row_does_to_each_reader(pp):
    """Hand-made rows: a masked end keeps its ray and leaves no hit; a hit from an unmasked row in the same cell wins; a
    ground row is unaffected; the scan ignores the row; the costmap observes its cell and counts nothing."""
    occ = dict(resolution=1.0, width=9, height=9, z_min=0.0, z_max=2.0, max_range=50.0)
    I = np.array([[1.0, 0, 0, 0.5], [0, 1.0, 0, 0.5], [0, 0, 1.0, 0]])                  # the sensor in the middle of cell (4, 4)
    rows = np.array([[3.0, 0.0, 1.0], [0.0, 3.0, 1.0], [0.0, 3.2, 1.0], [-3.0, 0.0, -1.0]], np.float32)
    mask = np.array([True, True, False, True])
    m = pp.occupancy.OccupancyMap(occ)
    info = m.update(rows, I, mask=mask)
    assert info == dict(hits=1, ground=1, ignored=0, cells_hit=1, cells_free=8, cleared=81, masked=2)
    L = m.logodds()
    assert L[4, 7] == 0 and not m.known()[4, 7]                                          # the masked end: neither hit nor passed
    assert (L[4, 4:7] == -m.cfg.l_miss).all()                                            # ... and the free space in front of it is kept
    assert L[7, 4] == m.cfg.l_hit                                                        # the unmasked row of that cell wins
    assert L[4, 1] == -m.cfg.l_miss                                                      # the ground row frees its own cell, masked or not
    cells, tally = pp.scan_match.scan_cells_np(occ, rows, I, mask)
    assert tally == (1, 3, 1) and cells.tolist() == [[512, 3 * 1024 + 512]]
    cm = dict(x_min=-4.5, y_min=-4.5, resolution=1.0, width=9, height=9, z_min=0.0, z_max=2.0)
    g, k = pp.costmap.costmap_np(rows, cm, mask=mask)
    assert k.sum() == 1 and k[7, 4] == 1 and g[4, 7] == 0 and g[7, 4] == 100 and g[4, 1] == 0 and (g == -1).sum() == 78


def test_a_crossing_object_leaves_no_ghost(pp):
    """The room of the issue: 40 frames of 1440 planar rays from a static sensor while a 0.6 m square object crosses 3 m in
    front of it.  As the map stands, inner cells stay at cost >= 65; with the rows inside the object's (padded) rectangle
    masked there is none after ANY frame, and the walls are the unmasked run's."""
    om = pp.object_mask
    inner = oc.room_regions(pp)
    plain, masked = pp.occupancy.OccupancyMap(oc.ROOM_OCC), pp.occupancy.OccupancyMap(oc.ROOM_OCC)
    pose = pp.sweeps.pose_from_xyyaw(0.0, 0.0, 0.0)
    n_masked = 0
    for k in range(oc.ROOM_FRAMES):
        rows, rect = oc.room_frame(k)
        fp = om.rect_footprints_np(rect, oc.ROOM_PAD)
        bits = om.object_mask_np(rows, fp)
        assert not (om.point_margins_np(rows, fp) < oc.MARGIN).any()
        n_masked += int(bits.sum())
        plain.update(rows, pose)
        info = masked.update(rows, pose, mask=bits)
        assert info["masked"] == int(bits.sum()) > 0
        g = masked.grid()
        assert int(((g >= oc.ROOM_COST) & inner).sum()) == 0, k
        assert np.array_equal((g >= oc.ROOM_COST) & ~inner, (plain.grid() >= oc.ROOM_COST) & ~inner), k
    ghosts = int(((plain.grid() >= oc.ROOM_COST) & inner).sum())
    walls = int(((plain.grid() >= oc.ROOM_COST) & ~inner).sum())
    print(f"crossing object: {ghosts} inner cells at cost >= {oc.ROOM_COST} unmasked, 0 masked; {walls} wall cells in both; {n_masked} rows masked")
    assert ghosts >= 1 and walls >= 300
