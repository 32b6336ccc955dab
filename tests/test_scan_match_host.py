"""The scan match's rule (scan_match.py) without a GPU: hand-made maps with the expected scores written out, the rounded
rotation and the cell shift on negative coordinates, the two statements of the score against each other, the tie rules,
every status bit, the corrected pose, the configuration's refusals, the C-ABI's structure -- and RECOVERY, which is a
property of the rule: in the L-shaped room the restatement finds a prior displaced by whole steps."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import scan_match_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def S(pp):
    return pp.scan_match


def _match(S, oc, L, known, origin, rows, pose, **scan):
    scan = dict(dict(nx=1, ny=1, nt=0, xy_step=1024, theta_step=8, min_cells=0, min_mean=-100000), **scan)
    return S.match_grid_np(oc, L, known, origin, rows, pose, scan)


# ---- hand-made maps: 1 m cells, the sensor on the lower corner of cell (4, 3), a scan of three cells ----
SCAN3 = [(1, 0), (2, 0), (2, 1)]                 # sensor-frame cells: they land on (5, 3), (6, 3), (6, 4) under the prior


def test_one_cell_wall_and_a_three_cell_scan(pp, S):
    oc, L, known = K.blank(pp, 9, 7)
    L[3, 5], known[3, 5] = 85, True
    cells, counts = S.scan_cells_np(oc, K.rows_at(SCAN3), K.IDENTITY)
    assert cells.tolist() == [[1536, 512], [2560, 512], [2560, 1536]] and counts == (3, 0, 3)
    assert S.sensor_subcells(oc, K.at(4.0, 3.0), (0, 0)) == (4096, 3072)
    words, scores = _match(S, oc, L, known, (0, 0), K.rows_at(SCAN3), K.at(4.0, 3.0))
    # c = iy * 3 + ix: the wall cell under the third scan cell (-1, -1), the second (-1, 0), the first (0, 0)
    assert scores.tolist() == [85, 0, 0, 85, 85, 0, 0, 0, 0]
    assert words.tolist() == [0, 0, 0, 0, 85, 85, 3, 0]          # three candidates tie: the smallest motion wins


def test_a_negative_cell_costs_and_an_unknown_cell_does_not(pp, S):
    oc, L, known = K.blank(pp, 9, 7)
    L[3, 5], known[3, 5] = 85, True
    L[3, 6], known[3, 6] = -41, True
    words, scores = _match(S, oc, L, known, (0, 0), K.rows_at(SCAN3), K.at(4.0, 3.0))
    assert scores.tolist() == [85, -41, 0, 85, 44, -41, 0, 0, 0]
    assert words.tolist() == [S.EDGE, -1, 0, 0, 85, 44, 3, 0]    # 85 at d = 2 and d = 1: the smaller motion, on the face of x
    known[3, 6] = False                                          # the same L, not known: it adds nothing
    words, scores = _match(S, oc, L, known, (0, 0), K.rows_at(SCAN3), K.at(4.0, 3.0))
    assert scores.tolist() == [85, 0, 0, 85, 85, 0, 0, 0, 0] and words.tolist() == [0, 0, 0, 0, 85, 85, 3, 0]


def test_a_candidate_that_pushes_scan_cells_out_of_the_window(pp, S):
    oc, L, known = K.blank(pp, 9, 7)
    L[:], known[:] = 10, True
    # the sensor on cell (7, 3): under the prior the scan lands on (8, 3), (9, 3), (9, 4), two of them outside
    words, scores = _match(S, oc, L, known, (0, 0), K.rows_at(SCAN3), K.at(7.0, 3.0), ny=0)
    assert scores.tolist() == [30, 10, 0]
    assert words.tolist() == [S.EDGE, -1, 0, 0, 30, 10, 3, 0]
    # a window whose origin is not (0, 0), negative too: the sensor's sub-cells are relative to it
    assert S.sensor_subcells(oc, K.at(-2.5, 3.25), (-10, 3)) == (7680, 256)
    words2, scores2 = _match(S, oc, L, known, (-3, 5), K.rows_at(SCAN3), K.at(4.0, 8.0), ny=0)
    assert scores2.tolist() == scores.tolist()


def test_shifts_are_floor_on_negative_coordinates(pp, S):
    assert (-16384 * 512 + 8192) >> 14 == -512 and int((-16384 * 512 + 8192) / 16384) == -511
    # the rounded rotation: sensor-frame cell (-2, 0) turned by +1024 ticks (a quarter turn): rx = -512 by floor (-511 by
    # truncation), ry = -1536; with sx = 4096 + 511 the cell is (3, 2) by floor and (4, 2) by truncation
    oc, L, known = K.blank(pp, 9, 9)
    L[2, 3], L[2, 4] = 7, -9
    known[:] = True
    pose = K.at((4096 + 511) / 1024.0, 4.0)
    assert S.sensor_subcells(oc, pose, (0, 0)) == (4607, 4096)
    cfg = dict(nx=0, ny=0, nt=2, xy_step=1, theta_step=512, min_cells=0, min_mean=-100000)
    cells, _ = S.scan_cells_np(oc, K.rows_at([(-2, 0)]), pose)
    assert cells.tolist() == [[-1536, 512]]
    words, scores = S.match_grid_np(oc, L, known, (0, 0), K.rows_at([(-2, 0)]), pose, cfg)
    assert scores[4] == 7 == S.score_np(L, known, cells, (4607, 4096), cfg, 4)
    # the cell shift: a scan cell left of the window's first column is OUTSIDE (cell -1), not cell 0
    oc, L, known = K.blank(pp, 5, 5)
    L[:, 0], known[:] = 50, True
    words, scores = _match(S, oc, L, known, (0, 0), K.rows_at([(-1, 0)]), K.at(0.25, 2.0), nx=0, ny=0)
    assert scores.tolist() == [0] and words.tolist()[4:] == [0, 0, 1, 0]


def test_scan_cells_tests_and_counts(pp, S):
    oc = pp.occupancy.OccupancyConfig(resolution=0.5, width=9, height=7, z_min=0.0, z_max=1.0, max_range=1.8)
    f32 = np.float32
    rows = np.array([[0.1, 0.1, 0.5], [0.2, 0.3, 0.9], [0.6, 0.1, 0.0], [0.6, 0.1, -1e-6], [0.6, 0.1, np.nextafter(f32(1.0), f32(2.0))],
                     [1.8, 0.0, 0.5], [np.nextafter(f32(1.8), f32(2.0)), 0.0, 0.5], [-2.1, 0.0, 0.5], [np.nan, 0.0, 0.5], [0.0, 0.0, np.nan],
                     [-0.1, -0.1, 0.5], [np.inf, 0.0, 0.5]], np.float32)
    cells, (used, ignored, n_scan) = S.scan_cells_np(oc, rows, K.IDENTITY)
    # rows 0 and 1 share cell (4, 3); row 2 is cell (5, 3) at z = z_min; rows 3 and 4 fail z; row 5 is on max_range in cell
    # (7, 3), row 6 beyond it; row 7 lies in cell (-1, 3); the NaN and infinite rows fail; row 10 is cell (3, 2)
    assert (used, ignored, n_scan) == (5, 7, 4)
    assert cells.tolist() == [[-512, -512], [512, 512], [1536, 512], [3584, 512]]          # ascending (gy, gx)
    # a rotation: the prior's yaw turns the rows before they are binned; its translation plays no part
    P = pp.sweeps.pose_from_xyyaw(100.0, -50.0, math.pi / 2)
    cells, _ = S.scan_cells_np(oc, np.array([[0.6, 0.1, 0.5]], np.float32), P)
    assert cells.tolist() == [[-512, 1536]]
    with pytest.raises(ValueError, match="float32"):
        S.scan_cells_np(oc, rows.astype(np.float64), K.IDENTITY)


def test_both_statements_of_the_score_agree_on_every_candidate(pp, S):
    rng = np.random.default_rng(5)
    oc = pp.occupancy.OccupancyConfig(resolution=0.2, width=23, height=17, z_min=0.0, z_max=1.0, max_range=3.0)
    L, known = K.random_map(rng, 23, 17)
    rows = K.random_rows(rng, 150, 23, 17, 0.2)
    pose = pp.sweeps.pose_from_xyyaw(0.93, -0.41, 0.8)
    cfg = S.ScanMatchConfig(nx=3, ny=2, nt=3, xy_step=700, theta_step=300, min_cells=0, min_mean=0)
    origin = (int(math.floor(0.93 / 0.2)) - 18, int(math.floor(-0.41 / 0.2)) - 4)          # near a corner: candidates leave
    cells, counts = S.scan_cells_np(oc, rows, pose)
    sensor = S.sensor_subcells(oc, pose, origin)
    assert 20 <= counts[2] <= 150 and 0 <= sensor[0] >> 10 < 23 and 0 <= sensor[1] >> 10 < 17
    all_at_once = S.scores_np(L, known, cells, sensor, cfg)
    one_by_one = [S.score_np(L, known, cells, sensor, cfg, c) for c in range(cfg.candidates)]
    assert all_at_once.tolist() == one_by_one and len(set(one_by_one)) > cfg.candidates // 2
    words, scores = S.match_grid_np(oc, L, known, origin, rows, pose, cfg)
    assert scores.tolist() == one_by_one and words[4] == max(one_by_one) and words[5] == one_by_one[cfg.candidates // 2]


def _corridor(pp, wall_rows):
    oc, L, known = K.blank(pp, 31, 15)
    L[:], known[:] = -41, True
    for r in wall_rows:
        L[r, :] = 85
    return oc, L, known


def test_ties_go_to_the_smallest_motion_then_the_lowest_index(pp, S):
    line = [(k, 3) for k in range(-5, 6)]                       # a scan of a straight wall along x, 3 cells up from the sensor
    # the wall is row 11; the sensor on cell (15, 7): the scan lands on row 10, one below: every x shift ties
    oc, L, known = _corridor(pp, [11])
    words, scores = _match(S, oc, L, known, (0, 0), K.rows_at(line), K.at(15.0, 7.0), nx=2, ny=2)
    assert words.tolist() == [0, 0, 1, 0, 11 * 85, 11 * -41, 11, 0]
    assert (scores.reshape(5, 5)[3] == 11 * 85).all()
    # walls on rows 9 and 11: dy = -1 and dy = +1 tie in score and motion: the lower index
    oc, L, known = _corridor(pp, [9, 11])
    words, _ = _match(S, oc, L, known, (0, 0), K.rows_at(line), K.at(15.0, 7.0), nx=2, ny=2)
    assert words.tolist()[:5] == [0, 0, -1, 0, 11 * 85]
    # every candidate ties: the prior
    L[:] = 20
    words, scores = _match(S, oc, L, known, (0, 0), K.rows_at(line), K.at(15.0, 7.0), nx=2, ny=2, nt=1)
    assert len(set(scores.tolist())) == 1 and words.tolist()[:6] == [0, 0, 0, 0, 220, 220]
    # best_np alone, on given scores: the key's order
    cfg = S.ScanMatchConfig(nx=1, ny=1, nt=1, xy_step=1, theta_step=1, min_cells=0, min_mean=-100000)
    s = np.zeros(27, np.int64)
    s[[0, 26]] = 5                                              # two corners, d = 3 each
    assert S.best_np(s, cfg, 1, 0).tolist()[:5] == [S.EDGE, -1, -1, -1, 5]
    s[14] = 5                                                   # (ix, iy, it) = (2, 1, 1): d = 1
    assert S.best_np(s, cfg, 1, 0).tolist()[:5] == [S.EDGE, 1, 0, 0, 5]
    s[:] = -7
    assert S.best_np(s, cfg, 1, 0).tolist()[:6] == [0, 0, 0, 0, -7, -7]
    with pytest.raises(ValueError, match="27 candidates"):
        S.best_np(s[:26], cfg, 1, 0)


def test_every_status_bit_alone(pp, S):
    oc, L, known = K.blank(pp, 9, 7)
    known[:] = True
    rows, pose = K.rows_at(SCAN3), K.at(4.0, 3.0)
    quiet = dict(min_cells=0, min_mean=0)
    assert (S.NO_MAP, S.OUTSIDE, S.FEW_CELLS, S.LOW_SCORE, S.EDGE) == (1, 2, 4, 8, 16) and S.REJECT == 15
    words, scores = _match(S, oc, L + 50, known, None, rows, pose, **quiet)
    assert words.tolist() == [S.NO_MAP, 0, 0, 0, 0, 0, 3, 0] and not scores.any()
    for far in (K.at(9.0, 3.0), K.at(4.0, -0.001), K.at(-1e6, 3.0)):
        words, scores = _match(S, oc, L + 50, known, (0, 0), rows, far, **quiet)
        assert words.tolist() == [S.OUTSIDE, 0, 0, 0, 0, 0, 3, 0] and not scores.any()
    words, _ = _match(S, oc, L, known, (0, 0), rows, pose, min_cells=4, min_mean=0)
    assert words.tolist() == [S.FEW_CELLS, 0, 0, 0, 0, 0, 3, 0]
    assert _match(S, oc, L, known, (0, 0), rows, pose, min_cells=3, min_mean=0)[0][0] == 0
    words, _ = _match(S, oc, L + 9, known, (0, 0), rows, pose, min_cells=0, min_mean=901)      # 27 * 100 < 901 * 3
    assert words.tolist() == [S.LOW_SCORE, 0, 0, 0, 27, 27, 3, 0]
    assert _match(S, oc, L + 9, known, (0, 0), rows, pose, min_cells=0, min_mean=900)[0][0] == 0
    words, _ = _match(S, oc, L - 9, known, (0, 0), rows, pose, min_cells=0, min_mean=-900)      # a negative bound, met exactly
    assert words.tolist() == [0, 0, 0, 0, -27, -27, 3, 0]
    assert _match(S, oc, L - 10, known, (0, 0), rows, pose, min_cells=0, min_mean=-900)[0][0] == S.LOW_SCORE
    wall = L.copy()
    wall[4, 7] = 85                                              # the third scan cell's wall one cell to the right: (7, 4)
    words, _ = _match(S, oc, wall, known, (0, 0), rows, pose, **quiet)
    assert words.tolist() == [S.EDGE, 1, 0, 0, 85, 0, 3, 0]      # ((1, 1) reaches it too, through the second cell, at d = 2)
    words, _ = _match(S, oc, wall, known, (0, 0), rows, pose, nx=2, **quiet)
    assert words.tolist() == [0, 1, 0, 0, 85, 0, 3, 0]           # the same best, no longer on a face
    # an axis of half-width 0 has no face
    assert _match(S, oc, wall, known, (0, 0), rows, pose, nx=0, ny=0, **quiet)[0].tolist()[:4] == [0, 0, 0, 0]


def test_corrected_pose(pp, S):
    oc = pp.occupancy.OccupancyConfig(resolution=0.1, width=50, height=50)
    cfg = S.ScanMatchConfig(nx=4, ny=4, nt=4, xy_step=512, theta_step=8)
    prior = pp.sweeps.pose_from_xyyaw(1.25, -0.5, 0.3)
    prior[2, 3] = 0.77
    for bit in (S.NO_MAP, S.OUTSIDE, S.FEW_CELLS, S.LOW_SCORE, 15, S.EDGE | S.LOW_SCORE):
        out = S.corrected_pose(prior, [bit, 2, -1, 3, 0, 0, 0, 0], oc, cfg)
        assert np.array_equal(out, prior) and out is not prior
    for status in (0, S.EDGE):
        out = S.corrected_pose(prior, [status, 2, -1, 3, 0, 0, 0, 0], oc, cfg)
        a = 2.0 * math.pi * 24.0 / 4096.0
        Rz = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
        assert np.array_equal(out[:, :3], Rz @ prior[:, :3])
        assert out[:, 3].tolist() == [1.25 + 1024.0 * 0.1 / 1024.0, -0.5 + -512.0 * 0.1 / 1024.0, 0.77]
        assert np.array_equal(out[2], prior[2])
        want = pp.sweeps.pose_from_xyyaw(1.35, -0.55, 0.3 + a)
        assert np.abs(out[:, :3] - want[:, :3]).max() < 1e-15
    with pytest.raises(ValueError, match="8 words"):
        S.corrected_pose(prior, [0, 0, 0], oc, cfg)


def test_config_refusals_by_field_name(pp, S):
    C = S.ScanMatchConfig
    assert C().to_dict() == dict(nx=10, ny=10, nt=10, xy_step=1024, theta_step=8, min_cells=50, min_mean=0) and C().candidates == 9261
    assert C.from_any(True) == C() and C.from_any(C(nx=3)) == C(nx=3) and C.from_any({"nt": 0}).nt == 0
    assert C(nx=127, ny=127, nt=0).candidates == 65025 and C(min_mean=-100000).min_mean == -100000
    for field, bad in (("nx", 128), ("nx", -1), ("ny", 128), ("nt", -1), ("nt", 128), ("xy_step", 0), ("xy_step", 4097), ("theta_step", 0),
                       ("theta_step", 513), ("min_cells", -1), ("min_mean", 100001), ("min_mean", -100001)):
        with pytest.raises(ValueError, match=rf"ScanMatchConfig: {field} = {bad} outside"):
            C(**{field: bad})
    for field, bad in (("nx", 1.0), ("ny", True), ("nt", "2"), ("xy_step", None), ("min_mean", 0.5)):
        with pytest.raises(ValueError, match=rf"ScanMatchConfig: {field} must be an integer"):
            C(**{field: bad})
    with pytest.raises(ValueError, match=r"= 195075 candidates, at most PP_SCAN_MAX_CANDIDATES = 65536"):
        C(nx=127, ny=127, nt=1)
    with pytest.raises(ValueError, match=r"unknown keys \['nz'\]"):
        C.from_any({"nz": 1})
    with pytest.raises(ValueError, match="a ScanMatchConfig, a dict of its fields or True"):
        C.from_any(3)


# ---- recovery: a property of the rule ----
def test_recovery_in_the_l_shaped_room(pp, S):
    """Twelve fixed seeds; each displaces the prior of the sixth frame by whole steps, -3 .. 3 on every axis.  The
    restatement must land within one step of the truth on every axis in all twelve and exactly on it in at least nine.
    (Seeds 1000 .. 1011 of scan_match_cases.room_case: exact in twelve; over 1000 .. 1023 exact in 21 of 24, the other
    three one step off on one axis.)"""
    exact = 0
    for seed in K.ROOM_SEEDS:
        m, rows, prior, want = K.room_case(pp, seed)
        words, scores = S.match_np(m, rows, prior, K.ROOM_SCAN)
        got = tuple(int(v) for v in words[1:4])
        print(f"seed {seed}: truth {want}, found {got}, status {words[0]}, best {words[4]}, prior {words[5]}, scan cells {words[6]}")
        assert not words[0] & S.REJECT and words[6] >= 400
        assert all(abs(g - w) <= 1 for g, w in zip(got, want)), (seed, want, got)
        exact += got == want
        if got == want:
            # the corrected pose is the true one: the prior moved forward by the steps it was moved back by
            out = S.corrected_pose(prior, words, K.ROOM_OCC, K.ROOM_SCAN)
            step = 0.1
            assert abs(out[0, 3] - (prior[0, 3] + want[0] * step)) < 1e-12 and abs(out[1, 3] - (prior[1, 3] + want[1] * step)) < 1e-12
            yaw = math.atan2(out[1, 0], out[0, 0]) - math.atan2(prior[1, 0], prior[0, 0])
            assert abs((yaw + math.pi) % (2 * math.pi) - math.pi - want[2] * 8 * K.TICK) < 1e-12
    assert exact >= 9, exact
    assert len(K.ROOM_SEEDS) == 12 and K.ROOM_SCAN == dict(nx=4, ny=4, nt=4, xy_step=1024, theta_step=8, min_cells=50, min_mean=0)
    assert (K.ROOM_OCC["resolution"], K.ROOM_OCC["width"], K.ROOM_OCC["height"], K.ROOM_RETURNS, K.ROOM_NOISE) == (0.1, 200, 200, 6000, 0.01)


# ---- the C-ABI's structure ----
NEW = ["pp_set_scan_match", "pp_get_scan_match_config", "pp_scan_match_async", "pp_get_scan_match", "pp_scan_match_grids"]


def test_struct_header_exports_and_sources(pp, S):
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    csrc = os.path.join(os.path.dirname(pp._lib.__file__), "csrc")
    assert ctypes.sizeof(pp._lib.PPScanMatchConfig) == 32
    fields = re.findall(r"^\s+int32_t (\w+);", hdr[hdr.index("typedef struct pp_scan_match_config"):hdr.index("} pp_scan_match_config;")], re.M)
    assert [f[0] for f in pp._lib.PPScanMatchConfig._fields_] == fields == list(S.ScanMatchConfig().to_dict()) + ["reserved"]
    api = open(os.path.join(csrc, "api_scan_match.hip")).read()
    assert "static_assert(sizeof(pp_scan_match_config) == 32" in api and "static_assert(sizeof(ScanCall) == 64" in api
    for name, v in (("PP_SCAN_MAX_CANDIDATES", 65536), ("PP_SCAN_RESULT", 8)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr) and getattr(pp._lib, name) == v, name
    for name, v in (("NO_MAP", 1), ("OUTSIDE", 2), ("FEW_CELLS", 4), ("LOW_SCORE", 8), ("EDGE", 16)):
        assert re.search(r"PP_SCAN_%s = %d\b" % (name, v), hdr) and getattr(pp._lib, "PP_SCAN_" + name) == v == getattr(S, name), name
    assert len(S.WORDS) == 8 and (S.SUB, S.HEADINGS) == (pp._lib.PP_LOCAL_SUB, pp._lib.PP_LOCAL_HEADINGS) == (1024, 4096)
    assert "#define PP_ABI_VERSION 4" in hdr
    # the structs the stage was not to touch
    assert ctypes.sizeof(pp._lib.PPOccupancyConfig) == 56 and ctypes.sizeof(pp._lib.PPLocalPlanConfig) == 32
    common = open(os.path.join(csrc, "pp_common.h")).read()
    assert 'static_assert(sizeof(OccCall) == 96' in open(os.path.join(csrc, "occupancy.hip")).read() and "struct ScanCall" in common
    later = hdr[hdr.index("later additions within 4"):hdr.index("#define PP_ABI_VERSION")]
    for name in ["PP_SCAN_MAX_CANDIDATES", "PP_SCAN_RESULT", "pp_scan_status", "pp_scan_match_config"] + NEW:
        assert re.search(r"\b%s\b" % name, later), name
        assert later.index("pp_local_plan_grids_movers") < later.index(name)               # appended, nothing before them changed
    exp = pp._lib.EXPORTS
    at = exp.index("pp_local_plan_grids_movers")
    assert exp[at + 1:at + 6] == NEW
    for name in NEW[:-1]:
        assert re.search(r"\bint %s\(pp_handle" % name, hdr), name
    assert re.search(r"\bint pp_scan_match_grids\(int device", hdr)
    src = pp._lib.SOURCES
    at = src.index("local_movers.hip")
    assert src[at + 1:at + 3] == ["api_scan_match.hip", "scan_match.hip"] and src[-2:] == ["api_track.hip", "track.hip"]
    assert src[src.index("inflate.hip") + 1:src.index("inflate.hip") + 3] == ["api_navfn.hip", "navfn.hip"]
    assert src[src.index("navfn.hip") + 1:src.index("navfn.hip") + 4] == ["api_local_plan.hip", "local_plan.hip", "local_movers.hip"]
    for s in ("api_scan_match.hip", "scan_match.hip"):
        assert os.path.exists(os.path.join(csrc, s))
    assert "scan_match" in pp.__all__
    for name in ("scan_cells_np", "sensor_subcells", "score_np", "scores_np", "best_np", "match_grid_np", "match_np", "corrected_pose", "scan_match_grids"):
        assert callable(getattr(S, name)), name
    for name in ("set_scan_match", "scan_match_async", "scan_match_results", "scan_match_poses", "localize"):
        assert callable(getattr(pp.Engine, name)), name
    assert isinstance(pp.Engine.scan_match, property) and callable(pp.VoxelNet.localize)
    assert "scan_match_release(e);" in open(os.path.join(csrc, "pp_api.hip")).read()
    # opt-in at run time only, plain C++ on the hot path: no switch, no getenv, no floating-point atomic
    kern = open(os.path.join(csrc, "scan_match.hip")).read()
    assert "SCAN" not in open(os.path.join(csrc, "pp_switches.h")).read().upper()
    assert "getenv" not in kern and "asm" not in kern.replace("namespace", "") and "atomicAdd(float" not in kern
    assert "scan" not in open(os.path.join(csrc, "api_occupancy.hip")).read().lower()      # the occupancy stage knows nothing of it
    doc = re.sub(r"\s+", " ", S.__doc__)
    for what in ("multi-resolution branch and bound", "sub-cell refinement", "a covariance from the score volume", "loop closure",
                 "removing tracked objects' points from the scan", "any correction of roll, pitch or z", "L = 0 wherever a cell is not known"):
        assert what in doc, what


def test_exported_from_the_library_and_null_handle(pp, hip_lib):
    for name in NEW:
        assert hasattr(hip_lib, name), name
    PP_ERR_ARG = 1
    pc = pp._lib.PPScanMatchConfig(1, 1, 1, 1024, 8, 0, 0, 0)
    on = ctypes.c_int32(7)
    P = np.zeros((1, 3, 4))
    words = np.zeros((1, 8), np.int32)
    assert hip_lib.pp_set_scan_match(None, ctypes.byref(pc), None, 0) == PP_ERR_ARG
    assert hip_lib.pp_get_scan_match_config(None, ctypes.byref(on), None) == PP_ERR_ARG and on.value == 7
    assert hip_lib.pp_scan_match_async(None, P.ctypes.data, 1) == PP_ERR_ARG
    assert hip_lib.pp_get_scan_match(None, words.ctypes.data, None, 1) == PP_ERR_ARG
    # the stand-alone call refuses before it looks for a device
    assert hip_lib.pp_scan_match_grids(0, None, None, 1, 4, 4, None, None, 3, None, None, None, None, None, None, 0, None, None) == PP_ERR_ARG
    assert b"logodds, known, occ_cfg or cfg is NULL" in hip_lib.pp_last_error(None)


def test_stand_alone_refusals_without_a_device(pp, S):
    oc, L, known = K.blank(pp, 5, 4)
    rows = [K.rows_at([(0, 0)])]
    with pytest.raises(ValueError, match=r"must be \[B, 4, 5\]"):
        S.scan_match_grids(L[None, :3], known[None, :3], rows, K.IDENTITY[None], [(0, 0)], oc, True)
    with pytest.raises(ValueError, match="1 float32"):
        S.scan_match_grids(L[None], known[None], [rows[0].astype(np.float64)], K.IDENTITY[None], [(0, 0)], oc, True)
    with pytest.raises(ValueError, match="2 origin cells for 1 grids"):
        S.scan_match_grids(L[None], known[None], rows, K.IDENTITY[None], [(0, 0), None], oc, True)
