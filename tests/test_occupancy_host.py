"""occupancy.py, the rule of the rolling occupancy map, on hand-made cases with the expected cells written out (no GPU),
and the plumbing of the stage: struct, header, exports, sources, Engine methods."""
import ctypes
import dataclasses
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 15, 11                 # the sensor's cell is (7, 5)
X0, Y0 = W // 2, H // 2


@pytest.fixture(scope="module")
def O(pp):
    return pp.occupancy


def _cfg(O, **kw):
    return O.OccupancyConfig(**dict(dict(resolution=1.0, z_min=0.0, z_max=2.0, max_range=50.0, width=W, height=H), **kw))


def _pose(x=0.0, y=0.0):
    return np.array([[1.0, 0.0, 0.0, x], [0.0, 1.0, 0.0, y], [0.0, 0.0, 1.0, 0.0]])


def _at(cells, z=1.0):
    """Rows that end in the middle of the cells (dx, dy) away from the sensor's cell (pose at the origin)."""
    return np.array([[dx + 0.5, dy + 0.5, z] for dx, dy in cells], np.float32).reshape(-1, 3)


def _cells(mask):
    """The set of (dx, dy) offsets from the sensor's cell where a [H, W] mask holds."""
    iy, ix = np.nonzero(mask)
    return {(int(x) - X0, int(y) - Y0) for x, y in zip(ix, iy)}


# ---- rays ----
# target (offset from the sensor's cell) -> the cells its walk marks passed, in order
RAYS = {
    (5, 2): [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2)],
    (2, 5): [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4)],
    (-2, 5): [(0, 0), (0, 1), (-1, 2), (-1, 3), (-2, 4)],
    (-5, 2): [(0, 0), (-1, 0), (-2, 1), (-3, 1), (-4, 2)],
    (-5, -2): [(0, 0), (-1, 0), (-2, -1), (-3, -1), (-4, -2)],
    (-2, -5): [(0, 0), (0, -1), (-1, -2), (-1, -3), (-2, -4)],
    (2, -5): [(0, 0), (0, -1), (1, -2), (1, -3), (2, -4)],
    (5, -2): [(0, 0), (1, 0), (2, -1), (3, -1), (4, -2)],
    (4, 0): [(0, 0), (1, 0), (2, 0), (3, 0)],
    (0, -3): [(0, 0), (0, -1), (0, -2)],
    (-4, 0): [(0, 0), (-1, 0), (-2, 0), (-3, 0)],
    (0, 3): [(0, 0), (0, 1), (0, 2)],
    (3, 3): [(0, 0), (1, 1), (2, 2)],
    (-3, 3): [(0, 0), (-1, 1), (-2, 2)],
    (-3, -3): [(0, 0), (-1, -1), (-2, -2)],
    (3, -3): [(0, 0), (1, -1), (2, -2)],
    # two targets whose walk from the far end visits other cells: the direction is part of the rule
    (4, 1): [(0, 0), (1, 0), (2, 0), (3, 1)],
    (6, 3): [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)],
}


@pytest.mark.parametrize("target", sorted(RAYS))
def test_ray_cells_literal_and_through_update(O, target):
    want = RAYS[target]
    assert O.ray_cells(0, 0, *target) == want
    assert O.ray_cells(X0, Y0, X0 + target[0], Y0 + target[1]) == [(X0 + x, Y0 + y) for x, y in want]
    c = _cfg(O)
    m = O.OccupancyMap(c)
    info = m.update(_at([target]), _pose())
    L = m.logodds()
    assert _cells(L == c.l_hit) == {target} and _cells(L == -c.l_miss) == set(want)
    assert _cells(m.known()) == set(want) | {target}
    assert info == {"hits": 1, "ground": 0, "ignored": 0, "cells_hit": 1, "cells_free": len(want), "cleared": W * H}


def test_walk_direction_is_part_of_the_rule(O):
    far = {(4, 1): [(4, 1), (3, 1), (2, 1), (1, 0)], (6, 3): [(6, 3), (5, 3), (4, 2), (3, 2), (2, 1), (1, 1)]}
    for t, back in far.items():
        assert O.ray_cells(*t, 0, 0) == back
        assert set(back[1:]) != set(RAYS[t][1:])
    # (5, 2) is one of the 169 targets whose two walks agree
    assert set(O.ray_cells(5, 2, 0, 0)[1:]) == set(RAYS[(5, 2)][1:])
    n = 0
    for y in range(-7, 8):
        for x in range(-7, 8):
            fwd = set(O.ray_cells(0, 0, x, y)) | {(x, y)}
            rev = set(O.ray_cells(x, y, 0, 0)) | {(0, 0)}
            n += fwd != rev
    assert n == 56


def test_rays_stepped_together_equal_rays_walked_alone(O):
    rng = np.random.default_rng(3)
    ex, ey = rng.integers(0, 37, 200), rng.integers(0, 29, 200)
    want = np.zeros((29, 37), bool)
    for x, y in zip(ex, ey):
        for px, py in O.ray_cells(18, 14, int(x), int(y)):
            want[py, px] = True
    assert np.array_equal(O._passed_by_rays(ex, ey, 18, 14, (29, 37)), want)


def test_endpoint_in_the_sensors_own_cell(O):
    c = _cfg(O)
    m = O.OccupancyMap(c)
    info = m.update(_at([(0, 0)]), _pose())
    assert _cells(m.known()) == {(0, 0)} and m.logodds()[Y0, X0] == c.l_hit
    assert info["cells_hit"] == 1 and info["cells_free"] == 0
    g = O.OccupancyMap(c)
    g.update(_at([(0, 0)], z=-1.0), _pose())                   # a ground return there: its own cell is freed
    assert _cells(g.known()) == {(0, 0)} and g.logodds()[Y0, X0] == -c.l_miss


def test_hit_beats_pass_ground_frees_and_many_rows_are_one_step(O):
    c = _cfg(O)
    m = O.OccupancyMap(c)
    # (2, 0) is hit, and passed by the ray to (4, 0); (4, 0) takes 150 rows; (0, 3) is a ground return
    rows = np.concatenate([_at([(2, 0)]), _at([(4, 0)] * 150), _at([(0, 3)], z=-0.5)])
    info = m.update(rows, _pose())
    L = m.logodds()
    assert L[Y0, X0 + 2] == c.l_hit and L[Y0, X0 + 4] == c.l_hit
    assert L[Y0 + 3, X0] == -c.l_miss and m.known()[Y0 + 3, X0]
    assert _cells(L == -c.l_miss) == {(0, 0), (1, 0), (3, 0), (0, 1), (0, 2), (0, 3)}
    assert info == {"hits": 151, "ground": 1, "ignored": 0, "cells_hit": 2, "cells_free": 6, "cleared": W * H}
    # ground and hit in one cell: a hit
    m2 = O.OccupancyMap(c)
    m2.update(np.concatenate([_at([(3, 1)], z=-0.5), _at([(3, 1)])]), _pose())
    assert m2.logodds()[Y0 + 1, X0 + 3] == c.l_hit
    g = m.grid()
    t = O.cost_table(c)
    assert g[Y0, X0 + 2] == t[c.l_hit - c.l_min] and g[Y0, X0] == t[-c.l_miss - c.l_min] and g[0, 0] == -1
    assert (g == -1).sum() == W * H - 8


def test_z_band_range_and_non_finite_rows(O):
    c = _cfg(O, max_range=3.0)
    up = np.nextafter(np.float32(2.0), np.float32(3.0))
    beyond = np.nextafter(np.float32(3.0), np.float32(4.0))
    rows = np.array([
        [1.5, 0.5, 0.0],            # z == z_min: a hit
        [2.5, 0.5, 2.0],            # z == z_max: a hit
        [0.5, 1.5, up],             # just above z_max: ignored
        [0.5, 2.5, -1e-6],          # just below z_min: ground
        [3.0, 0.0, 1.0],            # range exactly max_range: used
        [0.0, beyond, 1.0],         # one float32 step beyond: ignored
        [np.nan, 0.5, 1.0], [0.5, np.nan, 1.0], [0.5, 0.5, np.nan],
        [np.inf, 0.5, 1.0], [0.5, -np.inf, 1.0], [0.5, 0.5, np.inf], [0.5, 0.5, -np.inf],
        [1e30, 0.5, 1.0], [0.5, -1e30, 1.0],
    ], np.float32)
    m = O.OccupancyMap(c)
    info = m.update(rows, _pose())
    assert info["hits"] == 3 and info["ground"] == 1 and info["ignored"] == 11
    assert _cells(m.logodds() == c.l_hit) == {(1, 0), (2, 0), (3, 0)}
    assert _cells(m.logodds() == -c.l_miss) == {(0, 0), (0, 1), (0, 2)}
    # one cell outside each window edge (and the cells just inside)
    w = O.OccupancyMap(_cfg(O))
    out = [(-X0 - 1, 0), (W - X0, 0), (0, -Y0 - 1), (0, H - Y0)]
    inside = [(-X0, 0), (W - X0 - 1, 0), (0, -Y0), (0, H - Y0 - 1)]
    info = w.update(_at(out + inside), _pose())
    assert info["ignored"] == 4 and info["hits"] == 4 and _cells(w.logodds() == 85) == set(inside)
    with pytest.raises(ValueError, match="float32"):
        w.update(np.zeros((2, 3)), _pose())


def test_saturation_at_both_clamps(O):
    c = _cfg(O)
    m = O.OccupancyMap(c)
    n_hit, n_miss = math.ceil(c.l_max / c.l_hit) + 2, math.ceil(-c.l_min / c.l_miss) + 2
    for k in range(max(n_hit, n_miss)):
        m.update(_at([(3, 0)]), _pose())
        L = m.logodds()
        assert L[Y0, X0 + 3] == min((k + 1) * c.l_hit, c.l_max) and L[Y0, X0 + 1] == max(-(k + 1) * c.l_miss, c.l_min)
    assert L[Y0, X0 + 3] == c.l_max == 350 and L[Y0, X0 + 1] == c.l_min == -200
    assert m.grid()[Y0, X0 + 3] == 97 and m.grid()[Y0, X0 + 1] == 12


def _seeded_map(O, c, at=(0.0, 0.0)):
    rng = np.random.default_rng(5)
    m = O.OccupancyMap(c)
    for _ in range(3):
        m.update(np.concatenate([rng.uniform(-7, 7, (40, 2)), rng.uniform(-1, 2, (40, 1))], 1).astype(np.float32), _pose(*at))
    return m


@pytest.mark.parametrize("shift", [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (2, -3), (W - 1, 0), (W, 0), (W + 5, 0),
                                   (0, H - 1), (0, H), (-3, -(H + 2))])
def test_shift_keeps_the_overlap_bit_for_bit(O, shift):
    c = _cfg(O)
    m = _seeded_map(O, c)
    L0, K0 = m.logodds(), m.known()
    assert K0.sum() > 40 and m.origin_cell == (-X0, -Y0)
    sx, sy = shift
    info = m.update(np.zeros((0, 3), np.float32), _pose(float(sx) + 0.25, float(sy) + 0.25))
    assert m.origin_cell == (sx - X0, sy - Y0)
    L1, K1 = m.logodds(), m.known()
    kept = 0
    for iy in range(H):
        for ix in range(W):
            ox, oy = ix + sx, iy + sy                     # the same global cell in the old window
            if 0 <= ox < W and 0 <= oy < H:
                kept += 1
                assert L1[iy, ix] == L0[oy, ox] and K1[iy, ix] == K0[oy, ox]
            else:
                assert L1[iy, ix] == 0 and not K1[iy, ix]
    assert info["cleared"] == W * H - kept
    if abs(sx) >= W or abs(sy) >= H:
        assert kept == 0 and not K1.any() and (m.grid() == -1).all()


def test_a_cell_that_leaves_and_re_enters_is_unknown(O):
    c = _cfg(O)
    m = O.OccupancyMap(c)
    m.update(_at([(-X0, 0)]), _pose())                        # the window's left edge
    assert m.known()[Y0, 0]
    m.update(np.zeros((0, 3), np.float32), _pose(1.0, 0.0))     # it leaves
    m.update(np.zeros((0, 3), np.float32), _pose(0.0, 0.0))     # and is back
    assert not m.known()[Y0, 0] and m.logodds()[Y0, 0] == 0
    assert m.known()[Y0, 1:X0 + 1].all()                      # the rest of the ray stayed


def test_origin_floors_negative_translations(O):
    c = _cfg(O, resolution=0.25)
    m = O.OccupancyMap(c)
    assert m.origin is None and m.origin_cell is None
    m.update(np.zeros((0, 3), np.float32), _pose(-0.1, -1.0))
    assert m.origin_cell == (-1 - X0, -4 - Y0) and m.origin == ((-1 - X0) * 0.25, (-4 - Y0) * 0.25)
    assert O.window_origin(c, _pose(0.26, -0.26)) == (1 - X0, -2 - Y0)
    m.reset()
    assert m.origin is None and not m.known().any()
    with pytest.raises(ValueError, match="2\\^30"):
        O.window_origin(c, _pose(0.25 * 2 ** 30, 0.0))
    assert O.window_origin(c, _pose(0.25 * (2 ** 30 - 1), 0.0))[0] == 2 ** 30 - 1 - X0
    with pytest.raises(ValueError, match="2\\^30"):
        m.update(np.zeros((0, 3), np.float32), _pose(0.0, -0.25 * 2 ** 30))
    with pytest.raises(ValueError, match="orthonormal"):
        m.update(np.zeros((0, 3), np.float32), 2.0 * _pose())
    assert m.origin is None


def test_rotated_pose_uses_rows_0_and_1(O, pp):
    c = _cfg(O)
    m = O.OccupancyMap(c)
    P = pp.sweeps.pose_from_xyyaw(2.0, -1.0, math.pi / 2)     # sensor x -> fixed y
    m.update(np.array([[3.5, 0.2, 1.0]], np.float32), P)
    assert m.origin_cell == (2 - X0, -1 - Y0)
    # fixed (2 - 0.2, -1 + 3.5) = (1.8, 2.5): global cell (1, 2), window cell (1 - 2 + 7, 2 + 1 + 5)
    assert _cells(m.logodds() == c.l_hit) == {(-1, 3)}


def test_cost_table(O):
    c = O.OccupancyConfig()
    t = O.cost_table(c)
    assert t.dtype == np.int8 and t.shape == (c.l_max - c.l_min + 1,)
    assert t[0] == 12 and t[-1] == 97 and t[-c.l_min] == 50
    assert (np.diff(t.astype(int)) >= 0).all()
    full = O.cost_table(O.OccupancyConfig(l_min=-1000, l_max=1000))
    assert full.shape == (2001,) and full[0] == 0 and full[-1] == 100 and full[1000] == 50
    assert O.OccupancyConfig.from_probabilities() == c
    assert O.OccupancyConfig.from_probabilities(0.8, 0.3, 0.05, 0.99, width=10).to_dict() == dict(
        c.to_dict(), l_hit=139, l_miss=85, l_min=-294, l_max=460, width=10)
    with pytest.raises(ValueError, match="p_hit"):
        O.OccupancyConfig.from_probabilities(p_hit=1.0)


def test_config_validation_names_the_field(O):
    for kw, field in [(dict(resolution=0.0), "resolution"), (dict(resolution=float("nan")), "resolution"),
                      (dict(resolution="a"), "resolution"), (dict(max_range=0.0), "max_range"),
                      (dict(max_range=float("inf")), "max_range"), (dict(z_min=1.0, z_max=0.0), "z_min"),
                      (dict(z_max=float("nan")), "z_max"), (dict(width=0), "width"), (dict(height=0), "height"),
                      (dict(width=1.5), "width"), (dict(width=True), "width"), (dict(width=2048, height=1024), "width \\* height"),
                      (dict(l_hit=0), "l_hit"), (dict(l_hit=1001), "l_hit"), (dict(l_miss=0), "l_miss"), (dict(l_miss=-41), "l_miss"),
                      (dict(l_min=0), "l_min"), (dict(l_min=-1001), "l_min"), (dict(l_max=0), "l_max"), (dict(l_max=1001), "l_max")]:
        with pytest.raises(ValueError, match=field):
            O.OccupancyConfig(**kw)
    assert O.OccupancyConfig(width=1024, height=1024).width == 1024
    assert O.OccupancyConfig(z_min=float("-inf"), z_max=float("inf")).z_max == float("inf")
    with pytest.raises(ValueError, match="rezolution"):
        O.OccupancyConfig.from_any({"rezolution": 0.1})
    with pytest.raises(ValueError, match="occupancy"):
        O.OccupancyConfig.from_any(3)
    assert O.OccupancyConfig.from_any(True) == O.OccupancyConfig()
    d = O.OccupancyConfig(width=37).to_dict()
    assert O.OccupancyConfig.from_any(d).to_dict() == d and d["l_hit"] == 85 and d["l_miss"] == 41


def test_to_occupancy_grid_fields(O):
    c = _cfg(O, resolution=0.25)
    m = O.OccupancyMap(c)
    m.update(np.array([[0.6, 0.1, 1.0]], np.float32), _pose(-0.1, -1.0))
    msg = O.to_occupancy_grid(m.grid(), m.origin, c, stamp=12.5, frame_id="odom")
    assert msg["header"] == {"stamp": 12.5, "frame_id": "odom"}
    info = msg["info"]
    assert info["width"] == W and info["height"] == H and info["resolution"] == np.float32(0.25)
    assert info["origin"]["position"] == {"x": (-1 - X0) * 0.25, "y": (-4 - Y0) * 0.25, "z": 0.0}
    assert info["origin"]["orientation"] == {"x": 0.0, "y": 0.0, "z": 0.0, "w": 1.0}
    data = np.asarray(msg["data"])
    assert data.dtype == np.int8 and data.shape == (W * H,)
    assert data[Y0 * W + X0] == m.grid()[Y0, X0] != -1       # row-major, data[iy * width + ix]
    assert O.to_occupancy_grid(m.grid(), m.origin, c)["header"] == {"stamp": None, "frame_id": ""}
    with pytest.raises(ValueError, match="grid must be"):
        O.to_occupancy_grid(m.grid()[:3], m.origin, c)
    with pytest.raises(ValueError, match="origin"):
        O.to_occupancy_grid(m.grid(), (0.0, 0.0, 0.0), c)


# ---- structure ----
NEW = ["pp_set_occupancy", "pp_get_occupancy_config", "pp_occupancy_update_async", "pp_get_occupancy", "pp_occupancy_info",
       "pp_occupancy_reset"]


def test_struct_size_header_exports_and_sources(pp, O):
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    body = re.search(r"typedef struct pp_occupancy_config \{(.*?)\} pp_occupancy_config;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(double|int32_t)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in pp._lib.PPOccupancyConfig._fields_]
    assert [n for _, n in fields] == [f.name for f in dataclasses.fields(O.OccupancyConfig)]
    kinds = [t for t, _ in fields]
    assert kinds == sorted(kinds)                             # the doubles first
    size = sum(8 if t == "double" else 4 for t in kinds)
    assert size == ctypes.sizeof(pp._lib.PPOccupancyConfig) == 56
    csrc = os.path.join(os.path.dirname(pp._lib.__file__), "csrc")
    assert "static_assert(sizeof(pp_occupancy_config) == 56" in open(os.path.join(csrc, "api_occupancy.hip")).read()
    assert re.search(r"#define PP_OCC_MAX_CELLS 1048576\b", hdr)
    assert pp._lib.PP_OCC_MAX_CELLS == O.PP_OCC_MAX_CELLS == 1048576
    assert "#define PP_ABI_VERSION 4" in hdr
    later = hdr[hdr.index("later additions within 4"):hdr.index("#define PP_ABI_VERSION")]
    for name in ["PP_OCC_MAX_CELLS", "pp_occupancy_config"] + NEW:
        assert re.search(r"\b%s\b" % name, later), name
    exp = pp._lib.EXPORTS
    for name in NEW:
        assert name in exp and re.search(r"\bint %s\(pp_handle" % name, hdr), name
        assert exp.index(name) < exp.index("pp_soft_nms")
    src = pp._lib.SOURCES
    for s in ("api_occupancy.hip", "occupancy.hip"):
        assert s in src and os.path.exists(os.path.join(csrc, s))
        assert src.index(s) < src.index("api_track.hip")
    assert src[-2:] == ["api_track.hip", "track.hip"]
    assert "occupancy" in pp.__all__
    for name in ("OccupancyConfig", "OccupancyMap", "cost_table", "ray_cells", "window_origin", "to_occupancy_grid"):
        assert hasattr(O, name)
    for name in ("set_occupancy", "occupancy_update_async", "occupancy_maps", "occupancy_info", "occupancy_reset"):
        assert callable(getattr(pp.Engine, name))
    assert isinstance(pp.Engine.occupancy, property)
    assert callable(pp.VoxelNet.occupancy_update) and callable(pp.VoxelNet.occupancy_maps)


def test_exported_from_the_library_and_null_handle(pp, hip_lib):
    for name in NEW:
        assert hasattr(hip_lib, name), name
    PP_ERR_ARG = 1
    c = pp._lib.PPOccupancyConfig()
    assert hip_lib.pp_set_occupancy(None, ctypes.byref(c), None, 0) == PP_ERR_ARG
    assert hip_lib.pp_set_occupancy(None, None, None, 0) == PP_ERR_ARG
    assert hip_lib.pp_occupancy_update_async(None, None, 1) == PP_ERR_ARG
    assert hip_lib.pp_occupancy_reset(None, -1) == PP_ERR_ARG
