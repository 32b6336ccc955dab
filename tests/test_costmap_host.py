"""costmap.py, the host restatement of the obstacle costmap (the GPU stage is held to it byte for byte in
tests/test_gpu_costmap.py).  The reference has no such path, so the restatement is held to hand-made frames whose cells are
known by construction, and its footprint rule to the package's existing point-in-box rule (gt_database.build_objects_np)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def C(pp):
    return pp.costmap


def _cfg(C, **kw):
    base = dict(x_min=0.0, y_min=0.0, resolution=1.0, width=5, height=4, z_min=0.0, z_max=1.0)
    base.update(kw)
    return C.CostmapConfig(**base)


def _pts(rows):
    return np.array(rows, np.float32).reshape(-1, 3)


def _tracks(pp, rows):
    """rows: (x, y, vx, vy, w, l, yaw, confirmed) -> TRACK_DTYPE rows."""
    t = np.zeros(len(rows), pp.tracking.TRACK_DTYPE)
    for i, r in enumerate(rows):
        t["state"][i, [0, 1, 3, 4]] = r[:4]
        t["size"][i] = (r[4], r[5], 1.5)
        t["yaw"][i] = r[6]
        t["confirmed"][i] = r[7]
        t["id"][i] = i + 1
    return t


def _dets(pp, rows):
    """rows: (x, y, w, l, yaw, score) -> DET_DTYPE rows."""
    d = np.zeros(len(rows), pp.Engine.det_dtype())
    for i, r in enumerate(rows):
        d["box3d_lidar"][i] = (r[0], r[1], 0.0, r[2], r[3], 1.5, r[4])
        d["score"][i] = r[5]
    return d


# ---- the point layer ----
def test_points_on_cell_edges_grid_edges_and_z_bounds(C):
    c = _cfg(C)
    pts = _pts([[1.0, 2.0, 0.5],          # exactly on the edge between cells: belongs to the upper cell (1, 2)
                [0.0, 0.0, 0.0],          # the lower grid edge (fx == 0) and z == z_min: in, counted
                [4.5, 3.5, 1.0],          # z == z_max: counted
                [5.0, 1.0, 0.5],          # the upper grid edge (ix == width): out
                [1.0, 4.0, 0.5],          # ... in y
                [-1e-7, 1.0, 0.5],        # just under the lower edge: out
                [2.5, 1.5, 1.5],          # above z_max: observed, not counted
                [2.5, 1.5, -0.5],         # under z_min: observed, not counted
                [np.nan, 1.0, 0.5], [1.0, np.inf, 0.5], [-np.inf, 1.0, 0.5],      # fall out
                [3.5, 0.5, np.nan]])      # in the grid, z fails both comparisons: observed only
    grid, counts = C.costmap_np(pts, c)
    want_counts = np.zeros((4, 5), np.int32)
    want_counts[2, 1] = want_counts[0, 0] = want_counts[3, 4] = 1
    want = np.full((4, 5), -1, np.int8)
    want[2, 1] = want[0, 0] = want[3, 4] = 100
    want[1, 2] = want[0, 3] = 0
    assert np.array_equal(counts, want_counts) and np.array_equal(grid, want)
    assert grid.dtype == np.int8 and counts.dtype == np.int32
    # further feature columns are ignored
    wide = np.concatenate([pts, np.full((len(pts), 2), 7.0, np.float32)], axis=1)
    g2, c2 = C.costmap_np(wide, c)
    assert np.array_equal(g2, grid) and np.array_equal(c2, counts)
    # nothing touches an empty frame
    g0, c0 = C.costmap_np(np.zeros((0, 3), np.float32), c)
    assert (g0 == -1).all() and (c0 == 0).all()


def test_min_points_threshold(C):
    c = _cfg(C, min_points=3, point_cost=77)
    pts = _pts([[0.5, 0.5, 0.5]] * 2 + [[1.5, 0.5, 0.5]] * 3)
    grid, counts = C.costmap_np(pts, c)
    assert counts[0, 0] == 2 and counts[0, 1] == 3
    assert grid[0, 0] == 0 and grid[0, 1] == 77           # count == min_points - 1: free; count == min_points: an obstacle


# ---- the object layer ----
def test_axis_aligned_box_covers_the_listed_cells(pp, C):
    c = _cfg(C, width=6, height=6, objects="tracks", object_cost=90)
    # centre (3, 2), w = 2 along x, l = 4 along y at yaw 0: |dx| <= 1, |dy| <= 2 -> centres 2.5, 3.5 in x; 0.5 .. 3.5 in y
    tr = _tracks(pp, [(3.0, 2.0, 0, 0, 2.0, 4.0, 0.0, 1)])
    grid, _ = C.costmap_np(np.zeros((0, 3), np.float32), c, tracks=tr, n_tracks=1)
    want = np.full((6, 6), -1, np.int8)
    want[0:4, 2:4] = 90
    assert np.array_equal(grid, want)
    assert C.decision_margins(c, C.footprints_np(c, tracks=tr)).min() == 0.5      # every centre half a cell from an edge
    # pad widens both half extents: 0.5 more reaches the next centres on every side
    grid, _ = C.costmap_np(np.zeros((0, 3), np.float32), _cfg(C, width=6, height=6, objects=2, object_cost=90, pad=0.5),
                           tracks=tr, n_tracks=1)
    want[0:5, 1:5] = 90
    assert np.array_equal(grid, want)


def test_yawed_box_covers_the_listed_cells(pp, C):
    # centre (3, 3), w = 1 (half 0.5) along local x, l = 4 (half 2) along local y, yaw 30 degrees.  Local y maps to the
    # world direction (sin r, cos r) = (0.5, 0.866): the long axis leans towards +x as y grows.
    c = _cfg(C, width=6, height=6, objects=2)
    tr = _tracks(pp, [(3.0, 3.0, 0, 0, 1.0, 4.0, math.radians(30.0), 1)])
    grid, _ = C.costmap_np(np.zeros((0, 3), np.float32), c, tracks=tr, n_tracks=1)
    # by hand, with d = centre - (3, 3), u = 0.866 dx - 0.5 dy (|u| <= 0.5), v = 0.5 dx + 0.866 dy (|v| <= 2):
    #   dy = -2.5: |u| <= 0.5 needs dx in [-2.02, -0.87] -> dx = -1.5, v = -2.92: out
    #   dy = -1.5: dx in [-1.44, -0.29] -> dx = -0.5 (ix 2), v = -1.55: in
    #   dy = -0.5: dx in [-0.87, 0.29] -> dx = -0.5 (ix 2), v = -0.68: in
    #   dy = +0.5: dx in [-0.29, 0.87] -> dx = +0.5 (ix 3), v = 0.68: in
    #   dy = +1.5: dx in [0.29, 1.44] -> dx = +0.5 (ix 3), v = 1.55: in
    #   dy = +2.5: dx in [0.87, 2.02] -> dx = +1.5, v = 2.92: out
    covered = {(1, 2), (2, 2), (3, 3), (4, 3)}          # (iy, ix)
    assert {(int(a), int(b)) for a, b in zip(*np.nonzero(grid == 100))} == covered
    assert (grid[grid != 100] == -1).all()


@pytest.mark.parametrize("yaw", [0.0, 0.5, -1.1, 2.0, math.pi / 2])
def test_footprint_is_the_package_point_in_box_rule(pp, C, yaw):
    """pad = 0: the cells of a footprint are the cell centres gt_database.build_objects_np puts inside the lidar box (its
    faces are open, so centres within 1e-9 of an edge are left out of the comparison).  This pins the yaw sign."""
    c = _cfg(C, x_min=-5.0, y_min=-5.0, resolution=0.25, width=40, height=40, objects=2)
    box = np.array([[0.3, -0.2, 0.0, 2.0, 4.0, 1.5, yaw]])
    tr = _tracks(pp, [(0.3, -0.2, 0, 0, 2.0, 4.0, yaw, 1)])
    grid, _ = C.costmap_np(np.zeros((0, 3), np.float32), c, tracks=tr, n_tracks=1)
    cx = -5.0 + (np.arange(40) + 0.5) * 0.25
    X, Y = np.meshgrid(cx, cx)
    P = np.stack([X.ravel(), Y.ravel(), np.full(1600, 0.75)], 1).astype(np.float32)       # mid height
    n, d = pp.augment.box_planes(box)
    inside = (pp.augment.face_sign(P[:, :3].astype(np.float64), n, d) < 0).all(-1)[:, 0].reshape(40, 40)
    counts, _ = pp.gt_database.build_objects_np(P, box)
    assert counts[0] == inside.sum() > 100
    decided = C.decision_margins(c, C.footprints_np(c, tracks=tr)) >= 1e-9
    assert np.array_equal((grid == 100)[decided], inside[decided])
    assert (~decided).sum() <= (40 if yaw in (0.0, math.pi / 2) else 0)


def test_max_rule_between_layers_and_unknown_against_free(pp, C):
    c = _cfg(C, width=6, height=6, objects=2, point_cost=60, object_cost=40)
    tr = _tracks(pp, [(3.0, 2.0, 0, 0, 2.0, 4.0, 0.0, 1)])           # covers [0:4, 2:4]
    pts = _pts([[2.5, 0.5, 0.5],            # an obstacle point inside the footprint: max(60, 40)
                [2.5, 1.5, 5.0],            # an observed, uncounted point inside the footprint: max(0, 40)
                [0.5, 0.5, 0.5],            # an obstacle point outside
                [0.5, 1.5, 5.0]])           # observed only: free
    grid, _ = C.costmap_np(pts, c, tracks=tr, n_tracks=1)
    assert grid[0, 2] == 60 and grid[1, 2] == 40 and grid[0, 0] == 60 and grid[1, 0] == 0
    assert grid[3, 3] == 40 and grid[5, 5] == -1
    # a footprint of cost 0 over an unknown cell makes it 0; over an obstacle it changes nothing
    c0 = _cfg(C, width=6, height=6, objects=2, point_cost=60, object_cost=0)
    grid, _ = C.costmap_np(pts, c0, tracks=tr, n_tracks=1)
    assert grid[0, 2] == 60 and grid[3, 3] == 0 and grid[5, 5] == -1
    # two footprints over one cell: the larger cost
    c2 = _cfg(C, width=6, height=6, objects=2, object_cost=30, horizon_steps=1, horizon_dt=1.0, predict_cost=[80])
    tr2 = _tracks(pp, [(3.0, 2.0, 1.0, 0.0, 2.0, 4.0, 0.0, 1)])      # predicted: [0:4, 3:5]
    grid, _ = C.costmap_np(np.zeros((0, 3), np.float32), c2, tracks=tr2, n_tracks=1)
    assert grid[0, 2] == 30 and grid[0, 3] == 80 and grid[0, 4] == 80 and grid[0, 5] == -1


def test_predicted_footprints_sit_at_t_k(pp, C):
    tr = _tracks(pp, [(1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 0.3, 1)])
    c = _cfg(C, objects=2, horizon_steps=3, horizon_dt=0.25, predict_cost=[70, 50, 30], object_cost=99)
    fp = C.footprints_np(c, tracks=tr, n_tracks=1)
    assert fp.shape == (4, 7)
    assert fp[:, 0].tolist() == [1.0, 1.5, 2.0, 2.5] and fp[:, 1].tolist() == [1.0, 1.25, 1.5, 1.75]
    assert fp[:, 6].tolist() == [99.0, 70.0, 50.0, 30.0]
    assert (fp[:, 2] == math.cos(0.3)).all() and (fp[:, 3] == math.sin(0.3)).all()
    assert (fp[:, 4] == 0.5).all() and (fp[:, 5] == 0.5).all()
    # horizon_steps = 0: the current footprints alone
    c0 = _cfg(C, objects=2, horizon_steps=0, object_cost=99)
    assert np.array_equal(C.footprints_np(c0, tracks=tr, n_tracks=1), fp[:1])
    g0, _ = C.costmap_np(np.zeros((0, 3), np.float32), c0, tracks=tr, n_tracks=1)
    g3, _ = C.costmap_np(np.zeros((0, 3), np.float32), c, tracks=tr, n_tracks=1)
    assert np.array_equal(g3 == 99, g0 == 99) and (g3 == 70).any() and not (g0 == 70).any()
    # entries of predict_cost past horizon_steps are ignored, also invalid ones
    C.CostmapConfig(horizon_steps=1, predict_cost=[10, 500])


def test_confirmed_only_min_score_and_non_finite_fields(pp, C):
    tr = _tracks(pp, [(1.5, 1.5, 0, 0, 1.0, 1.0, 0.0, 1), (3.5, 1.5, 0, 0, 1.0, 1.0, 0.0, 0),
                      (np.nan, 1.5, 0, 0, 1.0, 1.0, 0.0, 1), (2.5, 2.5, 0, 0, 1.0, 1.0, np.inf, 1)])
    assert len(C.footprints_np(_cfg(C, objects=2), tracks=tr)) == 2          # the non-finite ones cover nothing
    assert len(C.footprints_np(_cfg(C, objects=2, confirmed_only=True), tracks=tr)) == 1
    assert len(C.footprints_np(_cfg(C, objects=2), tracks=tr, n_tracks=1)) == 1   # rows behind the count are not read
    grid, _ = C.costmap_np(np.zeros((0, 3), np.float32), _cfg(C, objects=2, confirmed_only=1), tracks=tr)
    assert grid[1, 1] == 100 and (grid == 100).sum() == 1
    # a predicted footprint with a non-finite velocity falls out, the current one stays
    tv = _tracks(pp, [(1.5, 1.5, np.nan, 0, 1.0, 1.0, 0.0, 1)])
    assert len(C.footprints_np(_cfg(C, objects=2, horizon_steps=2), tracks=tv)) == 1
    d = _dets(pp, [(1.5, 1.5, 1.0, 1.0, 0.0, 0.5), (3.5, 1.5, 1.0, 1.0, 0.0, 0.25), (2.5, 2.5, 1.0, 1.0, 0.0, 0.1)])
    c = _cfg(C, objects="detections", min_score=0.25, object_cost=55)
    grid, _ = C.costmap_np(np.zeros((0, 3), np.float32), c, dets=d, n_dets=3)
    assert grid[1, 1] == 55 and grid[1, 3] == 55 and grid[2, 2] == -1        # score >= min_score: the bound is inclusive
    assert len(C.footprints_np(c, dets=d, n_dets=1)) == 1
    with pytest.raises(ValueError, match="needs dets"):
        C.footprints_np(c)
    with pytest.raises(ValueError, match="needs tracks"):
        C.footprints_np(_cfg(C, objects=2))
    # objects = none: the rows are not looked at
    grid, _ = C.costmap_np(np.zeros((0, 3), np.float32), _cfg(C), dets=d, n_dets=3)
    assert (grid == -1).all()


# ---- refusals ----
REFUSED = [("resolution", 0.0), ("resolution", -1.0), ("resolution", float("nan")), ("resolution", float("inf")),
           ("x_min", float("nan")), ("y_min", float("inf")), ("z_min", float("nan")), ("z_max", float("nan")),
           ("pad", -0.1), ("pad", float("inf")), ("min_score", float("nan")), ("horizon_dt", 0.0), ("horizon_dt", float("nan")),
           ("width", 0), ("height", 0), ("width", 1.5), ("min_points", 0), ("objects", 3), ("objects", -1),
           ("objects", "boxes"), ("confirmed_only", 2), ("horizon_steps", -1), ("horizon_steps", 9), ("point_cost", 101),
           ("point_cost", -1), ("object_cost", 101), ("object_cost", -1), ("x_min", "left"), ("width", True)]


@pytest.mark.parametrize("field,value", REFUSED)
def test_config_refusals_name_the_field(C, field, value):
    with pytest.raises(ValueError, match=field):
        C.CostmapConfig(**{field: value})


def test_config_refusals_of_combinations(C):
    with pytest.raises(ValueError, match="width \\* height"):
        C.CostmapConfig(width=513, height=512)
    C.CostmapConfig(width=512, height=512)
    with pytest.raises(ValueError, match="z_min"):
        C.CostmapConfig(z_min=1.0, z_max=0.0)
    with pytest.raises(ValueError, match=r"predict_cost\[1\]"):
        C.CostmapConfig(horizon_steps=2, predict_cost=[10, 101])
    with pytest.raises(ValueError, match=r"predict_cost\[0\]"):
        C.CostmapConfig(horizon_steps=1, predict_cost=[-1])
    with pytest.raises(ValueError, match="predict_cost"):
        C.CostmapConfig(horizon_steps=3, predict_cost=[10, 20])
    with pytest.raises(ValueError, match="predict_cost"):
        C.CostmapConfig(predict_cost=[1] * 9)
    with pytest.raises(ValueError, match="predict_cost"):
        C.CostmapConfig(predict_cost=5)
    with pytest.raises(ValueError, match="rezolution"):
        C.CostmapConfig.from_any({"rezolution": 0.1})
    with pytest.raises(ValueError, match="costmap"):
        C.CostmapConfig.from_any(3)
    assert C.CostmapConfig.from_any(True) == C.CostmapConfig()
    assert C.CostmapConfig(objects="tracks").objects == 2 and C.CostmapConfig(confirmed_only=True).confirmed_only == 1
    assert C.CostmapConfig(predict_cost=[5]).predict_cost == (5, 0, 0, 0, 0, 0, 0, 0)
    assert C.CostmapConfig(z_min=float("-inf"), z_max=float("inf")).z_max == float("inf")
    with pytest.raises(ValueError, match="float32"):
        C.costmap_np(np.zeros((3, 3)), C.CostmapConfig())


# ---- structure ----
NEW = ["pp_set_costmap", "pp_get_costmap_config", "pp_costmap_async", "pp_get_costmaps", "pp_costmap_info"]


def test_struct_size_header_exports_and_sources(pp, C):
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    body = re.search(r"typedef struct pp_costmap_config \{(.*?)\} pp_costmap_config;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(double|int32_t)\s+(\w+)(\[\w+\])?;", body)
    assert [n for _, n, _ in fields] == [n for n, _ in pp._lib.PPCostmapConfig._fields_]
    assert [n for _, n, _ in fields] == [f.name for f in __import__("dataclasses").fields(C.CostmapConfig)]
    size = sum((8 if t == "double" else 4) * (8 if arr else 1) for t, _, arr in fields)
    assert size == ctypes.sizeof(pp._lib.PPCostmapConfig) == 128
    csrc = os.path.join(os.path.dirname(pp._lib.__file__), "csrc")
    assert "static_assert(sizeof(pp_costmap_config) == 128" in open(os.path.join(csrc, "api_costmap.hip")).read()
    assert re.search(r"#define PP_COSTMAP_MAX_STEPS 8\b", hdr) and pp._lib.PP_COSTMAP_MAX_STEPS == C.PP_COSTMAP_MAX_STEPS == 8
    assert re.search(r"#define PP_COSTMAP_MAX_CELLS 262144\b", hdr)
    assert pp._lib.PP_COSTMAP_MAX_CELLS == C.PP_COSTMAP_MAX_CELLS == 262144
    assert "#define PP_ABI_VERSION 4" in hdr
    later = hdr[hdr.index("later additions within 4"):hdr.index("#define PP_ABI_VERSION")]
    for name in ["PP_COSTMAP_MAX_STEPS", "PP_COSTMAP_MAX_CELLS", "pp_costmap_config"] + NEW:
        assert re.search(r"\b%s\b" % name, later), name
    for name in NEW:
        assert name in pp._lib.EXPORTS and re.search(r"\bint %s\(pp_handle" % name, hdr), name
    src = pp._lib.SOURCES
    for s in ("api_costmap.hip", "costmap.hip"):
        assert s in src and os.path.exists(os.path.join(csrc, s))
    assert "costmap" in pp.__all__
    for name in ("CostmapConfig", "costmap_np", "footprints_np", "decision_margins", "to_occupancy_grid"):
        assert hasattr(C, name)
    for name in ("set_costmap", "costmap_async", "costmaps", "costmap_info"):
        assert callable(getattr(pp.Engine, name))
    assert isinstance(pp.Engine.costmap, property)
    assert callable(pp.VoxelNet.costmaps)


def test_exported_from_the_library(hip_lib):
    for name in NEW:
        assert hasattr(hip_lib, name), name


def test_config_key_round_trips(pp, C):
    cfg = pp.config.tiny_config(1)
    assert pp.config.Derived(cfg).costmap is None
    cfg["model"]["second"]["costmap"] = False
    assert pp.config.Derived(cfg).costmap is None
    cfg["model"]["second"]["costmap"] = True
    assert pp.config.Derived(cfg).costmap == C.CostmapConfig().to_dict()
    cfg["model"]["second"]["costmap"] = {"resolution": 0.1, "objects": "tracks", "horizon_steps": 2, "predict_cost": [50, 25]}
    d = pp.config.Derived(cfg)
    assert d.costmap == dict(C.CostmapConfig().to_dict(), resolution=0.1, objects=2, horizon_steps=2,
                             predict_cost=[50, 25, 0, 0, 0, 0, 0, 0])
    assert C.CostmapConfig.from_any(d.costmap).to_dict() == d.costmap
    assert "costmap" not in d.nms_dict() and "costmap" not in d.model_dict()
    cfg["model"]["second"]["costmap"] = {"resolution": -0.1}
    with pytest.raises(ValueError, match="model.second.costmap.*resolution"):
        pp.config.Derived(cfg)
    cfg["model"]["second"]["costmap"] = {"rezolution": 0.1}
    with pytest.raises(ValueError, match="rezolution"):
        pp.config.Derived(cfg)
    cfg["model"]["second"]["costmap"] = 3
    with pytest.raises(ValueError, match="costmap"):
        pp.config.Derived(cfg)


def test_to_occupancy_grid_fields(C):
    c = _cfg(C, x_min=-2.0, y_min=-1.5, resolution=0.25)
    grid, _ = C.costmap_np(_pts([[-1.9, -1.4, 0.5]]), c)
    msg = C.to_occupancy_grid(grid, c, stamp=12.5, frame_id="base_link")
    assert msg["header"] == {"stamp": 12.5, "frame_id": "base_link"}
    info = msg["info"]
    assert info["width"] == 5 and info["height"] == 4 and info["resolution"] == np.float32(0.25)
    assert info["origin"]["position"] == {"x": -2.0, "y": -1.5, "z": 0.0}
    assert info["origin"]["orientation"] == {"x": 0.0, "y": 0.0, "z": 0.0, "w": 1.0}
    data = np.asarray(msg["data"])
    assert data.dtype == np.int8 and data.shape == (20,) and data[0] == 100 and (data[1:] == -1).all()
    assert data[1 * 5 + 2] == grid[1, 2]                      # row-major, data[iy * width + ix]
    assert C.to_occupancy_grid(grid, c)["header"] == {"stamp": None, "frame_id": ""}
    with pytest.raises(ValueError, match="grid must be"):
        C.to_occupancy_grid(grid[:3], c)


# ---- wide grids: the compose kernel's waves inside one row (tests/test_gpu_costmap.py runs them on the GPU) ----
@pytest.mark.parametrize("name", ["w300", "w257"])
def test_wide_grids_put_compose_waves_inside_one_row(pp, C, name):
    """The wave arithmetic from CM_BLOCK and the pitch rule read out of the sources, so the case cannot drift off the
    branch `wiy0 == wiy1, wix0 > 0` of k_costmap_compose; and, on tracks of the host tracker, what the GPU test relies on:
    every cell decided by more than the margin, every cost present, object cells in the columns past the first wave of a
    row and in the first quad."""
    import grid_shape_cases as gc
    csrc = os.path.join(os.path.dirname(pp._lib.__file__), "csrc")
    src = open(os.path.join(csrc, "costmap.hip")).read()
    block = int(re.search(r"constexpr int CM_BLOCK = (\d+);", src).group(1))
    assert block % 64 == 0 and "const int q = blockIdx.x * CM_BLOCK + tid;" in src and "wq0 = q - lane" in src
    assert "wix0 = wiy0 == wiy1 ? (wq0 - wiy0 * qpr) * 4 : 0;" in src and "const int qpr = p.pitch >> 2;" in src
    assert int(re.search(r"constexpr int CM_TILE = (\d+);", src).group(1)) == 64
    assert "const int pitch = (c.width + 3) & ~3;" in open(os.path.join(csrc, "api_costmap.hip")).read()
    g = gc.WIDE_COSTMAPS[name]
    W, H = g["width"], g["height"]
    waves = gc.compose_waves(W, H)
    one_row = [w for w in waves if w[0] == w[1]]
    if name == "w300":
        assert (W + 3) // 4 == 75 and len(waves) == 11 and len(one_row) == 3
        assert [w[2] for w in one_row] == [0, 36, 160] and one_row[0][3] == 255 and one_row[2][3] == 299
    else:
        assert (W + 3) // 4 == 65 and ((W + 3) & ~3) - W == 3 and len(waves) == 6
        assert [(w[0], w[2], w[3]) for w in one_row] == [(0, 0, 255), (4, 240, 259)] and waves[1][:2] == (0, 1)
    past0 = [w for w in one_row if w[2] > 0]
    assert past0
    # the tracks, on the host tracker: two updates 0.05 m apart
    per = [gc.wide_track_rows(name, s) for s in range(gc.WIDE_STREAMS)]
    assert all(len(rr) == 24 for rr in per) and abs(math.hypot(*gc.WIDE_MOVE) - 0.05) < 1e-12
    t = pp.tracking.Tracker(gc.wide_track_config(), gc.WIDE_STREAMS)
    t.step(*gc.wide_det_rows(per), [0.1] * gc.WIDE_STREAMS)
    tr, nt, _ = t.step(*gc.wide_det_rows([gc.wide_moved(rr) for rr in per]), [0.1] * gc.WIDE_STREAMS)
    assert nt.tolist() == [24] * gc.WIDE_STREAMS and np.abs(tr["state"][:, :24, 3]).min() > 0
    frames = gc.wide_frames(name)
    assert all(len(f) >= gc.WIDE_ROWS for f in frames)
    for steps in (0, 2):
        c = C.CostmapConfig.from_any(gc.wide_costmap_config(name, steps))
        culled = 0
        for b in range(gc.WIDE_STREAMS):
            fp = C.footprints_np(c, tracks=tr[b], n_tracks=int(nt[b]))
            assert len(fp) == 24 * (1 + steps)                               # 72: more than one LDS tile of 64
            margin = float(C.decision_margins(c, fp).min())
            assert margin > 1e-7, (steps, b, margin)                         # the GPU test leaves no cell out
            grid, _ = C.costmap_np(frames[b], c, tracks=tr[b], n_tracks=int(nt[b]))
            vals = set(np.unique(grid).tolist())
            assert {100, 0, -1} <= vals and ({70, 60} <= vals) == (steps == 2)
            obj = grid >= 60
            assert obj[:, 256:].any() and obj[:, :4].any() and obj[:, 4:252].any()
            # a wave past column 0 with object cells inside its columns and others of its row outside them: the column cull
            # has footprints to keep and footprints to drop
            culled += sum(1 for r0, _, c0, c1 in past0 if obj[r0, c0:c1 + 1].any() and obj[r0, :c0].any())
        assert culled >= 1, steps
