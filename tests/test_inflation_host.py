"""inflation.py's rule on the CPU: the hand case, the restatement's row / column form against a literal loop over the
obstacles, the table's edges, the compose, the validation, the C-ABI's structure, and that every shared case
(tests/inflation_cases.py) has the property it is there for.  No GPU."""
import ctypes
import dataclasses
import math
import os
import re

import numpy as np
import pytest

import inflation_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def I(pp):
    return pp.inflation


# ---- the rule ----
HAND_TABLE = [100, 99, 65, 47, 36, 28, 23, 19, 16, 13]


def test_hand_case_cell_by_cell(I):
    c = I.InflationConfig(resolution=1.0, inscribed_radius=1.0, inflation_radius=3.0, cost_scaling_factor=1.0)
    assert I.radius_cells(c) == 3
    table = I.cost_table(c)
    assert table.dtype == np.int8 and table.tolist() == HAND_TABLE
    g = np.zeros((9, 9), np.int8)
    g[4, 4] = 100
    out, d2, info = I.inflate_np(g, c, clearance=True, info=True)
    assert out.dtype == np.int8 and d2.dtype == np.uint16 and out.shape == d2.shape == (9, 9)
    for y in range(9):
        for x in range(9):
            q = (x - 4) ** 2 + (y - 4) ** 2
            assert d2[y, x] == (q if q <= 9 else 10), (y, x)
            assert out[y, x] == (HAND_TABLE[q] if q <= 9 else 0), (y, x)
    assert info == {"lethal": 1, "raised": 28}           # the 29 cells within 3 cells, less the obstacle itself
    assert np.array_equal(I.inflate_np(g, c), out)


@pytest.mark.parametrize("name", ["one_cell", "one_row", "corners", "radius_beyond_both_sides", "two_words"])
def test_distance_against_a_loop_over_the_obstacles(I, name):
    _, g, cfg = K.case(name)
    c = I.InflationConfig(**cfg)
    R = I.radius_cells(c)
    assert (g.shape, R) in {((1, 1), 3), ((1, 37), 5), ((29, 37), 4), ((29, 37), 40), ((65, 130), 17)}
    d2 = I.distance2_np(g, c)
    assert d2.dtype == np.uint16 and np.array_equal(d2, K.brute_distance2(g, c.lethal_threshold, R))


def test_table_edges(I):
    # cells of 0.25 m: d = sqrt(d2) * 0.25 is exact for a square d2, so d2 = 4 is exactly 0.5 m and d2 = 16 exactly 1 m
    c = I.InflationConfig(resolution=0.25, inscribed_radius=0.5, inflation_radius=1.0, cost_scaling_factor=2.0)
    assert I.radius_cells(c) == 4
    t = I.cost_table(c)
    assert len(t) == 17 and t[0] == 100
    assert t[1] == t[2] == t[3] == t[4] == 99                      # d = 0.5 at d2 = 4: still inscribed
    assert t[5] == math.floor(98.0 * math.exp(-2.0 * (math.sqrt(5.0) * 0.25 - 0.5)) + 0.5) == 87
    assert t[16] == math.floor(98.0 * math.exp(-2.0 * 0.5) + 0.5) == 36     # d = 1.0 exactly: still inside
    # R is a ceiling: 0.9 m in cells of 0.25 m is R = 4, and the entries from sqrt(d2) * 0.25 > 0.9 on are 0 inside R * R
    c2 = dataclasses.replace(c, inflation_radius=0.9)
    t2 = I.cost_table(c2)
    assert I.radius_cells(c2) == 4 and len(t2) == 17
    assert t2[12] > 0 and t2[13] == t2[14] == t2[15] == t2[16] == 0   # sqrt(13) * 0.25 = 0.9014 > 0.9 >= sqrt(12) * 0.25
    # and such a cell, in reach by d2 but beyond the radius, stays what it was
    g = np.zeros((1, 9), np.int8)
    g[0, 0] = 100
    out, d2 = I.inflate_np(g, c2, clearance=True)
    assert d2[0].tolist() == [0, 1, 4, 9, 16, 17, 17, 17, 17] and out[0, 4] == 0 and out[0, 3] == t2[9] > 0
    # inscribed radius 0: only the obstacle's own cell reads 99 or more
    assert I.cost_table(dataclasses.replace(c, inscribed_radius=0.0))[1] < 99


def test_unknown_min_cost(I):
    g = np.full((1, 9), -1, np.int8)
    g[0, 0] = 100
    base = dict(resolution=1.0, inscribed_radius=1.0, inflation_radius=3.0, cost_scaling_factor=1.0)
    assert I.inflate_np(g, dict(base, unknown_min_cost=1))[0].tolist() == [100, 99, 36, 13, -1, -1, -1, -1, -1]
    assert I.inflate_np(g, dict(base, unknown_min_cost=99))[0].tolist() == [100, 99, -1, -1, -1, -1, -1, -1, -1]
    assert I.inflate_np(g, dict(base, unknown_min_cost=37))[0].tolist() == [100, 99, -1, -1, -1, -1, -1, -1, -1]
    assert I.inflate_np(g, dict(base, unknown_min_cost=36))[0].tolist() == [100, 99, 36, -1, -1, -1, -1, -1, -1]


def test_lethal_threshold(I):
    g = np.zeros((1, 12), np.int8)
    g[0, 1], g[0, 5], g[0, 9] = 64, 65, 100
    base = dict(resolution=1.0, inscribed_radius=0.0, inflation_radius=1.0, cost_scaling_factor=1.0)
    t = I.cost_table(base)[1]
    assert t == 36
    out, info = I.inflate_np(g, dict(base, lethal_threshold=65), info=True)
    assert out[0].tolist() == [0, 64, 0, 0, t, 100, t, 0, t, 100, t, 0] and info == {"lethal": 2, "raised": 5}
    out, info = I.inflate_np(g, dict(base, lethal_threshold=100), info=True)
    assert out[0].tolist() == [0, 64, 0, 0, 0, 65, 0, 0, t, 100, t, 0] and info == {"lethal": 1, "raised": 2}
    out = I.inflate_np(g, dict(base, lethal_threshold=64))
    assert out[0].tolist() == [t, 100, t, 0, t, 100, t, 0, t, 100, t, 0]


def test_compose_is_a_max(I):
    c = dict(resolution=1.0, inscribed_radius=1.0, inflation_radius=3.0, cost_scaling_factor=1.0)
    g = np.zeros((1, 5), np.int8)
    g[0, 0], g[0, 2] = 100, 90
    assert I.cost_table(c)[4] == 36
    assert I.inflate_np(g, c)[0].tolist() == [100, 99, 90, 13, 0]        # 90 under t = 36 stays 90
    g[0, 2] = 20
    assert I.inflate_np(g, c)[0].tolist() == [100, 99, 36, 13, 0]
    g = np.array([[90, 0], [0, 100]], np.int8)                            # the diagonal neighbour: d2 = 2, t = 65
    assert I.inflate_np(g, c).tolist() == [[90, 99], [99, 100]]


def test_validation(I, pp):
    C = I.InflationConfig
    assert C() == C(0.0, 0.3, 1.0, 3.0, 100, 1)
    for kw, msg in ((dict(resolution=-0.1), "resolution = -0.1 must be >= 0"),
                    (dict(resolution=float("nan")), "resolution = nan is not finite"),
                    (dict(resolution="fine"), "resolution must be a number"),
                    (dict(inscribed_radius=-1.0), "inscribed_radius = -1.0 must be >= 0"),
                    (dict(inscribed_radius=True), "inscribed_radius must be a number"),
                    (dict(inflation_radius=0.2), "inflation_radius = 0.2 below inscribed_radius = 0.3"),
                    (dict(inflation_radius=float("inf")), "inflation_radius = inf is not finite"),
                    (dict(cost_scaling_factor=0.0), "cost_scaling_factor = 0.0 must be > 0"),
                    (dict(cost_scaling_factor=float("inf")), "cost_scaling_factor = inf is not finite"),
                    (dict(lethal_threshold=0), r"lethal_threshold = 0 outside \[1, 100\]"),
                    (dict(lethal_threshold=101), r"lethal_threshold = 101 outside \[1, 100\]"),
                    (dict(lethal_threshold=50.0), "lethal_threshold must be an integer"),
                    (dict(unknown_min_cost=0), r"unknown_min_cost = 0 outside \[1, 100\]"),
                    (dict(unknown_min_cost=True), "unknown_min_cost must be an integer"),
                    (dict(resolution=0.1, inflation_radius=6.41), "inflation_radius = 6.41 is 65 cells of 0.1 m, at most PP_INFLATE_MAX_RADIUS = 64")):
        with pytest.raises(ValueError, match="InflationConfig: " + msg):
            C(**kw)
    assert I.radius_cells(C(resolution=0.1, inflation_radius=6.4)) == 64
    assert I.radius_cells(C(resolution=0.1)) == 10 and I.radius_cells(C(resolution=0.3)) == 4      # a ceiling
    with pytest.raises(ValueError, match="rezolution"):
        C.from_any({"rezolution": 0.1})
    with pytest.raises(ValueError, match="inflation"):
        C.from_any(3)
    assert C.from_any(True) == C()
    d = C(resolution=0.05, unknown_min_cost=99).to_dict()
    assert list(d) == [f.name for f in dataclasses.fields(C)] and C.from_any(d).to_dict() == d
    # resolution 0.0 stands for a source's, on the engine only
    for call in (I.cost_table, I.radius_cells, lambda c: I.inflate_np(np.zeros((2, 2), np.int8), c),
                 lambda c: I.distance2_np(np.zeros((2, 2), np.int8), c), lambda c: I.inflate(np.zeros((2, 2), np.int8), c)):
        with pytest.raises(ValueError, match="resolution = 0.0 must be > 0"):
            call(C())
    ok = C(resolution=1.0)
    for bad in (np.zeros((2, 2), np.int16), np.zeros((2,), np.int8), np.zeros((0, 3), np.int8)):
        with pytest.raises(ValueError, match="int8"):
            I.inflate_np(bad, ok)
        with pytest.raises(ValueError, match="int8"):
            I.inflate(bad, ok)
    with pytest.raises(ValueError, match="PP_OCC_MAX_CELLS"):
        I.inflate(np.zeros((1025, 1024), np.int8), ok)
    with pytest.raises(ValueError, match="source must be one of"):
        pp.Engine._infl_source("points")


def test_to_occupancy_grid_passthrough(I):
    g = np.arange(-1, 5, dtype=np.int8).reshape(2, 3)
    msg = I.to_occupancy_grid(g, (1.5, -2.0), 0.25, stamp=3.0, frame_id="odom")
    assert msg["header"] == {"stamp": 3.0, "frame_id": "odom"}
    assert msg["info"]["width"] == 3 and msg["info"]["height"] == 2 and msg["info"]["resolution"] == np.float32(0.25)
    assert msg["info"]["origin"]["position"] == {"x": 1.5, "y": -2.0, "z": 0.0}
    assert msg["data"].dtype == np.int8 and msg["data"].tolist() == [-1, 0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="origin"):
        I.to_occupancy_grid(g, (0.0,), 0.25)


# ---- the shared cases ----
def test_every_case_has_its_property(I):
    res = {}
    for name, g, cfg in K.CASES:
        c = I.InflationConfig(**cfg)
        out, d2, info = I.inflate_np(g, c, clearance=True, info=True)
        res[name] = (g, c, I.radius_cells(c), out, d2, info)
        assert g.dtype == np.int8 and out.shape == g.shape
    assert len(set(K.NAMES)) == len(K.NAMES) == 10
    g, c, R, out, d2, info = res["one_cell"]
    assert g.shape == (1, 1) and out.tolist() == [[100]] and info == {"lethal": 1, "raised": 0}
    g, c, R, out, d2, info = res["one_row"]
    assert g.shape[0] == 1 and g.shape[1] % 4 and info["lethal"] >= 2 and (d2 == R * R + 1).any() and (d2 == R * R).any()
    g, c, R, out, d2, info = res["corners"]
    assert g.shape[1] % 4 and g.shape[0] < K.TILE_H and g.shape[1] < K.TILE_W     # one partial tile, a width no multiple of 4
    assert all(out[y, x] == 100 for y in (0, -1) for x in (0, -1))                # an obstacle in each corner
    assert (g == -1).any() and ((g == -1) & (out > 0)).any() and ((g > 0) & (out == g) & (d2 <= R * R)).any()
    g, c, R, out, d2, info = res["radius_beyond_both_sides"]
    assert R > g.shape[0] and R > g.shape[1] and info["lethal"] >= 2
    assert (d2 <= R * R).all() and d2.max() > 17 * 17                             # every cell is in reach of some obstacle
    g, c, R, out, d2, info = res["two_words"]
    assert g.shape[0] > 2 * K.TILE_H and g.shape[1] > 2 * K.TILE_W                # three tile rows, three words
    assert g[31, 63] == 100 and not (g[:, :100] == 100).sum() - 1
    y, x = 33, 66                                                                 # its nearest obstacle: another word, another tile row
    assert d2[y, x] == 3 * 3 + 2 * 2 and x // K.TILE_W != 63 // K.TILE_W and y // K.TILE_H != 31 // K.TILE_H
    assert d2[31, 63 + R] == R * R and d2[31, 64 + R] == R * R + 1 and d2[31 + R, 63] == R * R
    g, c, R, out, d2, info = res["max_radius"]
    assert R == 64 and g.shape == (70, 70) and info["lethal"] == 2
    assert d2[0, 64] == 64 * 64 and d2[0, 65] == 64 * 64 + 1 and d2[64, 0] == 64 * 64 and d2[5, 69] == 64 * 64
    assert out[0, 64] == max(g[0, 64], I.cost_table(c)[4096]) if g[0, 64] >= 0 else True
    g, c, R, out, d2, info = res["all_obstacle"]
    assert (out == 100).all() and (d2 == 0).all() and info == {"lethal": g.size, "raised": 0}
    assert g.shape[0] > K.TILE_H and g.shape[1] > K.TILE_W
    g, c, R, out, d2, info = res["no_obstacle"]
    assert np.array_equal(out, g) and (d2 == R * R + 1).all() and info == {"lethal": 0, "raised": 0} and (g == -1).any() and (g > 0).any()
    g, c, R, out, d2, info = res["all_unknown"]
    assert (out == -1).all() and (d2 == R * R + 1).all() and info == {"lethal": 0, "raised": 0}
    g, c, R, out, d2, info = res["threshold"]
    assert c.lethal_threshold == 65 and c.unknown_min_cost == 99
    assert g[10, 10] == 64 and out[10, 10] == 64 and d2[10, 10] > 0 and out[10, 20] == 100 and out[20, 10] == 100
    assert ((g == -1) & (out == 99)).any() and ((g == -1) & (out == -1) & (d2 > 1) & (d2 <= R * R)).any()
    # the batch: one shape, three different grids
    assert K.BATCH.shape == (3, 29, 37) and K.BATCH.dtype == np.int8
    assert not np.array_equal(K.BATCH[0], K.BATCH[1]) and not np.array_equal(K.BATCH[1], K.BATCH[2])


# ---- structure ----
NEW = ["pp_set_inflation", "pp_get_inflation_config", "pp_inflate_async", "pp_get_inflated", "pp_inflation_info"]


def test_struct_header_exports_and_sources(pp, I):
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    body = re.search(r"typedef struct pp_inflation_config \{(.*?)\} pp_inflation_config;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(double|int32_t)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in pp._lib.PPInflationConfig._fields_]
    assert [n for _, n in fields] == [f.name for f in dataclasses.fields(I.InflationConfig)]
    kinds = [t for t, _ in fields]
    assert kinds == sorted(kinds)                             # the doubles first
    size = sum(8 if t == "double" else 4 for t in kinds)
    assert size == ctypes.sizeof(pp._lib.PPInflationConfig) == 40
    csrc = os.path.join(os.path.dirname(pp._lib.__file__), "csrc")
    assert "static_assert(sizeof(pp_inflation_config) == 40" in open(os.path.join(csrc, "api_inflate.hip")).read()
    assert re.search(r"#define PP_INFLATE_MAX_RADIUS 64\b", hdr)
    assert pp._lib.PP_INFLATE_MAX_RADIUS == I.PP_INFLATE_MAX_RADIUS == 64
    assert re.search(r"enum \{ PP_INFLATE_COSTMAP = 0, PP_INFLATE_OCCUPANCY = 1 \}", hdr)
    assert (pp._lib.PP_INFLATE_COSTMAP, pp._lib.PP_INFLATE_OCCUPANCY) == (0, 1) and I.SOURCES == ("costmap", "occupancy")
    assert "#define PP_ABI_VERSION 4" in hdr
    # the structs the stage was not to touch
    assert ctypes.sizeof(pp._lib.PPCostmapConfig) == 128 and ctypes.sizeof(pp._lib.PPOccupancyConfig) == 56
    later = hdr[hdr.index("later additions within 4"):hdr.index("#define PP_ABI_VERSION")]
    for name in ["PP_INFLATE_MAX_RADIUS", "pp_inflation_config", "PP_INFLATE_COSTMAP", "PP_INFLATE_OCCUPANCY", "pp_inflate_grids"] + NEW:
        assert re.search(r"\b%s\b" % name, later), name
    exp = pp._lib.EXPORTS
    for name in NEW:
        assert name in exp and re.search(r"\bint %s\(pp_handle" % name, hdr), name
        assert exp.index("pp_occupancy_reset") < exp.index(name) < exp.index("pp_soft_nms")
    assert "pp_inflate_grids" in exp and re.search(r"\bint pp_inflate_grids\(int device", hdr)
    src = pp._lib.SOURCES
    for s in ("api_inflate.hip", "inflate.hip"):
        assert s in src and os.path.exists(os.path.join(csrc, s))
        assert src.index("occupancy.hip") < src.index(s) < src.index("api_track.hip")
    assert src[-2:] == ["api_track.hip", "track.hip"]
    assert "inflation" in pp.__all__
    for name in ("InflationConfig", "radius_cells", "cost_table", "distance2_np", "inflate_np", "inflate", "to_occupancy_grid"):
        assert callable(getattr(I, name)), name
    for name in ("set_inflation", "inflation_config", "inflate_async", "inflated_costmaps", "inflated_occupancy_maps", "inflation_info"):
        assert callable(getattr(pp.Engine, name)), name
    assert callable(pp.VoxelNet.inflated_costmaps) and callable(pp.VoxelNet.inflated_occupancy_maps)
    # opt-in at run time only: no configuration key, no environment switch
    assert not hasattr(pp.config.Derived(pp.config.tiny_config(1)), "inflation")
    assert "INFL" not in open(os.path.join(csrc, "pp_switches.h")).read().upper()
    for f in ("api_inflate.hip", "inflate.hip"):
        assert "getenv" not in open(os.path.join(csrc, f)).read()


def test_exported_from_the_library_and_null_handle(pp, hip_lib):
    for name in NEW + ["pp_inflate_grids"]:
        assert hasattr(hip_lib, name), name
    PP_ERR_ARG = 1
    c = pp._lib.PPInflationConfig()
    on = ctypes.c_int32(7)
    assert hip_lib.pp_set_inflation(None, 0, ctypes.byref(c), None, 0) == PP_ERR_ARG
    assert hip_lib.pp_set_inflation(None, 1, None, None, 0) == PP_ERR_ARG
    assert hip_lib.pp_get_inflation_config(None, 0, ctypes.byref(on), None) == PP_ERR_ARG and on.value == 7
    assert hip_lib.pp_inflate_async(None, 0) == PP_ERR_ARG
    assert hip_lib.pp_get_inflated(None, 0, None, None, 1) == PP_ERR_ARG
    assert hip_lib.pp_inflation_info(None, 1, None, None, 1) == PP_ERR_ARG
    # the stand-alone call refuses its arguments before it looks for a device
    g = np.zeros((2, 2), np.int8)
    ok = pp._lib.PPInflationConfig(1.0, 0.3, 1.0, 3.0, 100, 1)
    call = hip_lib.pp_inflate_grids
    assert call(0, None, 1, 2, 2, ctypes.byref(ok), None, 0, g.ctypes.data, None, None) == PP_ERR_ARG
    assert call(0, g.ctypes.data, 0, 2, 2, ctypes.byref(ok), None, 0, g.ctypes.data, None, None) == PP_ERR_ARG
    assert b"batch = 0" in hip_lib.pp_last_error(None)
    assert call(0, g.ctypes.data, 1, 1025, 1024, ctypes.byref(ok), None, 0, g.ctypes.data, None, None) == PP_ERR_ARG
    assert b"PP_OCC_MAX_CELLS" in hip_lib.pp_last_error(None)
    far = pp._lib.PPInflationConfig(0.1, 0.3, 6.41, 3.0, 100, 1)
    assert call(0, g.ctypes.data, 1, 2, 2, ctypes.byref(far), None, 0, g.ctypes.data, None, None) == PP_ERR_ARG
    assert b"inflation_radius = 6.41 is 65 cells of 0.1 m, at most PP_INFLATE_MAX_RADIUS = 64" in hip_lib.pp_last_error(None)
    t = np.zeros(3, np.int8)
    assert call(0, g.ctypes.data, 1, 2, 2, ctypes.byref(ok), t.ctypes.data, 3, g.ctypes.data, None, None) == PP_ERR_ARG
    assert b"table has 3 entries, R * R + 1 = 2" in hip_lib.pp_last_error(None)
    t = np.array([100, 101], np.int8)
    assert call(0, g.ctypes.data, 1, 2, 2, ctypes.byref(ok), t.ctypes.data, 2, g.ctypes.data, None, None) == PP_ERR_ARG
    assert b"table[1] = 101 outside [0, 100]" in hip_lib.pp_last_error(None)
    for field, v, msg in (("resolution", 0.0, b"resolution = 0 must be > 0"), ("lethal_threshold", 0, b"lethal_threshold = 0 outside [1, 100]"),
                          ("cost_scaling_factor", float("nan"), b"cost_scaling_factor is not finite")):
        bad = pp._lib.PPInflationConfig(1.0, 0.3, 1.0, 3.0, 100, 1)
        setattr(bad, field, v)
        assert call(0, g.ctypes.data, 1, 2, 2, ctypes.byref(bad), None, 0, g.ctypes.data, None, None) == PP_ERR_ARG
        assert msg in hip_lib.pp_last_error(None), hip_lib.pp_last_error(None)
