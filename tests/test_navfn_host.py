"""navfn.py's rule on the CPU: the pinned field, the heap Dijkstra against the relaxation sweeps on every shared case
(tests/navfn_cases.py), the path's invariants and tie-break, the metres-to-cells arithmetic, the validation, the overflow
bound and the C-ABI's structure.  No GPU."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import navfn_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def N(pp):
    return pp.navfn


# ---- the rule ----
def test_pinned_field_cell_by_cell(N):
    _, g, goal, start, cfg = K.case("pinned")
    pot, info = N.navfn_np(g, goal, cfg, info=True)
    assert pot.dtype == np.uint32 and pot.shape == (5, 5) and N.UNREACHED == 0xFFFFFFFF
    for y in range(5):
        for x in range(5):
            want = K.PINNED_FIELD[y][x]
            assert pot[y, x] == (N.UNREACHED if want is None else want), (x, y)
    assert info == {"goal_state": 0, "reached": 22}
    assert pot[1, 3] == 570                                # its diagonal to (4, 2) is barred: (3, 2) is blocked
    cost = N.cell_costs_np(g, cfg)
    assert cost.dtype == np.uint16 and cost[1, 3] == 70 and cost[2, 2] == 0 and cost[0, 0] == 10


@pytest.mark.parametrize("name", K.NAMES)
def test_dijkstra_equals_the_relaxation_sweeps(N, name):
    _, g, goal, start, cfg = K.case(name)
    pot, info, _, _ = K.reference(name)
    relaxed, rinfo = N.relax_np(g, goal, cfg, info=True)
    assert relaxed.dtype == np.uint32 and np.array_equal(pot, relaxed)
    assert {k: rinfo[k] for k in info} == info
    blocked = N.cell_costs_np(g, cfg) == 0
    assert (pot[blocked] == N.UNREACHED).all()


@pytest.mark.parametrize("name", K.NAMES)
def test_path_invariants(N, name):
    _, g, goal, start, cfg = K.case(name)
    c = N.NavfnConfig.from_any(cfg)
    pot, info, path, state = K.reference(name)
    assert path.dtype == np.int32 and path.shape == (len(path), 2) and len(path) <= c.max_path
    if state in (1, 2, 4):
        assert len(path) == 0
        return
    cost = N.cell_costs_np(g, cfg).astype(np.int64)
    assert tuple(path[0]) == tuple(start)
    total = 0
    for (x, y), (qx, qy) in zip(path[:-1], path[1:]):
        dx, dy = qx - x, qy - y
        assert (dx, dy) in N.NEIGHBOURS[:c.connectivity]
        assert cost[qy, qx] != 0
        if dx and dy:
            assert cost[y, qx] != 0 and cost[qy, x] != 0           # no corner cutting
        assert pot[qy, qx] < pot[y, x]
        total += (N.D if dx and dy else N.A) * cost[y, x]
    if state == 0:
        assert tuple(path[-1]) == tuple(goal) and total == pot[start[1], start[0]]
    else:
        assert state == 3 and len(path) == c.max_path and pot[path[-1][1], path[-1][0]] != 0


def test_the_cases_have_their_properties(N):
    ref = {n: K.reference(n) for n in K.NAMES}
    assert ref["one_cell"][0].tolist() == [[0]] and ref["one_cell"][2].tolist() == [[0, 0]]
    assert ref["diagonal_both_beside_blocked"][1]["reached"] == 1 and ref["diagonal_both_beside_blocked"][3] == 1
    assert ref["diagonal_one_beside_blocked"][2].tolist() == [[1, 1], [0, 1], [0, 0]]      # round the blocked cell, not across
    assert ref["diagonal_connectivity_4"][2].tolist() == [[2, 2], [1, 2], [0, 2], [0, 1], [0, 0]]
    for n in K.NAMES:
        if n.startswith("random_"):
            g = K.case(n)[1]
            assert K.reached_share(n) >= 0.5 and ref[n][3] == 0 and (g == -1).any() and (g == 100).any()
    assert {K.case(n)[1].shape for n in K.NAMES if n.startswith("random_")} == set(K.RANDOM_SHAPES)
    assert K.case("random_37x63_known_flat")[1].shape[1] % 4 == 3
    assert ref["goal_enclosed"][1] == {"goal_state": 0, "reached": 1} and ref["goal_enclosed"][3] == 1
    assert ref["goal_blocked"][1] == {"goal_state": 1, "reached": 0}
    assert ref["goal_outside_negative"][1]["goal_state"] == ref["goal_outside_right"][1]["goal_state"] == 2
    assert [ref[n][3] for n in ("start_blocked", "start_outside", "start_absent")] == [1, 2, 4]
    assert ref["max_path_short"][3] == 3 and len(ref["max_path_short"][2]) == 5
    assert ref["max_path_exact"][3] == 0 and len(ref["max_path_exact"][2]) == 20            # the goal is the last cell allowed
    assert ref["serpentine_cut"][3] == 3 and len(ref["serpentine_cut"][2]) == 1024
    assert ref["serpentine_whole"][3] == 0 and 1024 < len(ref["serpentine_whole"][2]) <= 4096
    assert np.array_equal(ref["serpentine_whole"][2][:1024], ref["serpentine_cut"][2])
    g = K.case("corridor")[1]
    assert g.shape == (8, 2048) and g.shape[1] // K.TILE >= 32 and ref["corridor"][3] == 0
    assert K.BATCH.shape == (3, 65, 40) and K.BATCH.dtype == np.int8 and K.BATCH[0][10, 7] == 100


def test_tie_break_on_an_empty_grid(N):
    g = np.zeros((3, 3), np.int8)
    pot = N.navfn_np(g, (1, 1), True)
    assert pot.tolist() == [[70, 50, 70], [50, 0, 50], [70, 50, 70]]
    # from a corner the diagonal is the only minimum; from (0, 0) with the goal at (2, 1): E then NE ties with NE then E
    pot = N.navfn_np(g, (2, 1), True)
    assert pot[0, 0] == 120
    path, state = N.descend_np(pot, g, (0, 0), True)
    assert state == 0 and path.tolist() == [[0, 0], [1, 0], [2, 1]]       # E comes before NE in the rule's order
    path, state = N.descend_np(N.navfn_np(g, (0, 1), True), g, (2, 2), True)
    assert path.tolist() == [[2, 2], [1, 2], [0, 1]]                      # W before SW


def test_goal_cells_and_path_to_metres(N):
    shape = (29, 37)
    xy = np.array([[-0.05, 0.0], [0.0, 0.1], [0.1, 0.05], [3.7, 0.0], [1e300, -1e300], [np.nan, 0.0], [0.3, np.inf]])
    c = N.goal_cells(xy, (0.0, 0.0), 0.1, shape)
    assert c.dtype == np.int32 and c.tolist() == [[-1, 0], [0, 1], [1, 0], [37, 0], [37, -1], [-1, -1], [-1, -1]]
    assert N.goal_cells((0.25, 0.25), (0.0, 0.0), 0.25, shape).tolist() == [[1, 1]]        # an exact cell edge belongs to the upper cell
    assert N.goal_cells((-0.25, -0.26), (0.0, 0.0), 0.25, (64, 64)).tolist() == [[-1, -1]]
    assert N.goal_cells((-0.3, 0.2), (-1.0, -1.0), 0.5, shape).tolist() == [[1, 2]]
    org = np.array([[0.0, 0.0], [np.nan, 0.0]])
    assert N.goal_cells([[1.0, 1.0], [1.0, 1.0]], org, 0.5, shape).tolist() == [[2, 2], [-1, -1]]
    with pytest.raises(ValueError, match="resolution"):
        N.goal_cells((0.0, 0.0), (0.0, 0.0), 0.0, shape)
    m = N.path_to_metres(np.array([[0, 0], [2, 3]], np.int32), (-1.0, 0.5), 0.1)
    assert m.dtype == np.float64 and np.array_equal(m, np.array([-1.0, 0.5]) + (np.array([[0, 0], [2, 3]]) + 0.5) * 0.1)
    assert N.path_to_metres(np.zeros((0, 2), np.int32), (0.0, 0.0), 0.1).shape == (0, 2)


RANGES = [("lethal_cost", 1, 100), ("neutral_cost", 1, 50), ("cost_factor", 0, 5), ("allow_unknown", 0, 1), ("unknown_cost", 0, 100),
          ("connectivity", 4, 8), ("max_path", 1, 4096), ("queued_rounds", 0, 4096)]


def test_validation_field_by_field(N):
    C = N.NavfnConfig
    assert C() == C(99, 10, 1, 0, 50, 8, 1024, 0)
    assert [f.name for f in dataclasses.fields(C)] == [r[0] for r in RANGES]
    for name, lo, hi in RANGES:
        C(**{name: lo}), C(**{name: hi})
        for bad in (lo - 1, hi + 1):
            with pytest.raises(ValueError, match=r"NavfnConfig: %s = %d outside \[%d, %d\]" % (name, bad, lo, hi)):
                C(**{name: bad})
        for bad in (1.0, True, "x"):
            with pytest.raises(ValueError, match=f"NavfnConfig: {name} must be an integer"):
                C(**{name: bad})
    with pytest.raises(ValueError, match="NavfnConfig: connectivity = 6 must be 4 or 8"):
        C(connectivity=6)
    with pytest.raises(ValueError, match="konnectivity"):
        C.from_any({"konnectivity": 4})
    with pytest.raises(ValueError, match="navfn"):
        C.from_any(3)
    assert C.from_any(True) == C()
    d = C(max_path=7, connectivity=4).to_dict()
    assert list(d) == [r[0] for r in RANGES] and C.from_any(d).to_dict() == d
    for bad in (np.zeros((2, 2), np.int16), np.zeros((2,), np.int8), np.zeros((0, 3), np.int8)):
        with pytest.raises(ValueError, match="int8"):
            N.navfn_np(bad, (0, 0), True)
        with pytest.raises(ValueError, match="int8"):
            N.navfn(bad, (0, 0), True)
    with pytest.raises(ValueError, match="PP_OCC_MAX_CELLS"):
        N.navfn(np.zeros((1025, 1024), np.int8), (0, 0), True)
    with pytest.raises(ValueError, match="goals must be integer cells"):
        N.navfn(np.zeros((2, 2), np.int8), (0.5, 0.5), True)
    with pytest.raises(ValueError, match="goal must be an integer cell"):
        N.navfn_np(np.zeros((2, 2), np.int8), (0.5, 0.5), True)


def test_a_uint32_potential_cannot_overflow(N, pp):
    assert N.MAX_COST == 50 + 5 * 100 == 550 and N.D * N.MAX_COST == 3850
    assert 7 * 550 * 2 ** 20 < 2 ** 32 - 1 and pp._lib.PP_OCC_MAX_CELLS == 2 ** 20
    g = np.full((1, 3), 100, np.int8)
    assert N.cell_costs_np(g, dict(lethal_cost=100, cost_factor=5, neutral_cost=50))[0, 0] == 0     # 100 is blocked at the largest threshold
    g = np.full((1, 3), -1, np.int8)
    assert N.cell_costs_np(g, dict(allow_unknown=1, unknown_cost=100, cost_factor=5, neutral_cost=50)).max() == 550


# ---- structure ----
NEW = ["pp_set_navfn", "pp_get_navfn_config", "pp_navfn_async", "pp_get_navfn", "pp_navfn_info"]


def test_struct_header_exports_and_sources(pp, N):
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    body = re.search(r"typedef struct pp_navfn_config \{(.*?)\} pp_navfn_config;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in pp._lib.PPNavfnConfig._fields_] == [r[0] for r in RANGES]
    assert 4 * len(fields) == ctypes.sizeof(pp._lib.PPNavfnConfig) == 32
    csrc = os.path.join(os.path.dirname(pp._lib.__file__), "csrc")
    api = open(os.path.join(csrc, "api_navfn.hip")).read()
    assert "static_assert(sizeof(pp_navfn_config) == 32" in api
    assert re.search(r"#define PP_NAVFN_UNREACHED 0xFFFFFFFFu\b", hdr) and re.search(r"#define PP_NAVFN_MAX_PATH 4096\b", hdr)
    assert pp._lib.PP_NAVFN_UNREACHED == N.UNREACHED == 0xFFFFFFFF and pp._lib.PP_NAVFN_MAX_PATH == 4096
    assert "#define PP_ABI_VERSION 4" in hdr
    assert ctypes.sizeof(pp._lib.PPInflationConfig) == 40                 # the struct the stage was not to touch
    later = hdr[hdr.index("later additions within 4"):hdr.index("#define PP_ABI_VERSION")]
    for name in ["pp_navfn_config", "PP_NAVFN_UNREACHED", "PP_NAVFN_MAX_PATH", "pp_navfn_grids"] + NEW:
        assert re.search(r"\b%s\b" % name, later), name
    assert "3850 * PP_OCC_MAX_CELLS < 2^32 - 1" in hdr                     # the header says why the ranges are what they are
    exp = pp._lib.EXPORTS
    at = exp.index("pp_inflate_grids")
    assert exp[at + 1:at + 7] == NEW + ["pp_navfn_grids"]
    for name in NEW:
        assert re.search(r"\bint %s\(pp_handle" % name, hdr), name
    assert re.search(r"\bint pp_navfn_grids\(int device", hdr)
    src = pp._lib.SOURCES
    at = src.index("inflate.hip")
    assert src[at + 1:at + 3] == ["api_navfn.hip", "navfn.hip"] and src[-2:] == ["api_track.hip", "track.hip"]
    assert "navfn" in pp.__all__ and "planner" in pp.__all__
    for name in ("NavfnConfig", "cell_costs_np", "navfn_np", "relax_np", "descend_np", "goal_cells", "path_to_metres", "navfn"):
        assert callable(getattr(N, name)), name
    for name in ("set_navfn", "navfn_config", "navfn_async", "navfn_fields", "navfn_paths", "navfn_info", "plan"):
        assert callable(getattr(pp.Engine, name)), name
    assert callable(pp.VoxelNet.plan)
    # opt-in at run time only: no configuration key, no environment switch
    assert not hasattr(pp.config.Derived(pp.config.tiny_config(1)), "navfn")
    assert "NAV" not in open(os.path.join(csrc, "pp_switches.h")).read().upper()
    for f in ("api_navfn.hip", "navfn.hip"):
        assert "getenv" not in open(os.path.join(csrc, f)).read()
    assert "navfn_release(e);" in open(os.path.join(csrc, "pp_api.hip")).read()


def test_exported_from_the_library_and_null_handle(pp, hip_lib):
    for name in NEW + ["pp_navfn_grids"]:
        assert hasattr(hip_lib, name), name
    PP_ERR_ARG = 1
    c = pp._lib.PPNavfnConfig(99, 10, 1, 0, 50, 8, 1024, 0)
    on = ctypes.c_int32(7)
    cells = np.zeros((1, 2), np.int32)
    assert hip_lib.pp_set_navfn(None, 0, ctypes.byref(c)) == PP_ERR_ARG
    assert hip_lib.pp_set_navfn(None, 1, None) == PP_ERR_ARG
    assert hip_lib.pp_get_navfn_config(None, 0, ctypes.byref(on), None) == PP_ERR_ARG and on.value == 7
    assert hip_lib.pp_navfn_async(None, 0, cells.ctypes.data, None, 1) == PP_ERR_ARG
    assert hip_lib.pp_get_navfn(None, 0, None, None, None, 1) == PP_ERR_ARG
    assert hip_lib.pp_navfn_info(None, 1, None, None, None, None, 1) == PP_ERR_ARG
    # the stand-alone call refuses its arguments before it looks for a device
    g = np.zeros((2, 2), np.int8)
    call = hip_lib.pp_navfn_grids
    assert call(0, None, 1, 2, 2, ctypes.byref(c), cells.ctypes.data, None, None, None, None, None) == PP_ERR_ARG
    assert call(0, g.ctypes.data, 1, 2, 2, ctypes.byref(c), None, None, None, None, None, None) == PP_ERR_ARG
    assert call(0, g.ctypes.data, 0, 2, 2, ctypes.byref(c), cells.ctypes.data, None, None, None, None, None) == PP_ERR_ARG
    assert b"batch = 0" in hip_lib.pp_last_error(None)
    assert call(0, g.ctypes.data, 1, 1025, 1024, ctypes.byref(c), cells.ctypes.data, None, None, None, None, None) == PP_ERR_ARG
    assert b"PP_OCC_MAX_CELLS" in hip_lib.pp_last_error(None)
    for field, v, msg in (("lethal_cost", 0, b"lethal_cost = 0 outside [1, 100]"), ("neutral_cost", 51, b"neutral_cost = 51 outside [1, 50]"),
                          ("cost_factor", 6, b"cost_factor = 6 outside [0, 5]"), ("connectivity", 6, b"connectivity = 6 must be 4 or 8"),
                          ("max_path", 4097, b"max_path = 4097 outside [1, 4096]"), ("queued_rounds", -1, b"queued_rounds = -1 outside [0, 4096]")):
        bad = pp._lib.PPNavfnConfig(99, 10, 1, 0, 50, 8, 1024, 0)
        setattr(bad, field, v)
        assert call(0, g.ctypes.data, 1, 2, 2, ctypes.byref(bad), cells.ctypes.data, None, None, None, None, None) == PP_ERR_ARG
        assert msg in hip_lib.pp_last_error(None), hip_lib.pp_last_error(None)
