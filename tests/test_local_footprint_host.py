"""The footprint of local_planner.py on the CPU: the step-by-step statement against the all-samples-at-once statement on
every shared case (tests/local_footprint_cases.py, whose import asserts the properties the cases are named for), with and
without movers; the invariant on the counts; state 5 and start_probe; `Footprint.polygon` / `rectangle` on a hand-worked
rectangle, with every refusal; the C-ABI's structure; and the doorway, where the footprint changes what the robot may do.
footprint=None against the parent's digests is tests/test_local_movers_host.py's.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import local_footprint_cases as F
import local_mover_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def LP(pp):
    return pp.local_planner


# ---- the rule ----
@pytest.mark.parametrize("name", F.NAMES)
def test_step_by_step_equals_all_at_once(LP, name):
    c, b = F.case(name), F.case(name).base
    args = (b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, c.movers, c.mcfg, c.probes, c.fcfg)
    keys, reasons = LP.scores_np(*args)
    keys1, reasons1 = LP.keys_by_sample_np(*args)
    assert np.array_equal(keys, keys1) and np.array_equal(reasons, reasons1)
    want = F.reference(name)
    got = F.run(c, samples=LP.keys_by_sample_np)
    extra = {"n_movers", "n_dynamic", "near"} if c.movers is not None else set()
    assert set(want) == set(got) == set(LP.RESULT) | {"score", "traj", "keys"} | set(LP.FOOT_INFO) | extra
    for k in want:
        assert np.array_equal(want[k], got[k]), k
    n = b.cfg["nv"] * b.cfg["nw"]
    if want["cmd_state"] < 2:                               # the invariant on the counts, from the reasons themselves
        assert np.array_equal(want["keys"], keys) and want["n_footprint"] == int((reasons == LP.FOOTPRINT).sum())
        counts = [int((reasons == r).sum()) for r in range(6)]
        assert sum(counts) == n and counts[:4] == [want[k] for k in ("n_ok", "n_outside", "n_collision", "n_unreached")]
        assert counts[LP.DYNAMIC] == want.get("n_dynamic", 0) and ((keys != LP.INVALID) == (reasons == LP.OK)).all()
    else:
        assert (want["keys"] == LP.INVALID).all() and want["best"] == -1 and len(want["traj"]) == 0 and want["score"] == 0
        assert all(want[k] == 0 for k in ("sv", "sw", "n_ok", "n_outside", "n_collision", "n_unreached", "n_footprint"))
    if want["cmd_state"] == 0:                              # the winner is free of every probe at every pose it keeps
        for pose in want["traj"][1:]:
            assert F.first_bad(c, tuple(int(v) for v in pose)) is None


def test_batch_reference(LP):
    for b in range(3):
        k, _ = LP.keys_by_sample_np(F.BATCH[b], F.BATCH_POTS[b], F.BATCH_POSES[b], F.BATCH_WINDOWS[b], F.BATCH_NCFG, F.BATCH_CFG,
                                    footprint=F.BATCH_PROBES)
        if F.batch_reference(b)["cmd_state"] < 2:
            assert np.array_equal(F.batch_reference(b)["keys"], k)


def test_state_5_and_start_probe(LP):
    c = F.case("state_5_start_blocked")
    b = c.base
    r = F.reference(c.name)
    q, cell = F.first_bad(c, b.pose)
    assert r["cmd_state"] == LP.STATE_FOOTPRINT == 5 and r["start_probe"] == q == LP.start_probe_np(b.grid, b.pose, b.ncfg, c.probes)
    assert b.grid[cell[1], cell[0]] == 100 and F.first_bad(c._replace(probes=c.probes[:q]), b.pose) is None
    # a table that ends before that probe is free at the start, and the samples are rolled
    short = F.run(c._replace(probes=c.probes[:q]))
    assert short["cmd_state"] in (0, 1) and short["start_probe"] == -1 and short["n_footprint"] + short["n_ok"] > 0
    # the order 4, 3, 2 before 5; 5 before 1
    for name, state in (("state_goal_blocked", 4), ("state_pose_blocked", 3), ("state_pose_outside", 3), ("state_arrived", 2)):
        assert F.reference(name)["cmd_state"] == state and F.reference(name)["start_probe"] == -1
    arrived = F.case("state_arrived")
    assert LP.start_probe_np(arrived.base.grid, arrived.base.pose, arrived.base.ncfg, [(20 * LP.SUB, 0)]) == 0      # (it would not be free)
    assert F.reference("state_5_before_1")["cmd_state"] == 5 and F.point("state_5_before_1")["cmd_state"] == 1
    # outside counts as not free; unknown only while allow_unknown is 0
    assert F.reference("state_5_start_outside")["start_probe"] == 0
    g = np.full((8, 8), -1, np.int8)
    g[4, 4] = 0
    pose = (4 * LP.SUB + 512, 4 * LP.SUB + 512, 0)
    assert LP.start_probe_np(g, pose, dict(allow_unknown=0), [(0, 0), (LP.SUB, 0)]) == 1
    assert LP.start_probe_np(g, pose, dict(allow_unknown=1), [(0, 0), (LP.SUB, 0)]) == -1
    # foot_lethal: 100 lets a probe into the ring, 99 does not
    ring = F.case("ring_lethal_99")
    hit = {int(ring.base.grid[cy, cx]) for cx, cy in _probe_cells_that_end(LP, ring)}
    assert 99 in hit and LP.FootprintConfig().foot_lethal == 100


def _probe_cells_that_end(LP, c):
    b = c.base
    reasons = F.reasons(c.name)
    for s in np.flatnonzero(reasons == LP.FOOTPRINT):
        poses = LP.score_np(b.grid, b.pot, b.pose, *LP.sample(s, b.window, b.cfg), b.ncfg, b.cfg, None, None, c.probes, c.fcfg)[2]
        yield F.first_bad(c, poses[-1])[1]


def test_bounds(pp, LP):
    assert LP.FOOTPRINT == 5 and LP.STATE_FOOTPRINT == 5 and LP.FOOT_INFO == ("n_probes", "n_footprint", "start_probe")
    assert 32767 * 16384 * 2 + 8192 < 2 ** 31 and (pp._lib.PP_OCC_MAX_CELLS + 1) * 1024 + 2 * 32767 + 1 < 2 ** 31
    csrc = os.path.join(os.path.dirname(pp._lib.__file__), "csrc")
    src = open(os.path.join(csrc, "local_plan.hip")).read()
    assert "32767ll * 16384 * 2 + 8192 < (1ll << 31)" in src and "2ll * PP_LOCAL_MAX_PROBE + 1 < (1ll << 31)" in src
    assert "template <bool MOVERS, bool FOOT>" in src
    for name in ("k_local_rollout_foot", "k_local_rollout_movers_foot", "k_local_finish_foot", "k_local_finish_movers_foot",
                 "k_local_rollout", "k_local_rollout_movers", "k_local_finish", "k_local_finish_movers"):
        assert '"%s"' % name in src, name
    code = re.sub(r"//.*", "", src)
    assert "float" not in code and "double" not in code and "getenv" not in code
    common = open(os.path.join(csrc, "pp_common.h")).read()
    assert re.search(r"constexpr int LOC_FOOT_GROUP = (1|8|16|64);", common)


# ---- from metres to probes ----
def test_rectangle_by_hand(LP):
    """1.0 m x 0.5 m at 0.25 m cells, spacing 1 cell: 4 + 2 + 4 + 2 probes, every value a multiple of 1024 or 512."""
    f = LP.Footprint.rectangle(1.0, 0.5, resolution=0.25, spacing=1.0)
    want = [(-2048, -1024), (-1024, -1024), (0, -1024), (1024, -1024),          # the right side, rear to front
            (2048, -1024), (2048, 0),                                           # the front
            (2048, 1024), (1024, 1024), (0, 1024), (-1024, 1024),               # the left side, front to rear
            (-2048, 1024), (-2048, 0)]                                          # the rear
    assert f.probes.dtype == np.int64 and f.probes.tolist() == [list(p) for p in want] and len(f) == 12
    assert f.inscribed_radius() == 0.25 and f.circumscribed_radius() == np.hypot(0.5, 0.25)
    # the default spacing of half a cell: twice the points per edge
    assert len(LP.Footprint.rectangle(1.0, 0.5, resolution=0.25)) == 24
    # offset_x moves the outline, and the radii with it
    g = LP.Footprint.rectangle(1.0, 0.5, 0.25, resolution=0.25, spacing=1.0)
    assert g.probes.tolist() == [[x + 1024, y] for x, y in want] and g.inscribed_radius() == 0.25
    assert g.circumscribed_radius() == np.hypot(0.75, 0.25)
    # n = max(1, ceil(L / (spacing * resolution))): an edge of 0.5 m at 0.3 m a point gives 2 points, at the fractions 0 and 1 / 2
    t = LP.Footprint.polygon([(-0.25, -0.25), (0.25, -0.25), (0.0, 0.5)], 0.25, spacing=1.2)
    assert t.probes[:2].tolist() == [[-1024, -1024], [0, -1024]]
    # the robot of the cases
    assert len(F.RECT) == 56 and abs(F.RECT.inscribed_radius() - 0.25) < 1e-12 and abs(F.RECT.circumscribed_radius() - np.hypot(0.45, 0.25)) < 1e-12
    assert F.RECT == LP.Footprint(F.RECT.probes) and F.RECT != F.RECT_256


def test_duplicates_are_dropped_keeping_the_first(LP):
    # a vertex given twice in a row: an edge of length 0 gives n = 1 point, the vertex again
    v = [(-0.5, -0.25), (0.5, -0.25), (0.5, -0.25), (0.5, 0.25), (-0.5, 0.25)]
    f = LP.Footprint.polygon(v, 0.25, spacing=1.0)
    assert f == LP.Footprint.rectangle(1.0, 0.5, resolution=0.25, spacing=1.0)
    # points closer than a sub-cell collapse: cells of 256 m make 1 m four sub-cells, and a point every 0.125 m rounds (half
    # to even) onto -2 -2 -1 -0 0 0 1 2 along the first edge
    f = LP.Footprint.rectangle(1.0, 0.5, resolution=256.0, spacing=1.0 / 2048.0)
    assert f.probes.tolist() == [[-2, -1], [-1, -1], [0, -1], [1, -1], [2, -1], [2, 0], [2, 1], [1, 1], [0, 1], [-1, 1], [-2, 1], [-2, 0]]


def test_polygon_refusals(LP):
    sq = [(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)]
    for v, msg in (([(0.0, 0.0), (1.0, 0.0)], "fewer than 3"), ([], "vertices must be"), ([(0.0, 0.0, 0.0)] * 3, "vertices must be"),
                   ([(np.nan, 0.0), (1.0, 0.0), (0.0, 1.0)], "vertices must be"),
                   ([(0.1, 0.1), (1.0, 0.1), (1.0, 1.0), (0.1, 1.0)], "origin is not strictly inside"),
                   ([(0.0, -0.5), (0.5, -0.5), (0.5, 0.5), (0.0, 0.5)], "origin is not strictly inside"),      # on an edge
                   ([(0.0, 0.0), (0.5, 0.0), (0.5, 0.5)], "origin is not strictly inside")):                  # on a vertex
        with pytest.raises(ValueError, match="Footprint.polygon: .*" + msg):
            LP.Footprint.polygon(v, 0.25)
    assert len(LP.Footprint.polygon(sq[::-1], 0.25)) == len(LP.Footprint.polygon(sq, 0.25))                   # either sense of rotation
    with pytest.raises(ValueError, match=r"Footprint.polygon: the probe \(32768, -1024\).*out of range"):
        LP.Footprint.polygon([(-0.25, -0.25), (8.0, -0.25), (8.0, 0.25), (-0.25, 0.25)], 0.25, spacing=64.0)
    assert LP.Footprint.polygon([(-0.25, -0.25), (32767 / 4096, -0.25), (32767 / 4096, 0.25), (-0.25, 0.25)], 0.25, spacing=64.0).probes.max() == 32767
    with pytest.raises(ValueError, match="Footprint.polygon: 258 probes, more than PP_LOCAL_MAX_PROBES = 256"):
        LP.Footprint.rectangle(0.9, 0.5, resolution=0.1, spacing=0.109375)
    for kw, msg in ((dict(resolution=0.0), "resolution"), (dict(resolution=np.nan), "resolution"), (dict(resolution=0.25, spacing=0.0), "spacing"),
                    (dict(resolution=0.25, spacing=np.inf), "spacing")):
        with pytest.raises(ValueError, match="Footprint.polygon: " + msg):
            LP.Footprint.polygon(sq, **kw)
    for a in ((0.0, 0.5), (1.0, -0.5), (np.inf, 0.5)):
        with pytest.raises(ValueError, match="Footprint.rectangle"):
            LP.Footprint.rectangle(*a, resolution=0.25)
    with pytest.raises(TypeError):
        LP.Footprint.rectangle(1.0, 0.5)                    # no resolution
    raw = LP.Footprint([(100, 0), (0, 100)])
    for f in (raw.inscribed_radius, raw.circumscribed_radius):
        with pytest.raises(ValueError, match="no outline in metres"):
            f()
    assert "InflationConfig.inscribed_radius" in LP.Footprint.inscribed_radius.__doc__


def test_probe_and_config_refusals(LP):
    c = LP.FootprintConfig()
    assert c.foot_lethal == 100 and LP.FootprintConfig.from_any(True) == c and LP.FootprintConfig.from_any(c) is c
    assert LP.FootprintConfig.from_any(c.to_dict()) == c and LP.FootprintConfig(foot_lethal=1).foot_lethal == 1
    for v in (0, 101, 1.0, True, "100", None):
        with pytest.raises(ValueError, match="foot_lethal"):
            LP.FootprintConfig(foot_lethal=v)
    with pytest.raises(ValueError, match="foot_lethall"):
        LP.FootprintConfig.from_any(dict(foot_lethall=3))
    for bad in (None, False, 3, "on"):
        with pytest.raises(ValueError, match="FootprintConfig"):
            LP.FootprintConfig.from_any(bad)
    edge = [(32767, -32767), (-32767, 32767)]
    assert LP.check_probes(edge).tolist() == [list(e) for e in edge]
    for i, v in ((0, 32768), (1, -32768)):
        p = [[0, 0], [0, 0]]
        p[1][i] = v
        with pytest.raises(ValueError, match="probe 1: "):
            LP.check_probes(p)
    for bad, msg in ((np.zeros((0, 2), np.int32), "0 probes"), (np.zeros((257, 2), np.int32), "257 probes"), (np.zeros((2, 3), np.int32), "probes must be integers"),
                     (np.zeros((2, 2)), "probes must be integers"), (np.zeros(2, np.int32), "probes must be integers")):
        with pytest.raises(ValueError, match=msg):
            LP.check_probes(bad)
    b = F.R
    for f in (LP.scores_np, LP.keys_by_sample_np, LP.best_np):
        with pytest.raises(ValueError, match="fcfg without a footprint"):
            f(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, fcfg=True)
        with pytest.raises(ValueError, match="probe 0: "):
            f(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, footprint=[(40000, 0)])
    with pytest.raises(ValueError, match="fcfg without a footprint"):
        LP.score_np(b.grid, b.pot, b.pose, 1000, 0, b.ncfg, b.cfg, fcfg=True)
    # the stand-alone GPU call refuses on the host, before it looks for a library or a device
    g, pot = np.zeros((4, 4), np.int8), np.zeros((4, 4), np.uint32)
    call = lambda **kw: LP.local_plan(g, pot, (0, 0, 0), (0, 0, 0, 0), {}, dict(nv=1, nw=1, steps=1), **kw)      # noqa: E731
    with pytest.raises(ValueError, match="fcfg without a footprint"):
        call(fcfg=True)
    with pytest.raises(ValueError, match="probe 0: "):
        call(footprint=[(0, -32768)])
    with pytest.raises(ValueError, match="foot_lethal = 0"):
        call(footprint=[(0, 0)], fcfg=dict(foot_lethal=0))


# ---- the C-ABI's structure ----
NEW = ["pp_set_local_footprint", "pp_get_local_footprint_config", "pp_get_local_footprint"]


def test_struct_header_exports_and_sources(pp, LP):
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    csrc = os.path.join(os.path.dirname(pp._lib.__file__), "csrc")
    assert ctypes.sizeof(pp._lib.PPLocalFootprintConfig) == 16
    body = hdr[hdr.index("typedef struct pp_local_footprint_config"):hdr.index("} pp_local_footprint_config;")]
    assert [f[0] for f in pp._lib.PPLocalFootprintConfig._fields_] == re.findall(r"^\s+int32_t (\w+)(?:\[3\])?;", body, re.M) == ["foot_lethal", "reserved"]
    api = open(os.path.join(csrc, "api_local_plan.hip")).read()
    assert "static_assert(sizeof(pp_local_footprint_config) == 16" in api
    for size in ("sizeof(pp_local_plan_config) == 32", "sizeof(pp_local_mover_config) == 32", "sizeof(LocalFrame) == 32"):
        assert "static_assert(" + size in api
    assert ctypes.sizeof(pp._lib.PPLocalPlanConfig) == 32 and ctypes.sizeof(pp._lib.PPLocalMoverConfig) == 32
    for name, v in (("PP_LOCAL_MAX_PROBES", 256), ("PP_LOCAL_MAX_PROBE", 32767), ("PP_LOCAL_FOOT_INFO", 4)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr) and getattr(pp._lib, name) == v, name
    assert "#define PP_ABI_VERSION 4" in hdr and "#define PP_LOCAL_RESULT 8 " in hdr
    later = hdr[hdr.index("later additions within 4"):hdr.index("#define PP_ABI_VERSION")]
    for name in ["pp_local_footprint_config", "PP_LOCAL_MAX_PROBES", "PP_LOCAL_MAX_PROBE", "PP_LOCAL_FOOT_INFO", "pp_local_plan_grids_footprint"] + NEW:
        assert re.search(r"\b%s\b" % name, later), name
    assert later.index("pp_frontier_grids") < later.index("PP_LOCAL_MAX_PROBES")
    exp = pp._lib.EXPORTS
    at = exp.index("pp_frontier_grids")
    assert exp[at + 1:at + 5] == NEW + ["pp_local_plan_grids_footprint"]
    for name in NEW:
        assert re.search(r"\bint %s\(pp_handle" % name, hdr), name
    assert re.search(r"\bint pp_local_plan_grids_footprint\(int device", hdr)
    assert not re.search(r"\bint pp_local_plan\w*foot\w*_async\(", hdr)                   # no third and fourth async entry
    src = pp._lib.SOURCES
    assert src[src.index("local_plan.hip") + 1] == "local_movers.hip" and src[-2:] == ["api_track.hip", "track.hip"]
    assert not any("foot" in s for s in src)                # no new translation unit was needed
    for name in ("Footprint", "FootprintConfig", "check_probes", "start_probe_np"):
        assert callable(getattr(LP, name)), name
    for name in ("set_local_footprint", "local_footprint_config", "local_footprint"):
        assert callable(getattr(pp.Engine, name)), name
    # opt-in at run time only: no configuration key, no environment switch
    assert "FOOT" not in open(os.path.join(csrc, "pp_switches.h")).read().upper()
    assert "getenv" not in api and "getenv" not in open(os.path.join(csrc, "local_plan.hip")).read()
    doc = re.sub(r"\s+", " ", LP.__doc__)
    for what in ("footprints other than a point", "unless a footprint is set", "filled footprints", "swept between two steps", "footprint-aware inflation",
                 "circumscribed circle free", "rectangular movers", "escaping from state 5", "holonomic samples", "the outline cannot jump an obstacle cell",
                 "4, 3, 2, 5, 1, 0", "Probes never contribute to occ"):
        assert what in doc, what


def test_exported_from_the_library_and_null_handle(pp, LP, hip_lib):
    for name in NEW + ["pp_local_plan_grids_footprint"]:
        assert hasattr(hip_lib, name), name
    PP_ERR_ARG = 1
    fc = pp._lib.PPLocalFootprintConfig(100, (0, 0, 0))
    on = ctypes.c_int32(7)
    probes = np.array([[100, 0], [0, 100]], np.int32)
    assert hip_lib.pp_set_local_footprint(None, 0, ctypes.byref(fc), probes.ctypes.data, 2) == PP_ERR_ARG
    assert hip_lib.pp_get_local_footprint_config(None, 0, ctypes.byref(on), None, None, None) == PP_ERR_ARG and on.value == 7
    assert hip_lib.pp_get_local_footprint(None, 0, None, 1) == PP_ERR_ARG
    # the stand-alone call refuses its arguments before it looks for a device
    c = pp._lib.PPLocalPlanConfig(3, 3, 2, 0, 1, 0, 1, 1)
    n = pp._lib.PPNavfnConfig(99, 10, 1, 0, 50, 8, 1024, 0)
    trig = np.ascontiguousarray(LP.trig_table())
    g, pot = np.zeros((2, 2), np.int8), np.zeros((2, 2), np.uint32)
    three, four = np.zeros((1, 3), np.int32), np.zeros((1, 4), np.int32)
    table = np.zeros((1, 64, 6), np.int32)

    def call(probes=probes, n_probes=2, foot_lethal=100, probe=None, movers=None, n_movers=0, horizon=4):
        t = probes if probe is None else probes.copy()
        if probe is not None:
            t[1] = probe
        nm = np.array([n_movers], np.int32)
        P = lambda a: None if a is None else a.ctypes.data      # noqa: E731
        st = hip_lib.pp_local_plan_grids_footprint(0, P(g), P(pot), 1, 2, 2, ctypes.byref(n), ctypes.byref(c), P(trig), 4096, P(three), P(four), None,
                                                   horizon, 5, P(movers), P(nm), P(t), n_probes, foot_lethal, None, None, None, None, None, None)
        return st, (hip_lib.pp_last_error(None) or b"").decode()

    for kw, what in ((dict(probes=None), "probes is NULL"), (dict(n_probes=0), "n_probes = 0"), (dict(n_probes=257), "n_probes = 257"),
                     (dict(n_probes=-1), "n_probes = -1"), (dict(foot_lethal=0), "foot_lethal = 0"), (dict(foot_lethal=101), "foot_lethal = 101"),
                     (dict(probe=(32768, 0)), "probe 1: (32768, 0)"), (dict(probe=(0, -32768)), "probe 1: (0, -32768)"),
                     (dict(probe=(-2 ** 31, 0)), "probe 1: "), (dict(movers=table, horizon=257), "horizon = 257"),
                     (dict(movers=table, n_movers=65), "n_movers = 65")):
        st, msg = call(**kw)
        assert st == PP_ERR_ARG and "pp_local_plan_grids_footprint" in msg and what in msg, (kw, msg)


# ---- behaviour: the doorway ----
def test_the_doorway_separates_the_two_rules(pp, LP):
    """A wall with a door of 0.8 m; the robot, 0.9 m x 0.5 m, stands in it, facing through, on a grid inflated by its
    inscribed radius.  The point rule lets it turn in the door; its corners would sweep through the wall."""
    c = F.case("doorway")
    b = c.base
    assert abs(F.DOOR_INFL["inscribed_radius"] - F.RECT.inscribed_radius()) == 0.0 and F.RES == 0.1
    door = np.flatnonzero(F.DOOR_GRID[:, 31] < 99)
    assert len(np.flatnonzero(F._DOOR_RAW[:, 31] == 0)) == 8 and len(door) < 8             # 0.8 m, of which inflation leaves the centre less
    point, foot = F.reasons(c.name, footprint=False), F.reasons(c.name)
    turned = np.flatnonzero((point == LP.OK) & (foot == LP.FOOTPRINT))
    both = np.flatnonzero((point == LP.OK) & (foot == LP.OK))
    print("doorway: point ok", int((point == LP.OK).sum()), "-> footprint", len(turned), "; ok under both", len(both))
    assert len(turned) >= 1 and len(both) >= 1
    assert all(LP.sample(s, b.window, b.cfg)[1] != 0 for s in turned)                      # every one of them turns
    straight = [s for s in range(len(point)) if LP.sample(s, b.window, b.cfg)[1] == 0]
    assert len(straight) == b.cfg["nv"] and all(point[s] == LP.OK and foot[s] == LP.OK for s in straight)
    # nothing else changed: a sample ends otherwise under the footprint only if it ended so under the point rule
    assert ((foot == point) | (foot == LP.FOOTPRINT)).all()
    # the corners of a turned sample meet an obstacle cell itself, not its ring
    for s in turned:
        poses = LP.score_np(b.grid, b.pot, b.pose, *LP.sample(s, b.window, b.cfg), b.ncfg, b.cfg, None, None, c.probes)[2]
        cx, cy = F.first_bad(c, poses[-1])[1]
        assert F.DOOR_GRID[cy, cx] == 100 and F._DOOR_RAW[cy, cx] == 100
    # the footprint command's whole trajectory keeps every probe off cells that read 100
    r = F.reference(c.name)
    assert r["cmd_state"] == 0 and len(r["traj"]) == b.cfg["steps"] + 1
    n = pp.navfn.NavfnConfig.from_any(b.ncfg)
    for X, Y, h in r["traj"].tolist():
        for fx, fy in c.probes.tolist():
            cx, cy = LP._probe_cell(X, Y, h, fx, fy)
            assert 0 <= cx < 64 and 0 <= cy < 64 and F.DOOR_GRID[cy, cx] < 100
    assert n.lethal_cost == 99 and LP.FootprintConfig().foot_lethal == 100      # the centre keeps off the ring, the corners may enter it


def test_the_half_diagonal_does_not_fit_the_door(pp, LP):
    """The other choice the point rule leaves: inflated by the circumscribed radius, the door is closed to the centre."""
    wide = pp.inflation.inflate_np(F._DOOR_RAW, dict(F.DOOR_INFL, inscribed_radius=F.RECT.circumscribed_radius(), inflation_radius=0.6))
    assert (wide[:, 31] >= 99).all() and (F.DOOR_GRID[:, 31] < 99).any()


def test_movers_cases_are_unchanged_by_footprint_none(LP):
    """footprint=None is the default everywhere: one movers case through the new signature."""
    c = M.case("a_crossing")
    b = c.base
    a = LP.best_np(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, b.goal_state, None, c.movers, c.mcfg)
    z = LP.best_np(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, b.goal_state, None, c.movers, c.mcfg, None, None)
    assert set(a) == set(z) == set(M.reference("a_crossing")) and all(np.array_equal(a[k], z[k]) for k in a)
