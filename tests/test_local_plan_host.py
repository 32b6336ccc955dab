"""local_planner.py's rule on the CPU: the pinned window with its keys worked out by hand, the step-by-step statement
against the all-samples-at-once statement on every shared case (tests/local_plan_cases.py), the trig table's symmetries,
the bounds, the dynamic window's limits, the validation and the C-ABI's structure.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import local_plan_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGES = [("nv", 1, 16384), ("nw", 1, 16384), ("steps", 1, 256), ("lookahead", 0, 16384), ("pot_weight", 0, 255),
          ("occ_weight", 0, 65535), ("speed_weight", 0, 65535), ("turn_weight", 0, 65535)]


@pytest.fixture(scope="module")
def LP(pp):
    return pp.local_planner


# ---- the rule ----
def test_pinned_window_key_by_key(pp, LP):
    """5 x 5 cells, (3, 3) blocked, the goal at (4, 2); the robot at the centre of (1, 2) along +x; sv 0, 512, 1024 and sw
    -512, 0, 512 (an eighth of a turn per step), 2 steps; the weights 1, 0, 1, 1.  Step 1 moves sv along +x exactly
    (C[0] = 16384, S[0] = 0).  Step 2 runs under heading 0 or +-512, where C = S = 11585: (512 * 11585 + 8192) >> 14 = 362,
    (-512 * 11585 + 8192) >> 14 = -362, and 724 / -724 for sv = 1024.  The field: 50 per orthogonal and 70 per diagonal
    move of a free cell."""
    g = np.zeros((5, 5), np.int8)
    g[3, 3] = 100
    pot = pp.navfn.navfn_np(g, (4, 2), {})
    assert (pot[2, 1], pot[2, 2], pot[2, 3], pot[1, 3]) == (150, 100, 50, 70) and pot[3, 3] == pp.navfn.UNREACHED
    assert LP.trig_table()[512].tolist() == [11585, 11585] and LP.trig_table()[3584].tolist() == [11585, -11585]
    pose = (1 * 1024 + 512, 2 * 1024 + 512, 0)
    cfg = dict(nv=3, nw=3, steps=2, lookahead=0, pot_weight=1, occ_weight=0, speed_weight=1, turn_weight=1)
    window = (0, 512, -512, 512)
    # sample:  sv, sw -> end (X, Y), cell, pot + (1024 - |sv|) + |sw|
    scores = [150 + 1024 + 512,     # 0:    0, -512 -> (1536, 2560) (1, 2)
              150 + 1024 + 0,       # 1:    0,    0
              150 + 1024 + 512,     # 2:    0,  512
              100 + 512 + 512,      # 3:  512, -512 -> (2048 + 362, 2560 - 362) = (2410, 2198) (2, 2)
              100 + 512 + 0,        # 4:  512,    0 -> (2560, 2560) (2, 2)
              100 + 512 + 512,      # 5:  512,  512 -> (2410, 2922) (2, 2)
              70 + 0 + 512,         # 6: 1024, -512 -> (2560 + 724, 2560 - 724) = (3284, 1836) (3, 1)
              50 + 0 + 0,           # 7: 1024,    0 -> (3584, 2560) (3, 2)
              None]                 # 8: 1024,  512 -> (3284, 3284) (3, 3): blocked
    want = np.array([LP.INVALID if s is None else (s << 14) | i for i, s in enumerate(scores)], np.uint64)
    for how in (LP.scores_np, LP.keys_by_sample_np):
        keys, reasons = how(g, pot, pose, window, {}, cfg)
        assert keys.dtype == np.uint64 and np.array_equal(keys, want), how.__name__
        assert reasons.tolist() == [0] * 8 + [LP.COLLISION]
        r = LP.best_np(g, pot, pose, window, {}, cfg, samples=how)
        assert {k: r[k] for k in LP.RESULT} == dict(cmd_state=0, best=7, sv=1024, sw=0, n_ok=8, n_outside=0, n_collision=1, n_unreached=0)
        assert r["score"] == 50 and r["traj"].dtype == np.int32
        assert r["traj"].tolist() == [[1536, 2560, 0], [2560, 2560, 0], [3584, 2560, 0]]
    assert LP.score_np(g, pot, pose, 1024, -512, {}, cfg)[2] == [(1536, 2560, 0), (2560, 2560, 3584), (3284, 1836, 3072)]


@pytest.mark.parametrize("name", K.NAMES)
def test_step_by_step_equals_all_at_once(LP, name):
    c = K.case(name)
    keys, reasons = LP.scores_np(c.grid, c.pot, c.pose, c.window, c.ncfg, c.cfg)
    keys1, reasons1 = LP.keys_by_sample_np(c.grid, c.pot, c.pose, c.window, c.ncfg, c.cfg)
    assert np.array_equal(keys, keys1) and np.array_equal(reasons, reasons1)
    a = K.reference(name)
    b = LP.best_np(c.grid, c.pot, c.pose, c.window, c.ncfg, c.cfg, c.goal_state, samples=LP.keys_by_sample_np)
    assert set(a) == set(b) == set(LP.RESULT) | {"score", "traj", "keys"}
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["traj"].shape == ((c.cfg["steps"] + 1, 3) if a["cmd_state"] == 0 else (0, 3))
    if a["cmd_state"] >= 2:
        assert (a["keys"] == LP.INVALID).all()


def test_batch_reference(LP):
    for b in range(3):
        r = K.batch_reference(b)
        k, _ = LP.keys_by_sample_np(K.BATCH[b], K.BATCH_POTS[b], K.BATCH_POSES[b], K.BATCH_WINDOWS[b], K.BATCH_NCFG, K.BATCH_CFG)
        assert np.array_equal(r["keys"], k)


def test_trig_table_symmetries(LP):
    t = LP.trig_table()
    assert t.dtype == np.int32 and t.shape == (4096, 2) and LP.HEADINGS == 4096 and LP.SUB == 1024 and LP.ONE == 16384
    C, S = t[:, 0], t[:, 1]
    h = np.arange(4096)
    assert np.array_equal(C, S[(h + 1024) & 4095])
    assert C[0] == 16384 and S[0] == 0 and S[1024] == 16384 and C[1024] == 0
    assert np.array_equal(C[(h + 2048) & 4095], -C) and np.array_equal(S[(h + 2048) & 4095], -S)      # half a turn flips the signs
    assert np.array_equal(C[(-h) & 4095], C) and np.array_equal(S[(-h) & 4095], -S)
    assert np.abs(t).max() == 16384 and np.abs(C.astype(np.int64) ** 2 + S.astype(np.int64) ** 2 - 2 ** 28).max() < 2 ** 15
    assert np.array_equal(t, np.rint(np.stack([np.cos(2 * np.pi * h / 4096), np.sin(2 * np.pi * h / 4096)], 1) * 16384).astype(np.int32))


def test_bounds(pp, LP):
    assert LP.MAX_SCORE == 255 * (2 ** 32 - 2) + 65535 * (100 + 1024 + 512) < 2 ** 41
    assert ((LP.MAX_SCORE << 14) | 16383) < LP.INVALID == 2 ** 64 - 1
    assert (pp._lib.PP_OCC_MAX_CELLS + 1) * 1024 + 16384 < 2 ** 31
    assert 1024 * 16384 + 8192 < 2 ** 31 and 16384 * 16384 + 8192 < 2 ** 31
    # a step never moves more than one cell along an axis
    t = LP.trig_table().astype(np.int64)
    for sv in (1024, -1024):
        assert np.abs((sv * t + 8192) >> 14).max() == 1024
    # occ never passes 100: an unblocked known cell is below lethal_cost <= 100, unknown_cost is at most 100
    assert [r for r in pp.navfn._RANGES if r[0] in ("lethal_cost", "unknown_cost")] == [("lethal_cost", 1, 100), ("unknown_cost", 0, 100)]
    csrc = os.path.join(os.path.dirname(pp._lib.__file__), "csrc")
    src = open(os.path.join(csrc, "local_plan.hip")).read()
    assert "< (1ull << 41)" in src and "< (1ll << 31)" in src and src.count("static_assert") >= 6
    assert "float" not in re.sub(r"//.*", "", src) and "double" not in src


def test_window_stays_inside_the_limits(LP):
    rng = np.random.default_rng(5)
    for _ in range(300):
        v_max = rng.uniform(0.1, 3.0)
        lim = LP.LocalLimits(v_min=-rng.uniform(0.0, 1.0) * v_max * rng.integers(0, 2), v_max=v_max, w_max=rng.uniform(0.0, 4.0),
                             acc_v=rng.uniform(0.0, 5.0), acc_w=rng.uniform(0.0, 10.0), sim_time=rng.uniform(0.2, 5.0),
                             period=rng.uniform(0.01, 0.5))
        res = rng.choice([0.02, 0.05, 0.1, 0.25])
        nv, nw = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        v, w = rng.uniform(lim.v_min - 0.2, lim.v_max + 0.2), rng.uniform(-lim.w_max - 0.5, lim.w_max + 0.5)
        win = lim.window(v, w, nv, nw, res)
        assert all(isinstance(x, int) for x in win)
        v0, dv, w0, dw = LP.check_window(win, dict(nv=nv, nw=nw))
        dt = lim.step_dt(res)
        assert dt == res / max(abs(lim.v_min), abs(lim.v_max)) and 1 <= lim.steps(res) <= 256
        sv = v0 + np.arange(nv) * dv
        sw = w0 + np.arange(nw) * dw
        assert dv >= 0 and dw >= 0 and np.abs(sv).max() <= 1024 and np.abs(sw).max() <= 512
        mv, mw = LP.command_metric(sv, sw, res, dt)
        assert mv.min() >= lim.v_min - 1e-9 and mv.max() <= lim.v_max + 1e-9
        assert np.abs(mw).max() <= lim.w_max + 1e-9
    lim = LP.LocalLimits(v_min=-0.2, v_max=0.5, w_max=1.0, acc_v=10.0, acc_w=100.0, sim_time=2.0, period=0.1)
    assert lim.step_dt(0.05) == 0.1 and lim.steps(0.05) == 20
    assert lim.window(0.0, 0.0, 8, 9, 0.05) == (-409, 204, -65, 16)          # 0.2 / 0.5 * 1024 = 409.6, 1.0 * 0.1 / 2 pi * 4096 = 65.19
    v, w = LP.command_metric(1024, 65, 0.05, 0.1)
    assert v == 0.5 and abs(w - 65 * 2 * np.pi / 4096 / 0.1) < 1e-12
    for bad in (dict(v_min=1.0, v_max=0.5), dict(v_min=0.0, v_max=0.0), dict(w_max=-1.0), dict(period=0.0), dict(sim_time=float("nan"))):
        with pytest.raises(ValueError, match="LocalLimits"):
            LP.LocalLimits(**bad)


def test_pose_ticks(LP):
    p = LP.pose_ticks([[0.0, 0.0], [0.126, -0.01], [np.nan, 0.0], [1e9, 0.0]], [0.0, np.pi / 2, 0.0, -np.pi / 2], (-0.125, -0.75), 0.0625)
    assert p.dtype == np.int32 and p.shape == (4, 3)
    assert p[0].tolist() == [2048, 12288, 0] and p[1].tolist() == [4112, 12124, 1024]      # 0.251 and 0.74 m at 16384 sub-cells per metre
    assert p[2].tolist() == [-1024, -1024, 0] and p[3].tolist() == [2 ** 30, 12288, 3072]
    assert LP.pose_ticks((0.0, 0.0), -1e-9, (0.0, 0.0), 1.0)[0].tolist() == [0, 0, 0]
    assert LP.pose_ticks((0.0, 0.0), 2 * np.pi - 1e-9, (0.0, 0.0), 1.0)[0, 2] == 0


# ---- validation ----
def test_config_ranges_are_refused_by_name(LP):
    C = LP.LocalPlanConfig
    assert [r[0] for r in LP._RANGES] == [r[0] for r in RANGES] and [tuple(r) for r in LP._RANGES] == RANGES
    for f, lo, hi in RANGES:
        for v in (lo - 1, hi + 1):
            with pytest.raises(ValueError, match=rf"LocalPlanConfig: {f} = {v} outside \[{lo}, {hi}\]"):
                C(**{f: v})
        with pytest.raises(ValueError, match=f"{f} must be an integer"):
            C(**{f: 1.5})
    with pytest.raises(ValueError, match="nv \\* nw = 16512 samples, at most PP_LOCAL_MAX_SAMPLES = 16384"):
        C(nv=129, nw=128)
    assert C(nv=128, nw=128).nv == 128
    with pytest.raises(ValueError, match="unknown keys \\['speed'\\]"):
        C.from_any(dict(speed=1))
    assert C.from_any(True) == C() and C.from_any(C(nv=3).to_dict()) == C(nv=3) and list(C().to_dict()) == [r[0] for r in RANGES]
    g, pot = K.case("samples_63").grid, K.case("samples_63").pot
    for win, msg in (((1000, 5, 0, 0), "sv runs from 1000 to 1030"), ((-1025, 0, 0, 0), "sv runs from -1025"),
                     ((0, 0, 0, 65), "sw runs from 0 to 520"), ((0, 0, -513, 1), "sw runs from -513")):
        for call in (lambda: LP.scores_np(g, pot, (0, 0, 0), win, {}, dict(nv=7, nw=9)),
                     lambda: LP.local_plan(g, pot, (0, 0, 0), win, {}, dict(nv=7, nw=9))):
            with pytest.raises(ValueError, match=msg):
                call()
    with pytest.raises(ValueError, match="int8"):
        LP.scores_np(np.zeros((2, 2), np.int16), pot, (0, 0, 0), (0, 0, 0, 0), {}, True)
    with pytest.raises(ValueError, match="pots must be uint32 of the grids' shape"):
        LP.local_plan(g, pot[:5], (0, 0, 0), (0, 0, 0, 0), {}, True)
    with pytest.raises(ValueError, match="poses must be integers"):
        LP.local_plan(g, pot, (0.5, 0, 0), (0, 0, 0, 0), {}, True)


# ---- structure ----
NEW = ["pp_set_local_plan", "pp_get_local_plan_config", "pp_local_plan_async", "pp_get_local_plan"]


def test_struct_header_exports_and_sources(pp, LP):
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    body = re.search(r"typedef struct pp_local_plan_config \{(.*?)\} pp_local_plan_config;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(int32_t)\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [n for _, n in fields] == [n for n, _ in pp._lib.PPLocalPlanConfig._fields_] == [r[0] for r in RANGES]
    assert 4 * len(fields) == ctypes.sizeof(pp._lib.PPLocalPlanConfig) == 32
    csrc = os.path.join(os.path.dirname(pp._lib.__file__), "csrc")
    api = open(os.path.join(csrc, "api_local_plan.hip")).read()
    assert "static_assert(sizeof(pp_local_plan_config) == 32" in api and "static_assert(sizeof(LocalCall) == 32" in api
    for name, v in (("PP_LOCAL_SUB", 1024), ("PP_LOCAL_HEADINGS", 4096), ("PP_LOCAL_MAX_SAMPLES", 16384), ("PP_LOCAL_MAX_STEPS", 256),
                    ("PP_LOCAL_MAX_LOOKAHEAD", 16384), ("PP_LOCAL_RESULT", 8)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr) and getattr(pp._lib, name) == v, name
    assert len(LP.RESULT) == pp._lib.PP_LOCAL_RESULT
    assert "#define PP_ABI_VERSION 4" in hdr and ctypes.sizeof(pp._lib.PPNavfnConfig) == 32
    later = hdr[hdr.index("later additions within 4"):hdr.index("#define PP_ABI_VERSION")]
    for name in ["pp_local_plan_config", "PP_LOCAL_SUB", "PP_LOCAL_HEADINGS", "pp_local_plan_grids"] + NEW:
        assert re.search(r"\b%s\b" % name, later), name
    exp = pp._lib.EXPORTS
    at = exp.index("pp_navfn_grids")
    assert exp[at + 1:at + 6] == NEW + ["pp_local_plan_grids"]
    for name in NEW:
        assert re.search(r"\bint %s\(pp_handle" % name, hdr), name
    assert re.search(r"\bint pp_local_plan_grids\(int device", hdr)
    src = pp._lib.SOURCES
    at = src.index("navfn.hip")
    assert src[at + 1:at + 3] == ["api_local_plan.hip", "local_plan.hip"] and src[-2:] == ["api_track.hip", "track.hip"]
    assert "local_planner" in pp.__all__
    for name in ("LocalPlanConfig", "LocalLimits", "trig_table", "score_np", "scores_np", "best_np", "pose_ticks", "command_metric", "local_plan"):
        assert callable(getattr(LP, name)), name
    for name in ("set_local_planner", "local_planner_config", "local_plan_async", "local_commands", "local_trajectories", "local_keys",
                 "local_plan_info", "drive"):
        assert callable(getattr(pp.Engine, name)), name
    assert callable(pp.VoxelNet.drive)
    # opt-in at run time only: no configuration key, no environment switch
    assert not hasattr(pp.config.Derived(pp.config.tiny_config(1)), "local_planner")
    assert "LOCAL" not in open(os.path.join(csrc, "pp_switches.h")).read().upper()
    for f in ("api_local_plan.hip", "local_plan.hip"):
        assert "getenv" not in open(os.path.join(csrc, f)).read()
    assert "local_plan_release(e);" in open(os.path.join(csrc, "pp_api.hip")).read()
    # the docstring lists what is out of scope, and navfn.py no longer disclaims this stage
    doc = LP.__doc__
    for what in ("escaping from a blocked pose", "footprints other than a point", "holonomic", "oscillation suppression",
                 "goal-orientation alignment", "touch only at a corner", "a configuration key", "any ROS import"):
        assert what in doc, what
    assert "a local planner or velocity commands" not in pp.navfn.__doc__


def test_exported_from_the_library_and_null_handle(pp, LP, hip_lib):
    for name in NEW + ["pp_local_plan_grids"]:
        assert hasattr(hip_lib, name), name
    PP_ERR_ARG = 1
    c = pp._lib.PPLocalPlanConfig(3, 3, 2, 0, 1, 0, 1, 1)
    n = pp._lib.PPNavfnConfig(99, 10, 1, 0, 50, 8, 1024, 0)
    trig = np.ascontiguousarray(LP.trig_table())
    on = ctypes.c_int32(7)
    three, four = np.zeros((1, 3), np.int32), np.zeros((1, 4), np.int32)
    assert hip_lib.pp_set_local_plan(None, 0, ctypes.byref(c), trig.ctypes.data, 4096) == PP_ERR_ARG
    assert hip_lib.pp_get_local_plan_config(None, 0, ctypes.byref(on), None) == PP_ERR_ARG and on.value == 7
    assert hip_lib.pp_local_plan_async(None, 0, three.ctypes.data, four.ctypes.data, 1) == PP_ERR_ARG
    assert hip_lib.pp_get_local_plan(None, 0, None, None, None, None, 1) == PP_ERR_ARG
    # the stand-alone call refuses its arguments before it looks for a device
    g, pot = np.zeros((2, 2), np.int8), np.zeros((2, 2), np.uint32)

    def call(grids=g, pots=pot, batch=1, H=2, W=2, ncfg=n, cfg=c, table=trig, n_trig=4096, poses=three, windows=four):
        P = lambda a: None if a is None else a.ctypes.data      # noqa: E731
        return hip_lib.pp_local_plan_grids(0, P(grids), P(pots), batch, H, W, ctypes.byref(ncfg), ctypes.byref(cfg), P(table), n_trig,
                                           P(poses), P(windows), None, None, None, None, None)

    for kw, msg in ((dict(grids=None), b"grids, pots, navfn_cfg or cfg is NULL"), (dict(pots=None), b"grids, pots, navfn_cfg or cfg is NULL"),
                    (dict(poses=None), b"poses or windows is NULL"), (dict(windows=None), b"poses or windows is NULL"),
                    (dict(batch=0), b"batch = 0"), (dict(H=1025, W=1024), b"PP_OCC_MAX_CELLS"),
                    (dict(table=None), b"trig is NULL"), (dict(n_trig=4095), b"the trig table has 4095 entries, it must have PP_LOCAL_HEADINGS = 4096"),
                    (dict(windows=np.array([[1000, 20, 0, 0]], np.int32)), b"grid 0: sv runs from 1000 to 1040, outside [-1024, 1024]"),
                    (dict(windows=np.array([[0, 0, -512, 513]], np.int32)), b"grid 0: sw runs from -512 to 514, outside [-512, 512]")):
        assert call(**kw) == PP_ERR_ARG, kw
        assert msg in hip_lib.pp_last_error(None), (kw, hip_lib.pp_last_error(None))
    bad = trig.copy()
    bad[77, 1] = 16385
    assert call(table=bad) == PP_ERR_ARG and b"trig[77] = (" in hip_lib.pp_last_error(None) and b"outside [-16384, 16384]" in hip_lib.pp_last_error(None)
    for field, v, msg in (("nv", 0, b"nv = 0 outside [1, 16384]"), ("steps", 257, b"steps = 257 outside [1, 256]"),
                          ("lookahead", 16385, b"lookahead = 16385 outside [0, 16384]"), ("pot_weight", 256, b"pot_weight = 256 outside [0, 255]"),
                          ("occ_weight", 65536, b"occ_weight = 65536 outside [0, 65535]"), ("turn_weight", -1, b"turn_weight = -1 outside [0, 65535]")):
        b = pp._lib.PPLocalPlanConfig(3, 3, 2, 0, 1, 0, 1, 1)
        setattr(b, field, v)
        assert call(cfg=b) == PP_ERR_ARG and msg in hip_lib.pp_last_error(None), hip_lib.pp_last_error(None)
    assert call(cfg=pp._lib.PPLocalPlanConfig(129, 128, 2, 0, 1, 0, 1, 1)) == PP_ERR_ARG
    assert b"nv * nw = 16512 samples, at most PP_LOCAL_MAX_SAMPLES = 16384" in hip_lib.pp_last_error(None)
    assert call(ncfg=pp._lib.PPNavfnConfig(101, 10, 1, 0, 50, 8, 1024, 0)) == PP_ERR_ARG and b"lethal_cost = 101" in hip_lib.pp_last_error(None)
