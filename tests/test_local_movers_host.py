"""The movers of local_planner.py on the CPU: the step-by-step statement against the all-samples-at-once statement on every
shared case (tests/local_mover_cases.py, whose import asserts the properties the cases are named for); movers=None against
what the functions returned before the movers existed (tests/golden/local_plan_parent.json, recorded from that commit);
`movers_np` on hand-made track rows; the refusals; the C-ABI's structure.  No GPU."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest

import local_mover_cases as M
import local_plan_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def LP(pp):
    return pp.local_planner


# ---- the rule ----
@pytest.mark.parametrize("name", M.NAMES)
def test_step_by_step_equals_all_at_once(LP, name):
    c, b = M.case(name), M.case(name).base
    keys, reasons = LP.scores_np(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, c.movers, c.mcfg)
    keys1, reasons1 = LP.keys_by_sample_np(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, c.movers, c.mcfg)
    assert np.array_equal(keys, keys1) and np.array_equal(reasons, reasons1)
    want = M.reference(name)
    got = M._best(b, c.movers, c.mcfg, samples=LP.keys_by_sample_np)
    assert set(want) == set(got) == set(LP.RESULT) | {"score", "traj", "keys", "n_movers", "n_dynamic", "near"}
    for k in want:
        assert np.array_equal(want[k], got[k]), k
    if want["cmd_state"] < 2:
        assert np.array_equal(want["keys"], keys) and want["n_dynamic"] == int((reasons == LP.DYNAMIC).sum())
    if want["cmd_state"] == 0:                              # the winner's score carries its near
        sv, sw = LP.sample(want["best"], b.window, b.cfg)
        plain_score = LP.score_np(b.grid, b.pot, b.pose, sv, sw, b.ncfg, b.cfg)[1]
        assert want["score"] == plain_score + c.mcfg["mover_weight"] * want["near"]


def test_batch_reference(LP):
    for b in range(3):
        k, _ = LP.keys_by_sample_np(K.BATCH[b], K.BATCH_POTS[b], K.BATCH_POSES[b], K.BATCH_WINDOWS[b], K.BATCH_NCFG, K.BATCH_CFG,
                                    M.BATCH_MOVERS[b, :M.BATCH_N[b]], M.BATCH_MCFG)
        assert np.array_equal(M.batch_reference(b)["keys"], k)


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_without_movers_nothing_changed(LP):
    """scores_np, best_np and score_np with movers=None on every case of local_plan_cases.py against the digests recorded
    from the commit before the movers: the same values, the same dict keys, the same tuple."""
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "local_plan_parent.json")))
    assert sorted(want) == sorted(K.NAMES)
    for c in K.CASES:
        w = want[c.name]
        keys, reasons = LP.scores_np(c.grid, c.pot, c.pose, c.window, c.ncfg, c.cfg)
        assert _digest(keys, reasons) == w["scores"], c.name
        r = LP.best_np(c.grid, c.pot, c.pose, c.window, c.ncfg, c.cfg, c.goal_state)
        assert sorted(r) == w["dict_keys"] and {k: int(r[k]) for k in LP.RESULT + ("score",)} == w["best"], c.name
        assert _digest(r["traj"]) == w["traj"], c.name
        out = LP.score_np(c.grid, c.pot, c.pose, *LP.sample(0, c.window, c.cfg), c.ncfg, c.cfg)
        assert len(out) == 3 and [out[0], out[1], _digest(np.array(out[2], np.int64))] == w["sample_0"], c.name
    c = K.case("samples_65")                                # (keys_by_sample_np is score_np per sample: one case suffices)
    assert _digest(*LP.keys_by_sample_np(c.grid, c.pot, c.pose, c.window, c.ncfg, c.cfg)) == want["samples_65"]["scores"]


def test_bounds(pp, LP):
    assert LP.DYNAMIC == 4 and LP.MAX_SCORE < LP.MAX_SCORE_MOVERS == LP.MAX_SCORE + 65535 * 256 < 2 ** 41
    assert ((LP.MAX_SCORE_MOVERS << 14) | 16383) < LP.INVALID
    # near <= horizon + 1 - 1; a mover's position and dx fit int32 and d2 int64 (X is compared inside the grid only)
    pos = 2 ** 29 + 256 * 16384
    dx = pp._lib.PP_OCC_MAX_CELLS * 1024 + pos
    assert pos < 2 ** 31 and dx < 2 ** 31 and 2 * dx * dx < 2 ** 63 and 32767 ** 2 < 2 ** 31
    csrc = os.path.join(os.path.dirname(pp._lib.__file__), "csrc")
    src = open(os.path.join(csrc, "local_plan.hip")).read()
    assert "65535ull * PP_LOCAL_MAX_STEPS < (1ull << 41)" in src and "d2 fits int64" in src and src.count("static_assert") >= 10
    assert "template <bool MOVERS>" in src and "k_local_rollout<false>" in src and "k_local_rollout<true>" in src
    mov = open(os.path.join(csrc, "local_movers.hip")).read()
    assert "PP_TRACK_MAX == 64 && PP_WAVE == 64" in mov and "atomic" not in re.sub(r"//.*", "", mov)
    for f in ("sqrt", "sin(", "cos(", "atan"):
        assert f not in re.sub(r"//.*", "", mov), f


# ---- from tracks to movers ----
def _rows(pp, n):
    r = np.zeros(n, pp.tracking.TRACK_DTYPE)
    r["confirmed"] = 1
    r["size"] = (0.6, 0.8, 1.7)
    return r


CFG = dict(horizon=16, mover_weight=64, pad_hard=0.25, pad_soft=0.5, confirmed_only=True)


def test_movers_np_by_hand(pp, LP):
    """res 0.25 m, dt 0.125 s, origin (-4, -8): exactly representable, so every value below is worked out by hand."""
    r = _rows(pp, 6)
    r["state"][0, :6] = (1.0, 2.0, 0.3, 0.5, -1.0, 0.0)     # MX = (1 + 4) / 0.25 * 1024 = 20480, MY = 40960
    r["state"][1, :6] = (-4.5, -8.0, 0.0, 0.0, 0.0, 0.0)    # x - ox = -0.5 -> -2048; y - oy = 0 -> 0
    r["confirmed"][2] = 0                                   # unconfirmed
    r["state"][3, :6] = (-4.0 - 0.25 / 1024 / 2, 0.0, 0.0, 0.0, 0.0, 0.0)      # half a sub-cell below the origin: floor -> -1
    r["state"][4, :6] = (0.0, 0.0, 0.0, 0.25 / 1024 * 8 * 2.5, 0.25 / 1024 * 8 * 3.5, -0.25 / 1024 * 8 * 0.5)   # vx * dt / res * 1024 = 2.5, 3.5
    r["state"][5, :6] = (0.0, 0.0, 0.0, -0.25 / 1024 * 8 * 2.5, -0.25 / 1024 * 8 * 0.5, 0.0)                       # -2.5, -0.5
    r["size"][5] = (100.0, 3.0, 1.0)                        # a radius that clips
    m, n, skipped = LP.movers_np(r, 6, (-4.0, -8.0), 0.25, 0.125, CFG)
    assert m.dtype == np.int32 and m.shape == (64, 6) and (n, skipped) == (5, 0)
    # vx * dt / res * 1024 = 0.5 * 0.125 / 0.25 * 1024 = 256; radii: (0.4 + 0.25) / 0.25 * 1024 = 2662.4 -> 2663, (0.4 + 0.5) -> 3686.4 -> 3687
    assert m[0].tolist() == [20480, 40960, 256, -512, 2663, 3687]
    assert m[1].tolist() == [-2048, 0, 0, 0, 2663, 3687]
    assert m[2].tolist() == [-1, 32768, 0, 0, 2663, 3687]
    assert m[3, 2:4].tolist() == [2, 4] and m[4, 2:4].tolist() == [-2, 0]       # ties go to even
    assert m[4, 4:].tolist() == [32767, 32767] and not m[5:].any()
    # every row counts where confirmed_only is off; rows behind n are not read
    m2, n2, _ = LP.movers_np(r, 6, (-4.0, -8.0), 0.25, 0.125, dict(CFG, confirmed_only=False))
    assert n2 == 6 and np.array_equal(m2[[0, 1, 3, 4, 5]], m[:5]) and m2[2, :2].tolist() == [16384, 32768]
    r2 = np.concatenate([r[:2], _rows(pp, 3)])
    r2["state"][2:, 0] = np.nan
    m3, n3, s3 = LP.movers_np(r2, 2, (-4.0, -8.0), 0.25, 0.125, CFG)
    assert (n3, s3) == (2, 0) and np.array_equal(m3, np.vstack([m[:2], np.zeros((62, 6), np.int32)]))
    # no posed step: no movers
    m4, n4, s4 = LP.movers_np(r, -1, (-4.0, -8.0), 0.25, 0.125, CFG)
    assert (n4, s4) == (-1, 0) and not m4.any()
    assert LP.movers_np(r[:0], 0, (0.0, 0.0), 0.25, 0.125, CFG)[1:] == (0, 0)


def test_movers_np_skips(pp, LP):
    base = _rows(pp, 1)
    base["state"][0, :6] = (1.0, 2.0, 0.3, 0.5, -1.0, 0.1)
    args = ((-4.0, -8.0), 0.25, 0.125, CFG)
    want = LP.movers_np(base, 1, *args)[0][0]
    for bad in (np.nan, np.inf, -np.inf):
        for field, i in [("state", q) for q in range(6)] + [("size", 0), ("size", 1)]:          # each of the eight inputs
            r = np.concatenate([base, base, base])
            r[field][1, i] = bad
            m, n, skipped = LP.movers_np(r, 3, *args)
            assert (n, skipped) == (2, 1) and np.array_equal(m[0], want) and np.array_equal(m[1], want) and not m[2:].any(), (field, i)
    for field, i, v in (("size", 2, np.nan), ("yaw", None, np.inf)):                            # h and yaw are no inputs
        r = base.copy()
        if i is None:
            r[field][0] = v
        else:
            r[field][0, i] = v
        assert LP.movers_np(r, 1, *args)[1:] == (1, 0)
    # too far: |MX| or |MY| above 2^29 sub-cells = 2^19 cells = 131072 m at 0.25 m; exactly 2^29 is in
    for x, n in ((131072.0 - 4.0, 1), (131072.25 - 4.0, 0), (-131072.0 - 4.0, 1), (-131072.25 - 4.0, 0), (1e300, 0)):
        for axis in (0, 1):
            r = base.copy()
            r["state"][0, axis] = x if axis == 0 else x - 4.0
            m, got, skipped = LP.movers_np(r, 1, *args)
            assert (got, skipped) == (n, 1 - n), (x, axis)
            if n:
                assert abs(int(m[0, axis])) == 2 ** 29
    # too fast: above 16384 sub-cells = 16 cells = 4 m per step of 0.125 s = 32 m/s; exactly 16384 is in
    for v, n in ((32.0, 1), (-32.0, 1), (32.001, 0), (-32.001, 0), (1e308, 0)):
        for axis in (3, 4):
            r = base.copy()
            r["state"][0, axis] = v
            m, got, skipped = LP.movers_np(r, 1, *args)
            assert (got, skipped) == (n, 1 - n), (v, axis)
            if n:
                assert abs(int(m[0, axis - 1])) == 16384
    # a skipped unconfirmed row is not counted: it was never a candidate
    r = base.copy()
    r["confirmed"] = 0
    r["state"][0, 0] = np.nan
    assert LP.movers_np(r, 1, *args)[1:] == (0, 0)
    # a negative size clips at 0; vz and z are inputs only in that they must be finite
    r = base.copy()
    r["size"][0, :2] = (-3.0, -2.0)
    assert LP.movers_np(r, 1, *args)[0][0, 4:].tolist() == [0, 0]
    # what movers_np makes, check_movers accepts
    rng = np.random.default_rng(3)
    r = _rows(pp, 64)
    r["state"][:, :6] = rng.uniform(-40.0, 40.0, (64, 6))
    r["size"][:, :2] = rng.uniform(0.0, 12.0, (64, 2))
    m, n, skipped = LP.movers_np(r, 64, *args)
    assert n + skipped == 64 and n > 32 and len(LP.check_movers(m[:n])) == n


def test_config_refusals(LP):
    c = LP.MoverConfig()
    assert (c.horizon, c.mover_weight, c.confirmed_only) == (32, 64, True) and 0.0 <= c.pad_hard <= c.pad_soft
    assert LP.MoverConfig.from_any(True) == c and LP.MoverConfig.from_any(c) is c and LP.MoverConfig.from_any(c.to_dict()) == c
    for field, lo, hi in (("horizon", 0, 256), ("mover_weight", 0, 65535)):
        for v in (lo, hi):
            assert getattr(LP.MoverConfig(**{field: v}), field) == v
        for v in (lo - 1, hi + 1, 1.0, True, "1", None):
            with pytest.raises(ValueError, match=field):
                LP.MoverConfig(**{field: v})
    for kw in (dict(pad_hard=-0.1), dict(pad_hard=0.5, pad_soft=0.4), dict(pad_hard=np.nan), dict(pad_soft=np.inf), dict(pad_hard="0.1"),
               dict(pad_soft=None), dict(pad_hard=True)):
        with pytest.raises(ValueError, match="pad_"):
            LP.MoverConfig(**kw)
    assert LP.MoverConfig(pad_hard=0, pad_soft=0).pad_soft == 0.0 and LP.MoverConfig(confirmed_only=0).confirmed_only is False
    with pytest.raises(ValueError, match="confirmed_only"):
        LP.MoverConfig(confirmed_only=2)
    with pytest.raises(ValueError, match="horizont"):
        LP.MoverConfig.from_any(dict(horizont=3))
    for bad in (None, False, 3, "on"):
        with pytest.raises(ValueError, match="MoverConfig"):
            LP.MoverConfig.from_any(bad)


def test_mover_and_call_refusals(pp, LP):
    b = M.A
    ok = (1000, 1000, 0, 0, 10, 20)
    for i, v, what in ((0, 2 ** 29 + 1, "position"), (1, -2 ** 29 - 1, "position"), (2, 16385, "movement"), (3, -16385, "movement"),
                       (4, -1, "radii"), (4, 21, "radii"), (5, 32768, "radii")):
        m = [ok, list(ok)]
        m[1][i] = v
        with pytest.raises(ValueError, match="mover 1.*" + what):
            LP.check_movers(m)
        for f in (LP.score_np, ):
            with pytest.raises(ValueError, match="mover 1"):
                f(b.grid, b.pot, b.pose, 1000, 0, b.ncfg, b.cfg, m, True)
        for f in (LP.scores_np, LP.keys_by_sample_np, LP.best_np):
            with pytest.raises(ValueError, match="mover 1"):
                f(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, movers=m, mcfg=True)
    edge = [(2 ** 29, -2 ** 29, 16384, -16384, 0, 0), (0, 0, 0, 0, 32767, 32767)]
    assert LP.check_movers(edge).tolist() == [list(e) for e in edge] and LP.check_movers([]).shape == (0, 6)
    with pytest.raises(ValueError, match="at most PP_LOCAL_MAX_MOVERS"):
        LP.check_movers([ok] * 65)
    for bad in (np.zeros((2, 5), np.int32), np.zeros((2, 6)), np.zeros(6, np.int32)):
        with pytest.raises(ValueError, match="movers must be integers"):
            LP.check_movers(bad)
    with pytest.raises(ValueError, match="movers need mcfg"):
        LP.best_np(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, movers=[ok])
    with pytest.raises(ValueError, match="mcfg without movers"):
        LP.best_np(b.grid, b.pot, b.pose, b.window, b.ncfg, b.cfg, mcfg=True)
    r = _rows(pp, 1)
    for kw, what in ((dict(res=0.0), "res"), (dict(res=-1.0), "res"), (dict(res=np.nan), "res"), (dict(dt=0.0), "dt"), (dict(dt=np.inf), "dt"),
                     (dict(origin=(np.nan, 0.0)), "origin")):
        a = dict(dict(origin=(0.0, 0.0), res=0.25, dt=0.125), **kw)
        with pytest.raises(ValueError, match="movers_np: " + what):
            LP.movers_np(r, 1, a["origin"], a["res"], a["dt"], CFG)
    with pytest.raises(ValueError, match="PP_TRACK_MAX"):
        LP.movers_np(_rows(pp, 65), 65, (0.0, 0.0), 0.25, 0.125, CFG)
    # the stand-alone GPU call refuses on the host, before it looks for a library or a device
    g, pot = np.zeros((4, 4), np.int8), np.zeros((4, 4), np.uint32)
    call = lambda **kw: LP.local_plan(g, pot, (0, 0, 0), (0, 0, 0, 0), {}, dict(nv=1, nw=1, steps=1), **kw)      # noqa: E731
    with pytest.raises(ValueError, match="movers need mover_cfg"):
        call(movers=[ok])
    with pytest.raises(ValueError, match="without movers"):
        call(mover_cfg=True)
    with pytest.raises(ValueError, match="mover 0.*radii"):
        call(movers=[(0, 0, 0, 0, 5, 4)], mover_cfg=True)
    with pytest.raises(ValueError, match=r"\[1, 64, 6\]"):
        call(movers=[ok], n_movers=[1], mover_cfg=True)
    with pytest.raises(ValueError, match="grid 0: n_movers = 65"):
        call(movers=np.zeros((1, 64, 6), np.int32), n_movers=[65], mover_cfg=True)


# ---- the C-ABI's structure ----
NEW = ["pp_set_local_movers", "pp_get_local_movers_config", "pp_local_plan_movers_async", "pp_get_local_movers"]


def test_struct_header_exports_and_sources(pp, LP):
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    csrc = os.path.join(os.path.dirname(pp._lib.__file__), "csrc")
    assert ctypes.sizeof(pp._lib.PPLocalMoverConfig) == 32
    assert [f[0] for f in pp._lib.PPLocalMoverConfig._fields_] == re.findall(r"^\s+(?:double|int32_t) (\w+);", hdr[hdr.index("typedef struct pp_local_mover_config"):hdr.index("} pp_local_mover_config;")], re.M)
    api = open(os.path.join(csrc, "api_local_plan.hip")).read()
    assert "static_assert(sizeof(pp_local_mover_config) == 32" in api and "static_assert(sizeof(LocalFrame) == 32" in api
    for name, v in (("PP_LOCAL_MAX_MOVERS", 64), ("PP_LOCAL_MAX_MOVER_SPEED", 16384), ("PP_LOCAL_MAX_MOVER_RADIUS", 32767), ("PP_LOCAL_MOVER_INFO", 4)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr) and getattr(pp._lib, name) == v, name
    assert LP.MOVER_INFO == ("n_movers", "n_skipped", "n_dynamic", "near") and pp._lib.PP_LOCAL_MAX_MOVERS == pp._lib.PP_TRACK_MAX
    assert "#define PP_ABI_VERSION 4" in hdr and "#define PP_LOCAL_RESULT 8 " in hdr
    later = hdr[hdr.index("later additions within 4"):hdr.index("#define PP_ABI_VERSION")]
    for name in ["pp_local_mover_config", "PP_LOCAL_MAX_MOVERS", "PP_LOCAL_MAX_MOVER_SPEED", "PP_LOCAL_MAX_MOVER_RADIUS", "PP_LOCAL_MOVER_INFO",
                 "pp_local_plan_grids_movers"] + NEW:
        assert re.search(r"\b%s\b" % name, later), name
    exp = pp._lib.EXPORTS
    at = exp.index("pp_local_plan_grids")
    assert exp[at + 1:at + 6] == NEW + ["pp_local_plan_grids_movers"]
    for name in NEW:
        assert re.search(r"\bint %s\(pp_handle" % name, hdr), name
    assert re.search(r"\bint pp_local_plan_grids_movers\(int device", hdr)
    src = pp._lib.SOURCES
    at = src.index("local_plan.hip")
    assert src[at + 1] == "local_movers.hip" and src[-2:] == ["api_track.hip", "track.hip"]
    for name in ("MoverConfig", "movers_np", "check_movers"):
        assert callable(getattr(LP, name)), name
    for name in ("set_local_movers", "local_movers_config", "local_movers"):
        assert callable(getattr(pp.Engine, name)), name
    # opt-in at run time only: no configuration key, no environment switch
    assert "MOVER" not in open(os.path.join(csrc, "pp_switches.h")).read().upper()
    assert "getenv" not in open(os.path.join(csrc, "local_movers.hip")).read()
    doc = LP.__doc__
    for what in ("swept collision between", "tunnel through a small radius", "rectangular mover shapes", "a lead time between", "movers that react to the robot",
                 "footprints other than a point"):
        assert what in re.sub(r"\s+", " ", doc), what


def test_exported_from_the_library_and_null_handle(pp, LP, hip_lib):
    for name in NEW + ["pp_local_plan_grids_movers"]:
        assert hasattr(hip_lib, name), name
    PP_ERR_ARG = 1
    mc = pp._lib.PPLocalMoverConfig(0.25, 0.5, 16, 64, 1, 0)
    on = ctypes.c_int32(7)
    three, four, frame = np.zeros((1, 3), np.int32), np.zeros((1, 4), np.int32), np.ones((1, 4))
    assert hip_lib.pp_set_local_movers(None, 0, ctypes.byref(mc)) == PP_ERR_ARG
    assert hip_lib.pp_get_local_movers_config(None, 0, ctypes.byref(on), None) == PP_ERR_ARG and on.value == 7
    assert hip_lib.pp_local_plan_movers_async(None, 0, three.ctypes.data, four.ctypes.data, frame.ctypes.data, 1) == PP_ERR_ARG
    assert hip_lib.pp_get_local_movers(None, 0, None, None, 1) == PP_ERR_ARG
    # the stand-alone call refuses its arguments before it looks for a device
    c = pp._lib.PPLocalPlanConfig(3, 3, 2, 0, 1, 0, 1, 1)
    n = pp._lib.PPNavfnConfig(99, 10, 1, 0, 50, 8, 1024, 0)
    trig = np.ascontiguousarray(LP.trig_table())
    g, pot = np.zeros((2, 2), np.int8), np.zeros((2, 2), np.uint32)
    table = np.zeros((1, 64, 6), np.int32)
    table[0, :2] = [(5, 5, 1, 1, 2, 3), (5, 5, 1, 1, 2, 3)]

    def call(movers=table, n_movers=2, horizon=4, weight=5, mover=None):
        t = movers if mover is None else movers.copy()
        if mover is not None:
            t[0, 1] = mover
        nm = np.array([n_movers], np.int32)
        P = lambda a: None if a is None else a.ctypes.data      # noqa: E731
        st = hip_lib.pp_local_plan_grids_movers(0, P(g), P(pot), 1, 2, 2, ctypes.byref(n), ctypes.byref(c), P(trig), 4096, P(three), P(four), None,
                                                horizon, weight, P(t), P(nm), None, None, None, None, None)
        return st, (hip_lib.pp_last_error(None) or b"").decode()

    for kw, what in ((dict(movers=None), "movers or n_movers is NULL"), (dict(horizon=-1), "horizon = -1"), (dict(horizon=257), "horizon = 257"),
                     (dict(weight=65536), "mover_weight = 65536"), (dict(n_movers=-1), "grid 0: n_movers = -1"), (dict(n_movers=65), "n_movers = 65"),
                     (dict(mover=(2 ** 29 + 1, 0, 0, 0, 0, 0)), "grid 0, mover 1: position"), (dict(mover=(0, -2 ** 29 - 1, 0, 0, 0, 0)), "mover 1: position"),
                     (dict(mover=(0, 0, 16385, 0, 0, 0)), "grid 0, mover 1: movement"), (dict(mover=(0, 0, 0, -16385, 0, 0)), "mover 1: movement"),
                     (dict(mover=(0, 0, 0, 0, -1, 0)), "grid 0, mover 1: radii"), (dict(mover=(0, 0, 0, 0, 4, 3)), "mover 1: radii"),
                     (dict(mover=(0, 0, 0, 0, 0, 32768)), "mover 1: radii"), (dict(mover=(-2 ** 31, 0, 0, 0, 0, 0)), "mover 1: position")):
        st, msg = call(**kw)
        assert st == PP_ERR_ARG and "pp_local_plan_grids_movers" in msg and what in msg, (kw, msg)
