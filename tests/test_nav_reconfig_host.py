"""What makes tests/test_gpu_nav_reconfig.py unable to pass vacuously, on the CPU: the scripts of tests/nav_reconfig_cases.py
run on the model alone.  Every row of part B gives other bytes in the stale order (its set_* in front of the source run: the
configuration in force) for every stream; the strides of part A's shrunk runs read other bytes at the kept buffers' caps
for streams 1 and 2; every walk of part C reaches what it is to reach; and the model's own results on an unreconfigured
chain are nav_cycle_cases.plan_np's on the same grids."""
import numpy as np
import pytest

import nav_cycle_cases as K
import nav_reconfig_cases as R

B = R.STREAMS


def _stream(v, b):
    """Stream b's part of an expected value."""
    if isinstance(v, dict):
        return {k: _stream(x, b) for k, x in v.items()}
    if isinstance(v, tuple):
        return tuple(_stream(x, b) for x in v)
    return v[b]


def _differs_at(a, c, b):
    """Two answers of one getter differ for stream b: another kind of answer, or other bytes."""
    if a[0] == "refused" or c[0] == "refused":
        return a[0] != c[0]
    return R.differs(_stream(a[1], b), _stream(c[1], b))


def _discriminated(right, stale, what, streams=range(B)):
    for b in streams:
        where = [g for g in right if _differs_at(right[g], stale[g], b)]
        assert where, (what, "stream", b, "the stale answer is the right one in every getter")


def test_no_point_lies_on_a_cell_border(pp):
    for seed in R.FRAME_SEEDS:
        for cfg in (R.CM_A, R.CM_B, R.CM_C, R.CM_A_MOVED, R.CM_A_COARSE):
            assert R.undecided_points(pp, R.frames(seed), cfg) == 0, (seed, cfg)


@pytest.mark.parametrize("name", R.ROW_NAMES)
def test_a_row_of_part_b_discriminates(pp, name):
    right = R.part_b_row(R.Pair(pp), name)
    stale = R.part_b_row(R.Pair(pp), name, stale=True)
    _discriminated(right, stale, name)
    _, k, _, place, _ = R.ROWS[R.ROW_NAMES.index(name)]
    if not name.startswith("costmap-coarse-behind-source"):
        assert all(v[0] == "ok" for v in right.values()), (name, {g: v[0] for g, v in right.items()})
    else:                                                       # the grids' resolution is the run's: the new table is refused
        assert all(v[0] == "refused" for v in right.values())


def test_part_b_refusal_rows_hold_on_the_model(pp):
    R.part_b_forgotten(R.Pair(pp), R.OCC_COARSE, R.infl_cfg(4, 0.2))
    R.part_b_forgotten(R.Pair(pp), R.OCC_B, None)
    for k in (0, 1):
        before, after = R.part_b_source_off(R.Pair(pp), k)
        _discriminated(before, after, ("another goal behind the source switched off", k))


@pytest.mark.parametrize("k", (0, 1))
def test_part_a_shapes_discriminate(pp, k):
    out = R.part_a_shapes(R.Pair(pp), k)
    chains = [out[0]] + out[2::2]
    for i, old in enumerate(out[1::2]):                         # behind the source's new run: the old shape's, not the new
        assert all(v[0] == "ok" for v in old.values())
        assert not any(R.differs(old[g], chains[i][g]) for g in R.GETTERS)
        for b in range(B):
            assert any(_differs_at(old[g], chains[i + 1][g], b) for g in R.GETTERS), (k, i, b)
    assert all(v[0] == "ok" for c in chains for v in c.values())


def _at_cap(prev, cur, b):
    """What stream b reads where a getter takes the kept buffer's stride (the previous, larger run's) for a buffer the
    current run wrote at its own: rows [B, n_cur] laid over rows [B, n_prev], read back at n_prev."""
    n_prev, n_cur = prev.shape[1], cur.shape[1]
    flat = prev.reshape(-1).copy()
    flat[:B * n_cur] = cur.reshape(-1)
    return flat[b * n_prev:b * n_prev + n_cur]


@pytest.mark.parametrize("k", (0, 1))
def test_part_a_strides_discriminate(pp, k):
    out = R.part_a_strides(R.Pair(pp), k)
    assert all(v[0] == "ok" for o in out for v in o.values())
    grown, shrunk = out[1], out[2]
    keys = (grown["local_keys"][1], shrunk["local_keys"][1])
    assert keys[0].shape == (B, 260) and keys[1].shape == (B, 21)
    pad = lambda paths, cap: np.stack([np.concatenate([p.reshape(-1), np.zeros(2 * cap - p.size, np.int32)]) for p in paths])
    paths = (pad(grown["navfn_paths"][1][0], 256), pad(shrunk["navfn_paths"][1][0], 32))
    for b in (1, 2):
        assert not np.array_equal(_at_cap(*keys, b), keys[1][b]), ("keys", k, b)
        assert not np.array_equal(_at_cap(*paths, b), paths[1][b]), ("paths", k, b)
    for a, c in ((out[0], out[1]), (out[1], out[2])):
        _discriminated(a, c, ("consecutive configurations", k))


def test_part_a_movers_discriminate(pp):
    out = R.part_a_movers(R.Pair(pp))
    getters = R.GETTERS + ("local_movers",)
    assert all(o[g][0] == "ok" for o in out[:4] for g in getters)
    info = out[0]["local_info"][1]
    assert (info["n_movers"] > 0).all() and (info["n_dynamic"] + info["near"] > 0).all(), info
    _discriminated({g: out[0][g] for g in R.LOCAL_GETTERS}, {g: out[1][g] for g in R.LOCAL_GETTERS}, "horizon 4 -> 0")
    assert not any(R.differs(out[2][g], out[0][g]) for g in getters)
    assert not any(R.differs(out[3][g], out[0][g]) for g in getters)        # the movers off behind the run: it keeps them
    _discriminated({g: out[3][g] for g in R.LOCAL_GETTERS}, {g: out[4][g] for g in R.LOCAL_GETTERS}, "a run with movers, one without")


@pytest.mark.parametrize("seed", R.WALK_SEEDS)
def test_a_walk_reaches_what_it_is_to_reach(pp, seed):
    assert len(R.WALK_SEEDS) == 6 and R.WALK_OPS == 40
    pair = R.Pair(pp)
    log = R.run_walk(pair, seed)
    ops = R.walk_ops(seed)
    assert len(log) == len(ops) == R.WALK_OPS
    ok = lambda names: sum(1 for name, want, _ in log if name in names and want == "ok")
    assert ok(R.LOCAL_GETTERS) >= 5, ok(R.LOCAL_GETTERS)
    assert ok(("navfn_fields",)) >= 3, ok(("navfn_fields",))
    assert sum(1 for _, want, _ in log if want == "refused") >= 3
    kinds = {"get" if name in R.GETTERS else name for name, _, _ in log}
    assert kinds == {"get" if name in R.GETTERS else name for name in R.WALK_KINDS}, sorted(kinds)


def test_the_model_is_plan_np_on_an_unreconfigured_chain(pp):
    rows = (np.zeros((B, 64), pp.tracking.TRACK_DTYPE), np.zeros(B, np.int32))
    for k, s in ((0, "cm"), (1, "occ")):
        ncfg, lcfg, _, res = K.plan_configs(pp, s)
        pair = R.Pair(pp)
        R.setup(pair, k, nav=(K.NAV_CM, K.NAV_OCC)[k], loc=(K.LOC_CM, K.LOC_OCC)[k])
        R.source_run(pair, k)
        got = pair.chain(k, R.GOALS[k], R.POSES[k])
        assert all(v[0] == "ok" for v in got.values())
        infl = pair.model.infl_run[k]
        P = R.poses(0, pp)
        asked = dict(goals_cm=R.GOALS_CM, poses_cm=R.POSES_CM, goals_occ=P[:, :2, 3] + R.GOALS_OCC, poses=P, velocities=R.VEL)
        assert np.array_equal(K.plan_windows(pp, s, R.VEL), pair.model.loc_run[k]["windows"])
        want = K.plan_np(pp, s, infl["grids"], asked, infl["org"], *rows)
        R.same(got["navfn_fields"][1], want[f"field_{s}"], "field")
        R.same(got["navfn_paths"][1][0], want[f"paths_{s}"], "paths")
        R.same(got["navfn_paths_m"][1], want[f"paths_m_{s}"], "paths in metres")
        R.same(got["navfn_info"][1], want[f"nav_info_{s}"], "navfn info")
        R.same(got["local_info"][1], {key: want[f"plan_info_{s}"][key] for key in pp.local_planner.RESULT + ("score",)}, "plan info")
        R.same(got["local_traj"][1], want[f"traj_{s}"], "trajectories")
        R.same(got["local_keys"][1], want[f"keys_{s}"], "keys")
        assert (got["navfn_info"][1]["reached"] > 100).all() and (got["local_info"][1]["n_ok"] > 0).all()
