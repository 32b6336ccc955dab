"""The navigation cycle's host chain alone (tests/nav_cycle_cases.py), with the CPU oracle for the passes: the scenario
reaches every edge the GPU test (tests/test_gpu_nav_cycle.py) is to compare at.  Each assertion is a condition on the inputs;
one that fails asks for another scenario, not for another assertion."""
import inspect
import os
import re

import numpy as np
import pytest

import nav_cycle_cases as K


@pytest.fixture(scope="module")
def run(pp):
    seq = K.sequence(pp)
    return seq, K.host_chain(seq, K.oracle_detector(pp), pp)


def test_the_sequence_is_one_more_than_two_turns_of_a_call_ring(pp, run):
    seq, outs = run
    assert len(seq) == len(outs) == K.ring_turn(pp) >= 9
    sizes = {len(f) for c in seq for f in c["frames"]}
    assert sizes == {0, 1, 63, 64, 65, 257}
    for b in range(K.STREAMS):
        assert {len(c["frames"][b]) for c in seq} == sizes, b
    for c in seq:
        assert all(f.dtype == np.float32 and f.shape[1] == K.F for f in c["frames"])
    gaps = np.diff([c["stamps"][0] for c in seq])
    assert (gaps > 0).all() and (gaps > K.SWEEPS["max_age"]).sum() == 1


def test_crop_and_sweeps_reach_their_edges(run):
    seq, outs = run
    for i, (c, o) in enumerate(zip(seq, outs)):
        for b, f in enumerate(c["frames"]):
            if len(f) >= 63:
                assert 1 <= o["kept"][b] < len(f), (i, b, o["kept"][b])
    used = [o["sweeps_info"]["used"] for o in outs]
    after = K.GAP_AFTER + 1
    for i in range(2, len(outs)):
        if i not in (after, after + 1):
            assert (used[i] == 2).any(), i
    assert (used[after] < 2).any() and (used[after - 1] == 2).any()
    assert sum(int(o["sweeps_info"]["truncated"].sum()) for o in outs) > 0
    assert sum(int(o["sweeps_info"]["push_truncated"].sum()) for o in outs) > 0
    assert all((o["sweeps_info"]["count"] <= K.NMAX).all() for o in outs)


def test_tracks_are_confirmed_and_move(run):
    _, outs = run
    assert sum(int(o["n"].sum()) for o in outs) > 0
    tr, nt, _ = outs[3]["tracks"]
    assert any(tr[b]["confirmed"][:nt[b]].any() for b in range(K.STREAMS))
    assert any((tr[b]["state"][:nt[b], 3:5] != 0).any() for b in range(K.STREAMS))
    ft, fn = outs[3]["tracks_fixed"]
    assert (fn >= 0).all()                                                              # every stream steps under a pose


def test_costmaps_hold_objects_and_predictions_and_few_undecided_cells(pp, run):
    _, outs = run
    cm = pp.costmap.CostmapConfig.from_any(K.COSTMAP)
    points_only = pp.costmap.CostmapConfig.from_any(K.GRID)
    for i, o in enumerate(outs):
        und = o["cm_undecided"]
        assert und.shape == o["cm_grid"].shape == (K.STREAMS, K.GRID["height"], K.GRID["width"])
        for b in range(K.STREAMS):
            assert int(und[b].sum()) <= K.UNDECIDED_CAP * und[b].size, (i, b, int(und[b].sum()))
        if i < 3:
            continue
        for b in range(K.STREAMS):
            g = o["cm_grid"][b]
            bare, _ = pp.costmap.costmap_np(o["accumulated"][b], points_only)
            assert ((g == cm.object_cost) & (bare != cm.object_cost)).any(), (i, b)    # cells only a footprint raised
            assert np.isin(g, cm.predict_cost[:cm.horizon_steps]).any(), (i, b)
            assert o["cm_info"]["footprints"][b] >= 3, (i, b)


def test_occupancy_maps_fill_and_their_windows_move(run):
    _, outs = run
    W, H = K.OCC["width"], K.OCC["height"]
    for i, o in enumerate(outs):
        for b in range(K.STREAMS):
            assert (o["occ_logodds"][b] > 0).any() and (o["occ_logodds"][b] < 0).any(), (i, b)      # hit cells, free cells
            assert (o["occ_grid"][b] == -1).any() and (o["occ_grid"][b] >= 0).any(), (i, b)
    assert (outs[0]["occ_info"]["cleared"] == W * H).all()
    moved = sum(int(((o["occ_info"]["cleared"] > 0) & (o["occ_info"]["cleared"] < W * H)).sum()) for o in outs[1:])
    assert moved >= K.STREAMS                                                           # every stream's origin moves
    assert len({tuple(o["occ_origin"][0]) for o in outs}) > 1
    assert sum(int(o["occ_info"]["hits"].sum()) for o in outs) > 0


def test_both_inflations_raise_cells(run):
    _, outs = run
    for i, o in enumerate(outs):
        for key in ("infl_cm", "infl_occ"):
            grid, d2, info = o[key]
            assert (info["raised"] > 0).all() and (info["lethal"] > 0).all(), (i, key, info)
            assert grid.dtype == np.int8 and d2.dtype == np.uint16


def test_the_planner_reaches_what_the_gpu_comparison_is_meant_to_see(pp, run):
    """Per source: commands on enough valid samples; movers that end samples and movers that are passed closely; a field
    without a goal, an arrival or a stop; and nothing that stands still from one cycle to the next, or a stale grid or
    field would pass unseen."""
    _, outs = run
    pairs = len(outs) * K.STREAMS
    states = []
    for s, _ in K.SRC:
        info = [o[f"plan_info_{s}"] for o in outs]
        good = sum(int(((w["cmd_state"] == 0) & (w["n_ok"] >= 8)).sum()) for w in info)
        assert 2 * good >= pairs, (s, good, pairs)
        states += [int(v) for w in info for v in w["cmd_state"]]
        for w, o in zip(info, outs):
            total = w["n_ok"] + w["n_outside"] + w["n_collision"] + w["n_unreached"] + w["n_dynamic"]
            rolled = w["cmd_state"] <= 1
            assert (total[rolled] == 65).all() and (total[~rolled] == 0).all(), (s, total)
            assert np.array_equal(w["cmd_state"] == 4, o[f"nav_info_{s}"]["goal_state"] != 0), s
    dyn = sum(int((o[f"plan_info_{s}"]["n_dynamic"] > 0).sum()) for o in outs for s, _ in K.SRC)
    near = sum(int((o[f"plan_info_{s}"]["near"] > 0).sum()) for o in outs for s, _ in K.SRC)
    assert dyn > 0 and near > 0, (dyn, near)
    assert 4 in states and (1 in states or 2 in states), sorted(set(states))
    assert pp.local_planner.MoverConfig(**K.MOV_CM).confirmed_only != pp.local_planner.MoverConfig(**K.MOV_OCC).confirmed_only
    still = []
    for s, infl in (("cm", "infl_cm"), ("occ", "infl_occ")):
        for i, (a, b) in enumerate(zip(outs, outs[1:])):
            for k in range(K.STREAMS):
                same = (np.array_equal(a[infl][0][k], b[infl][0][k]), np.array_equal(a[f"field_{s}"][k], b[f"field_{s}"][k]),
                        a[f"keys_{s}"][k].min() == b[f"keys_{s}"][k].min())
                still += [(s, what, i, i + 1, k) for what, v in zip(("inflated grid", "field", "best key"), same) if v]
    assert not still, still


def test_the_costmap_field_is_never_settled_by_one_round(pp, run):
    """NAV_CM queues one round.  A round relaxes each 32 x 32 tile against the halo the round before left, so a potential
    crosses one tile edge per round at the most: with a goal in the grid and a reached cell in another tile than the
    goal's, one round cannot give the exact field, and every fetch goes through the getter's settle and second rollout."""
    _, outs = run
    H, W = K.GRID["height"], K.GRID["width"]
    assert K.NAV_CM["queued_rounds"] == 1 and W > K.NAV_TILE and H > K.NAV_TILE
    for i, o in enumerate(outs):
        goals = pp.navfn.goal_cells(o["plan_in"]["goals_cm"], K.cm_origins(K.STREAMS), K.GRID["resolution"], (H, W))
        assert (o["nav_info_cm"]["goal_state"] == 0).all(), (i, o["nav_info_cm"]["goal_state"])
        for b in range(K.STREAMS):
            ys, xs = np.nonzero(o["field_cm"][b] != pp.navfn.UNREACHED)
            other = (xs // K.NAV_TILE != goals[b, 0] // K.NAV_TILE) | (ys // K.NAV_TILE != goals[b, 1] // K.NAV_TILE)
            assert other.any(), (i, b)


def test_a_reset_stream_continues_as_a_fresh_chain_does(pp, run):
    """What the GPU test's stream-independence case relies on: no stream's outputs depend on another's, and the short call
    and the reset both show in what follows (a run that ignored either would not pass by accident)."""
    seq, outs = run
    detect = K.oracle_detector(pp)
    at = K.short_at(len(seq))
    chain = K.HostChain(pp, detect)
    for c in seq[:at]:
        chain.step(c)
    chain.step(K.short(seq[at], 2))
    chain.reset(1)
    fresh = K.HostChain(pp, detect)
    assert len(seq) - at >= 3
    for i in range(at + 1, len(seq)):
        a, f = chain.step(seq[i]), fresh.step(seq[i])
        K.same_bytes({k: _stream(v, 1) for k, v in a.items() if k in _PER_STREAM},
                     {k: _stream(v, 1) for k, v in f.items() if k in _PER_STREAM}, ("stream 1", i))
        # stream 0 saw every cycle, the short one included: it is where the full run is
        K.same_bytes({k: _stream(v, 0) for k, v in a.items() if k in _PER_STREAM},
                     {k: _stream(v, 0) for k, v in outs[i].items() if k in _PER_STREAM}, ("stream 0", i))
        assert a["n"][1] > 0 and f["sweeps_info"]["used"][1] == i - at - 1
        if i == at + 1:
            assert outs[i]["sweeps_info"]["used"][1] == 2                              # the reset shows: unreset, two sweeps
            assert a["sweeps_info"]["used"][2] < outs[i]["sweeps_info"]["used"][2]     # the skipped cycle shows on stream 2
            assert not np.array_equal(a["occ_logodds"][1], outs[i]["occ_logodds"][1])


def test_the_documented_call_order_is_the_one_the_gpu_test_runs():
    """INTEGRATION.md's "One navigation cycle" listing, nav_cycle_cases.CYCLE_CALLS and the calls run_queued makes."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "INTEGRATION.md")) as f:
        doc = f.read()
    listing = doc[doc.index("# One navigation cycle"):]
    n = len(K.CYCLE_CALLS) - 1                      # (step 5 is two calls on one line)
    steps = [(int(m.group(1)), m.group(2)) for m in re.finditer(r"^#\s+(\d+)\. (engine\..*?)(?:\s{2,}#.*)?$", listing, re.M)][:n]
    assert [k for k, _ in steps] == list(range(1, n + 1)) and n == 13
    documented = K.calls_in(" \n".join(line.replace("; engine.", "\nengine.") for _, line in steps), "engine")
    assert tuple(documented) == K.CYCLE_CALLS
    src = "".join(inspect.getsource(f) for f in (K.run_queued, K.queue_stages, K.queue_behind_crop, K.queue_plan))
    made = [c for c in K.calls_in(src, "eng") if c.split("(")[0] in {x.split("(")[0] for x in K.CYCLE_CALLS}]
    assert tuple(made) == K.CYCLE_CALLS


_PER_STREAM = ("n", "kept", "occ_grid", "occ_logodds", "occ_origin", "cm_grid", "cm_counts")


def _stream(v, b):
    return np.asarray(v)[b:b + 1]
