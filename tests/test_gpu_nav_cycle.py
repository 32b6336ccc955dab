"""The whole navigation cycle on one handle -- live feed, occupancy update, frustum crop, sweep accumulation, the tracked pass
under ego poses with projection on, costmap, both inflations, and behind each inflation the navigation function, the movers
from the tracks and the local planner's command -- over 2 * OFF_RING + 1 cycles, held to the chain of the
package's numpy restatements (tests/nav_cycle_cases.py; tests/test_nav_cycle_host.py shows the chain reaches the edges).
Every comparison is np.array_equal or bytes; the one exclusion is the costmap's undecided cells (a footprint edge within
1e-9 m of a cell centre), at most 0.1 % of a cycle's cells, and an inflated costmap is then held to inflate_np of the run's
own grid; every planner output of a run is held to the restatements on that run's own inflated grids, tracks and origins
as well (K.same_plan).  The passes of the chain come from a second engine with no stage but the projection, fed
synchronously.  The costmap's navigation function queues one round, so its field is never settled at the call and every
fetch of its command goes through the getter's settle and second rollout.

What the single-stage files cannot see is what the stages share -- the two input buffers and their events, the call rings,
the graph key, scratch -- so the cases differ in how much the host waits: after every stage (1), once per cycle (2, 3), never
(4), with the next cycle's feed queued before this cycle's fetch (6), and with the next cycle queued through both
inflations before this cycle's command is fetched (8).

By design, stated here because two cases meet it:
  * pp_frustum_crop_async refuses frames whose sizes only the device knows (PP_ERR_STATE, "their sizes are device values"):
    behind a PointCloud2 ingest the crop cannot run.  The ingested case (3) asserts that refusal and its text in every
    cycle, then ingests the rows the crop keeps (the chain's, which case 1 has held to the GPU crop) as a second feed of the
    cycle; everything but crop_info() is compared.
  * Case 6 meets no refusal: upload_async, crop and sweeps of cycle k + 1 are accepted while cycle k's results are
    unfetched.  occupancy_update_async of cycle k + 1 stands between its feed and its crop, so cycle k's maps are fetched
    through their inflation (queued before that update), and the maps themselves at the last cycle.
  * Case 8: the inflated buffers are reused from cycle to cycle, so once cycle k + 1's inflation is queued, a command of
    cycle k can be fetched only if nothing has to be rolled again.  The navigation function keeps its own costs: fields,
    paths and info stay cycle k's.  A getter that has to queue the rollout again -- the field took a further round (the
    costmap source, always), or keys are asked for the first time -- is refused with PP_ERR_STATE; it never reads cycle
    k + 1's grid under cycle k's field.
  * The stream-independence case (5) runs its 2-of-3 cycle two thirds through, not halfway: nav_cycle_cases.short_at
    says why (the stamp gap sits at the halfway point and would hide a reset that did nothing)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import nav_cycle_cases as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REMADE = "PP_ERR_STATE.*pp_get_local_plan: the inflated grids of the {} source were re-made since its navigation function ran"
REFUSED = "PP_ERR_STATE.*pp_frustum_crop_async: .*ingested from camera messages, their sizes are device values"


@pytest.fixture(scope="module")
def seq(pp):
    return K.sequence(pp)


@pytest.fixture(scope="module")
def engines(pp, hip_lib):
    eng, plain = K.engine(pp), K.plain_engine(pp)
    yield eng, plain
    eng.close()
    plain.close()


@pytest.fixture(scope="module")
def want(pp, seq, engines):
    """The chain, once: its passes are the plain engine's."""
    return K.host_chain(seq, K.plain_detector(pp, engines[1]), pp)


def _run_stepwise(pp, eng, seq):
    """The synchronous calls, everything fetched behind its stage."""
    K.reset_all(eng)
    dts, outs = K.Dt(pp, eng), []
    for c in seq:
        B, out = len(c["frames"]), {}
        eng.upload(c["frames"])                                         # 1.
        eng.occupancy_update_async(c["poses"])                          # 2.
        out.update(K.fetch_occupancy(eng))
        kept, out["cropped"] = eng.crop_to_image(c["planes"], return_points=True)      # 3.
        out["kept"] = eng.crop_info()
        assert np.array_equal(kept, out["kept"])
        counts, out["accumulated"] = eng.accumulate_sweeps(c["poses"], c["stamps"], return_points=True)   # 4.
        out["sweeps_info"] = eng.sweeps_info()
        assert np.array_equal(counts, out["sweeps_info"]["count"])
        eng.set_track_dt(dts(c["stamps"]))                              # 5.
        eng.set_track_pose(c["poses"])
        eng.detect_async()                                              # 6.
        eng.sync()
        out.update(K.fetch_pass(eng, B))
        eng.costmap_async()                                             # 7.
        out.update(K.fetch_costmap(eng))
        eng.inflate_async("costmap")                                    # 8.
        eng.inflate_async("occupancy")                                  # 9.
        out.update(K.fetch_inflated(eng))
        wc, wo = (K.plan_windows(pp, s, c["velocities"]) for s, _ in K.SRC)
        eng.navfn_async(c["goals_cm"], "costmap")                       # 10.
        out.update(K.fetch_navfn(eng, c, K.SRC[:1]))
        eng.local_plan_async(c["poses_cm"], wc, "costmap", dt=K.PLAN_DT)        # 11. behind a settled field: no second rollout here
        out.update(K.fetch_local(eng, *K.SRC[0]))
        eng.navfn_async(c["goals_occ"], "occupancy")                    # 12.
        out.update(K.fetch_navfn(eng, c, K.SRC[1:]))
        eng.local_plan_async(None, wo, "occupancy", dt=K.PLAN_DT)       # 13.
        out.update(K.fetch_local(eng, *K.SRC[1]))
        outs.append(out)
    return outs


@pytest.fixture(scope="module")
def stepwise(pp, seq, engines):
    return _run_stepwise(pp, engines[0], seq)


@pytest.fixture(scope="module")
def queued(pp, seq, engines, stepwise):
    return K.run_queued(pp, engines[0], seq)


def _not_empty(outs):
    """No comparison was between empty results: detections, live confirmed tracks with a velocity, footprints, cells raised."""
    assert sum(int(o["n"].sum()) for o in outs) > 0
    tr, nt, _ = outs[-1]["tracks"]
    assert nt.sum() > 0 and any(tr[b]["confirmed"][:nt[b]].any() and (tr[b]["state"][:nt[b], 3:5] != 0).any() for b in range(len(nt)))
    assert (outs[-1]["cm_info"]["footprints"] > 0).all() and (outs[-1]["cm_grid"] == 90).any()
    assert (outs[-1]["infl_cm"][2]["raised"] > 0).all() and (outs[-1]["infl_occ"][2]["raised"] > 0).all()
    if "occ_logodds" in outs[-1]:
        assert (outs[-1]["occ_logodds"] > 0).any() and (outs[-1]["occ_logodds"] < 0).any()
    # the planner: fields that reach cells, commands on valid samples, movers in the tables
    for s, _ in K.SRC:
        assert any((o[f"nav_info_{s}"]["reached"] > 100).any() for o in outs), s
        assert any(((o[f"plan_info_{s}"]["cmd_state"] == 0) & (o[f"plan_info_{s}"]["n_ok"] >= 8)).any() for o in outs), s
        assert any((o[f"plan_info_{s}"]["n_movers"] > 0).any() for o in outs), s


def _planner_reached(outs):
    """The planner's share of tests/test_nav_cycle_host.py's conditions, on a run of the whole sequence."""
    pairs, states = len(outs) * K.STREAMS, []
    for s, _ in K.SRC:
        info = [o[f"plan_info_{s}"] for o in outs]
        assert 2 * sum(int(((w["cmd_state"] == 0) & (w["n_ok"] >= 8)).sum()) for w in info) >= pairs, s
        states += [int(v) for w in info for v in w["cmd_state"]]
    assert sum(int((o[f"plan_info_{s}"]["n_dynamic"] > 0).sum()) for o in outs for s, _ in K.SRC) > 0
    assert sum(int((o[f"plan_info_{s}"]["near"] > 0).sum()) for o in outs for s, _ in K.SRC) > 0
    assert 4 in states and (1 in states or 2 in states), sorted(set(states))
    # one queued round never settles the costmap's field: the getter finished it (and rolled the samples again)
    assert all((o["nav_info_cm"]["rounds"] > 1).all() for o in outs), [o["nav_info_cm"]["rounds"].tolist() for o in outs]


# ---- 1 ----
def test_step_by_step_every_cycle_equals_the_chain(pp, seq, stepwise, want):
    assert len(stepwise) == len(want) == K.ring_turn(pp)
    for i, (got, w) in enumerate(zip(stepwise, want)):
        K.same_as_chain(got, w, f"stepwise, cycle {i}")
        K.same_inflation(pp, got, f"stepwise, cycle {i}")
        K.same_plan(pp, got, f"stepwise, cycle {i}")
        print(f"cycle {i}: kept {got['kept'].tolist()} rows {got['sweeps_info']['count'].tolist()} detections {got['n'].tolist()} "
              f"tracks {got['tracks'][1].tolist()} undecided {int(w['cm_undecided'].sum())}")
    assert sum(int(o["sweeps_info"]["truncated"].sum()) for o in stepwise) > 0
    _not_empty(stepwise)
    _planner_reached(stepwise)


# ---- 2 ----
def test_all_queued_equals_step_by_step_byte_for_byte(pp, queued, stepwise, want):
    for i, (got, w) in enumerate(zip(queued, want)):
        K.same_as_chain(got, w, f"queued, cycle {i}")
        K.same_inflation(pp, got, f"queued, cycle {i}")
        K.same_plan(pp, got, f"queued, cycle {i}")
        K.same_bytes(got, stepwise[i], f"queued against stepwise, cycle {i}")
    _not_empty(queued)
    _planner_reached(queued)


# ---- 3 ----
def _messages(frames):
    """The PointCloud2 tuples of tests/test_gpu_sweeps.py::test_ingested_frames_sizes_on_the_device_only (x y z intensity)."""
    fields = [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1), ("intensity", 12, 7, 1)]
    return [(f.tobytes(), f.shape[0], 1, 4 * K.F, 4 * K.F * f.shape[0], fields) for f in frames]


def test_ingested_feed_equals_the_queued_run(pp, seq, engines, queued, want):
    from pp_amd import ingest
    eng = engines[0]
    feats, mount = [ingest.FeatureField("intensity")], ingest.Mount(np.eye(3), np.eye(3), 0.0)
    K.reset_all(eng)
    dts, outs, stagings = K.Dt(pp, eng), [], []
    for i, c in enumerate(seq):
        for frames in (c["frames"], want[i]["cropped"]):
            stagings.append(eng.staging_pointcloud2(_messages([np.ascontiguousarray(f) for f in frames]), features=feats, mount=mount))
        eng.ingest_pointcloud2_async(stagings[-2], first=0, decimate=1)                # 1. the frames as they arrive
        assert eng._offsets is None                                                    # nothing on the host knows the sizes
        eng.occupancy_update_async(c["poses"])                                         # 2.
        with pytest.raises(RuntimeError, match=REFUSED):                               # 3. refused by design (module docstring) ...
            eng.crop_to_image_async(c["planes"])
        eng.ingest_pointcloud2_async(stagings[-1], first=0, decimate=1)                # ... so the kept rows arrive as a feed
        K.queue_behind_crop(eng, c, dts(c["stamps"]))                                  # 4. .. 13.
        outs.append(K.fetch_all(eng, c, crop=False))
        assert np.array_equal(eng.ingest_info()["kept"], queued[i]["kept"])
    eng.sync()
    for st in stagings:
        st.close()
    for i, got in enumerate(outs):
        K.same_as_chain(got, want[i], f"ingested, cycle {i}")
        K.same_bytes(got, queued[i], f"ingested against queued, cycle {i}")
    assert set(queued[0]) - set(outs[0]) == {"kept"}
    _not_empty(outs)


# ---- 4 ----
def test_every_ring_full_at_once(pp, seq, engines, queued, want):
    eng = engines[0]
    K.reset_all(eng)
    dts = K.Dt(pp, eng)
    stagings = [eng.staging(c["frames"]) for c in seq]
    for c, st in zip(seq, stagings):                                    # nothing fetched, no sync(): every ring turns twice
        eng.upload_async(st)
        K.queue_stages(eng, c, dts(c["stamps"]))
    got = K.fetch_all(eng, seq[-1])
    eng.sync()
    for st in stagings:
        st.close()
    K.same_as_chain(got, want[-1], "back to back, last cycle")
    K.same_inflation(pp, got, "back to back, last cycle")
    K.same_plan(pp, got, "back to back, last cycle")
    K.same_bytes(got, queued[-1], "back to back against queued, last cycle")
    # the stateful outputs vouch for every earlier cycle: tracks that lived through them, sweeps of the two before
    assert got["tracks"][0]["hits"].max() >= 4 and (got["sweeps_info"]["used"] == 2).all()
    _not_empty([got])


# ---- 5 ----
def test_streams_are_independent(pp, seq, engines, queued, want):
    eng, plain = engines
    detect = K.plain_detector(pp, plain)
    at = K.short_at(len(seq))
    assert len(seq) - at >= 3
    chain, fresh = K.HostChain(pp, detect), K.HostChain(pp, detect)
    K.reset_all(eng)
    dts, stagings, outs = K.Dt(pp, eng), [], []

    def cycle(c):
        stagings.append(eng.staging(c["frames"]))
        eng.upload_async(stagings[-1])
        K.queue_stages(eng, c, dts(c["stamps"]))
        return K.fetch_all(eng, c)

    for i in range(at):
        K.same_bytes(cycle(seq[i]), queued[i], f"before the short call, cycle {i}")
        chain.step(seq[i])
    two = K.short(seq[at], 2)
    got = cycle(two)
    K.same_as_chain(got, chain.step(two), "the short call")
    assert got["n"].shape == (2,) and got["occ_grid"].shape[0] == 2 and got["infl_cm"][0].shape[0] == 2
    assert got["field_cm"].shape[0] == 2 and got["keys_occ"].shape[0] == 2 and len(got["traj_occ"]) == 2
    K.same_plan(pp, got, "the short call")
    K.reset_stream(eng, 1)
    chain.reset(1)
    dts.reset(1)
    for i in range(at + 1, len(seq)):
        got, w = cycle(seq[i]), chain.step(seq[i])
        outs.append(got)
        # stream 2 goes on from where it was before the short call, stream 1 from nothing, stream 0 from the short call
        K.same_as_chain(got, w, f"after the short call, cycle {i}")
        K.same_inflation(pp, got, f"after the short call, cycle {i}")
        K.same_plan(pp, got, f"after the short call, cycle {i}")
        K.same_as_chain(got, fresh.step(seq[i]), f"stream 1 against a fresh chain, cycle {i}", streams=[1])
        K.same_as_chain(got, want[i], f"stream 0 against the full run, cycle {i}", streams=[0])
        assert got["sweeps_info"]["used"][1] == i - at - 1
    # both the short call and the reset show: a run that ignored either would not be this one
    first = outs[0]
    assert queued[at + 1]["sweeps_info"]["used"][1] == 2 and first["sweeps_info"]["used"][2] < queued[at + 1]["sweeps_info"]["used"][2]
    assert not np.array_equal(first["occ_logodds"][1], queued[at + 1]["occ_logodds"][1])
    eng.sync()
    for st in stagings:
        st.close()
    _not_empty(outs)


# ---- 6 ----
def test_next_feed_queued_before_this_cycles_fetch(pp, seq, engines, queued, want):
    eng = engines[0]
    K.reset_all(eng)
    dts = K.Dt(pp, eng)
    stagings = [eng.staging(c["frames"]) for c in seq]

    def feed(i):
        eng.upload_async(stagings[i])                                   # 1. .. 4. of cycle i
        eng.occupancy_update_async(seq[i]["poses"])
        eng.crop_to_image_async(seq[i]["planes"])
        eng.accumulate_sweeps_async(seq[i]["poses"], seq[i]["stamps"])

    feed(0)
    outs, nxt = [], {"kept": eng.crop_info(), "sweeps_info": eng.sweeps_info()}
    for i, c in enumerate(seq):
        last = i + 1 == len(seq)
        got = nxt
        eng.set_track_dt(dts(c["stamps"]))                              # 5. .. 9. of cycle i
        eng.set_track_pose(c["poses"])
        eng.detect_async()
        eng.costmap_async()
        eng.inflate_async("costmap")
        eng.inflate_async("occupancy")
        K.queue_plan(eng, c)                                            # 10. .. 13. of cycle i: queued before the next feed ...
        if not last:
            feed(i + 1)                                                 # accepted: nothing of it is refused
        else:
            got.update(K.fetch_occupancy(eng))
        got.update(K.fetch_pass(eng, K.STREAMS))
        got.update(K.fetch_costmap(eng))
        got.update(K.fetch_inflated(eng))
        got.update(K.fetch_plan(eng, c))                                # ... and fetched after it, in cycle i's frame
        if not last:
            nxt = {"kept": eng.crop_info(), "sweeps_info": eng.sweeps_info()}          # (of cycle i + 1 by now)
        outs.append(got)
    eng.sync()
    for st in stagings:
        st.close()
    for i, got in enumerate(outs):
        K.same_as_chain(got, want[i], f"fed ahead, cycle {i}")
        K.same_bytes(got, queued[i], f"fed ahead against queued, cycle {i}")
        assert ("occ_grid" in got) == (i + 1 == len(seq)) and "infl_occ" in got
        # the window has moved on under most of these fetches: the paths in metres are still those of cycle i's window
        assert np.array_equal(got["plan_origin_occ"], want[i]["occ_origin"]), i
        for b in range(K.STREAMS):
            assert got["paths_m_occ"][b].dtype == np.float64 and np.array_equal(got["paths_m_occ"][b], want[i]["paths_m_occ"][b]), (i, b)
    assert any(not np.array_equal(want[i]["occ_origin"], want[i + 1]["occ_origin"]) for i in range(len(seq) - 1))
    _not_empty(outs)


# ---- 7 ----
def test_plain_launches_give_the_same_digests(pp, queued):
    """The queued run again in one fresh child process under PP_NO_GRAPH=1 (the switches are read once per process)."""
    env = dict(os.environ, PP_NO_GRAPH="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "nav_cycle_cases.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("NAV_CYCLE_DIGESTS ")]
    assert len(line) == 1, r.stdout[-2000:]
    child = json.loads(line[0].split(" ", 1)[1])
    assert child["no_graph"] == "1"
    assert child["digests"] == [K.digest(o) for o in queued]
    assert len(set(child["digests"])) == len(queued) and child["detections"] == sum(int(o["n"].sum()) for o in queued) > 0


# ---- 8 ----
def test_the_command_one_cycle_behind(pp, seq, engines, queued, want):
    """Cycle i queued whole, plan included and unfetched; cycle i + 1 queued through both inflations; then cycle i's planner
    results are asked for (module docstring)."""
    eng = engines[0]
    K.reset_all(eng)
    dts = K.Dt(pp, eng)
    stagings = [eng.staging(c["frames"]) for c in seq]
    queued_occ = 5                                                      # api_navfn.hip default_rounds(37, 29): 2 + 2 / 2 + 2
    assert K.NAV_OCC.get("queued_rounds", 0) == 0 and K.NAV_CM["queued_rounds"] == 1
    nav = [k for k in queued[0] if k.split("_")[0] in ("field", "paths", "nav")]
    local = lambda s: [f"plan_info_{s}", f"traj_{s}", f"movers_{s}"]
    behind = refused_occ = 0

    def stages(i):                                                      # 1. .. 9. of cycle i
        eng.upload_async(stagings[i])
        eng.occupancy_update_async(seq[i]["poses"])
        eng.crop_to_image_async(seq[i]["planes"])
        eng.accumulate_sweeps_async(seq[i]["poses"], seq[i]["stamps"])
        eng.set_track_dt(dts(seq[i]["stamps"]))
        eng.set_track_pose(seq[i]["poses"])
        eng.detect_async()
        eng.costmap_async()
        eng.inflate_async("costmap")
        eng.inflate_async("occupancy")

    stages(0)
    for i in range(len(seq) - 1):
        c, what = seq[i], f"one behind, cycle {i}"
        K.queue_plan(eng, c)                                            # 10. .. 13. of cycle i, nothing of it fetched
        stages(i + 1)                                                   # both inflated buffers now hold cycle i + 1's grids
        # the navigation function copied its costs at the call: the fields, paths and info are cycle i's, both sources
        got = K.fetch_navfn(eng, c)
        got["n"] = queued[i]["n"]
        K.same_bytes({k: got[k] for k in nav + ["n"]}, queued[i], what)
        assert set(nav) <= set(got) and np.array_equal(got["plan_origin_occ"], want[i]["occ_origin"]), what
        assert (got["nav_info_cm"]["rounds"] > 1).all(), what
        # the costmap's command needs the second rollout, over a grid that is no longer there: refused
        for fetch in (eng.local_commands, eng.local_plan_info, eng.local_trajectories, eng.local_keys):
            with pytest.raises(RuntimeError, match=REMADE.format("costmap")):
                fetch("costmap")
        # the occupancy field settled within the rounds its call queued, unless a grid ran all of them and more
        if (got["nav_info_occ"]["rounds"] <= queued_occ).all():
            occ = K.fetch_local(eng, "occ", "occupancy", keys=False)
            occ["n"] = queued[i]["n"]
            K.same_bytes({k: occ[k] for k in local("occ") + ["n"]}, queued[i], what)
            assert set(local("occ")) <= set(occ)
            with pytest.raises(RuntimeError, match=REMADE.format("occupancy")):      # keys were not stored: a rollout again
                eng.local_keys("occupancy")
            assert eng.local_plan_info("occupancy")["cmd_state"].tobytes() == queued[i]["plan_info_occ"]["cmd_state"].tobytes()
            behind += 1
        else:
            with pytest.raises(RuntimeError, match=REMADE.format("occupancy")):
                eng.local_commands("occupancy")
            refused_occ += 1
        # the handle goes on: cycle i + 1's plan, queued and fetched in order
        K.queue_plan(eng, seq[i + 1])
        nxt = K.fetch_plan(eng, seq[i + 1])
        nxt["n"] = queued[i + 1]["n"]
        K.same_bytes(nxt, queued[i + 1], f"in order again, cycle {i + 1}")
    got = K.fetch_all(eng, seq[-1])
    eng.sync()
    for st in stagings:
        st.close()
    K.same_bytes(got, queued[-1], "one behind, the last cycle whole")
    print(f"one behind: occupancy commands fetched in {behind} cycles, refused in {refused_occ}")
    assert behind >= (len(seq) - 1) // 2
