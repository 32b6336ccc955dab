"""The ground stage on the GPU (csrc/ground.hip: k_ground_hyp, k_ground_score, k_ground_pick, k_ground_moments,
k_ground_refit, k_ground_class; the readers' side of it in k_occ_endpoints, k_scan_cells, k_costmap_points) against
ground.py's restatement.  Everything is compared with NO tolerance: the rule is float64 + - * / and comparisons and the
library is built without contraction, so the plane's bits, every count, the winner, the info words, the sums and both bit
planes are the restatement's, and the downstream maps are the host restatements' fed those bits."""
import numpy as np
import pytest

import ground_cases as gc
import object_mask_cases as oc

pytestmark = pytest.mark.gpu

S = oc.CYCLE_STREAMS
NMAX = 512
ROWS = (257, 300, 65)            # unequal, and no frame but the first starts on a 64-row boundary of the buffer
ROWS_EMPTY = (257, 0, 65)


def _same(pp, got, frames, cfg, triples, what):
    """The stand-alone call's (or a handle's) results against ground_np, frame by frame."""
    g = pp.ground
    wpf = got["ground_words"].shape[1]
    for b, f in enumerate(frames):
        want = g.ground_np(f, cfg, triples[b])
        assert got["planes"][b].tobytes() == want["plane"].tobytes(), (what, b, got["planes"][b], want["plane"])
        assert got["info"][b].tolist() == want["info"].tolist(), (what, b)
        assert np.array_equal(got["ground_words"][b], g.pack_words(want["ground"], wpf)), (what, b)      # zero past the frame's rows
        assert np.array_equal(got["obstacle_words"][b], g.pack_words(want["obstacle"], wpf)), (what, b)
        assert got["sums"][b].tolist() == want["sums"].tolist(), (what, b)
        assert got["counts"][b].tolist() == want["counts"].tolist(), (what, b)


def _size_frames(F, seed):
    frames = [gc.floor_scene(seed + i, n, F)[0] for i, n in enumerate(gc.ROWS)]
    frames.append(np.full((70, F), np.nan, np.float32))                    # NaN rows only
    high = gc.floor_scene(seed + 50, 130, F)[0]
    high[:, 2] += 5.0                                                       # no candidate: every hypothesis invalid
    frames.append(high)
    return frames


@pytest.mark.parametrize("K", gc.HYPS)
def test_standalone_sizes(pp, hip_lib, K):
    """Every row count of ground_cases.ROWS (1025 is one past a score tile), a frame of NaN rows and a frame without a
    candidate, as the frames of one call, for every K of {1, 63, 64, 65, PP_GROUND_MAX_HYP}; F = 3 and 4; refine 0 and 1."""
    assert gc.HYPS[-1] == pp.ground.MAX_HYP
    g = pp.ground
    F = 3 + (gc.HYPS.index(K) % 2)
    frames = _size_frames(F, 10 * K)
    t = g.draw_triples(3, K, len(frames), K)
    seen = set()
    for refine in (1, 0):
        cfg = dict(gc.RECOVERY_CFG, hypotheses=K, min_inliers=2, refine=refine)
        got = g.ground(frames, cfg, t)
        _same(pp, got, frames, cfg, t, f"K {K} refine {refine}")
        assert got["info"][-2].tolist()[:5] == [g.FALLBACK, -1, 0, 0, 0] and got["info"][-2][9] == 70
        assert got["info"][-1].tolist()[:5] == [g.FALLBACK, -1, 0, 0, 0] and got["info"][-1][7] == 130       # all OVERHEAD of the fallback
        seen |= set(got["info"][:, 0].tolist())
        if refine and K >= 63:
            assert got["info"][:, 10].sum() >= 4 and np.abs(got["sums"]).sum() > 0
        if not refine:
            assert not got["sums"].any() and not got["info"][:, 10].any()
        again = g.ground(frames, cfg, t)
        assert all(again[k].tobytes() == got[k].tobytes() for k in ("planes", "info", "ground_words", "obstacle_words", "sums", "counts"))
    if K >= 63:
        assert seen == {g.OK, g.FALLBACK}
    # one frame on its own is the frame in the batch
    k = gc.ROWS.index(1025)
    alone = g.ground([frames[k]], cfg, t[k:k + 1])
    assert alone["planes"].tobytes() == got["planes"][k].tobytes() and np.array_equal(alone["ground_words"][0], got["ground_words"][k])


def test_fixed_cases(pp, hip_lib):
    """The degenerate, tie, fallback and boundary cases of tests/test_ground_host.py on the GPU."""
    g = pp.ground
    p = gc.fixed_frame()
    for names, over in ((("collinear", "wall", "ceiling", "nan", "floor"), {}), (("wall", "floor", "floor", "floor2"), {}),
                        (("wall", "collinear"), {}), (("floor",), dict(min_inliers=14)), (("floor",), dict(min_inliers=13)),
                        (("floor", "floor2"), dict(refine=1))):
        cfg = dict(gc.FIXED_CFG, hypotheses=len(names), **over)
        t = gc.triples_for([gc.FIXED_TRIPLES[k] for k in names], len(p))[None]
        _same(pp, g.ground([p], cfg, t), [p], cfg, t, names)
    got = g.ground([p], dict(gc.FIXED_CFG, hypotheses=4), gc.triples_for([gc.FIXED_TRIPLES[k] for k in ("wall", "floor", "floor", "floor2")], len(p))[None])
    assert got["info"][0][:3].tolist() == [g.OK, 1, 13] and got["counts"][0].tolist() == [0, 13, 13, 13]
    rows, want, t = gc.boundary_frame()
    got = g.ground([rows], gc.BOUNDARY_CFG, t[None])
    _same(pp, got, [rows], gc.BOUNDARY_CFG, t[None], "boundary")
    assert np.array_equal(got["ground"][0], want) and got["planes"][0].tolist() == [0.25, 0.0, -1.0]
    got = g.ground([rows], gc.BOUNDARY_CFG_BELOW, t[None])
    _same(pp, got, [rows], gc.BOUNDARY_CFG_BELOW, t[None], "boundary, the threshold one double below")
    assert np.array_equal(got["ground"][0], gc.boundary_on_plane(rows)) and got["info"][0][2] == 3
    with pytest.raises(RuntimeError, match=r"pp_ground_points failed \(1\).*inlier_dist"):
        c = g.GroundConfig(**gc.BOUNDARY_CFG)
        c.inlier_dist = -1.0
        g.ground([rows], c, t[None])
    with pytest.raises(ValueError, match="refine needs"):
        g.ground([rows], dict(gc.BOUNDARY_CFG, refine=1, max_range=100.0), t[None])


# ---- on a handle ----
def _engine(pp):
    import nav_cycle_cases as nc
    assert nc.STREAMS == S and nc.F == oc.CYCLE_F
    return pp.Engine(nc.config(pp), max_batch=S, max_points_per_frame=NMAX)


def _start(e, ground, mask):
    e.set_tracking(oc.CYCLE_TRACK)
    e.set_tracking(None)
    e.track_reset()
    e.set_occupancy(oc.CYCLE_OCC)
    e.occupancy_reset()
    e.set_scan_match(oc.CYCLE_SCAN)
    e.set_costmap(oc.CYCLE_COSTMAP)
    e.set_object_mask(mask)
    e.set_ground(ground)


def _frames(i):
    return gc.cycle_frames(700 + i, ROWS_EMPTY if i == 1 else ROWS)


def _run_cycles(pp, e, ground, mask):
    """Three cycles in the README's order: upload, ground, the mask in front, scan match and occupancy update, the tracking
    step, the mask behind it, the costmap.  Returns everything fetched, cycle by cycle."""
    outs = []
    for i, c in enumerate(oc.cycles(pp)):
        o = {"frames": _frames(i)}
        e.upload(o["frames"])
        if ground:
            e.ground_async()
            o["planes"], o["ginfo"], o["gnd"], o["obs"], o["sums"], o["counts"] = e.ground(bits=True, debug=True)
        if mask:
            e.object_mask_async(c["poses"], c["dt"])
            o["front"], _ = e.object_mask()
        e.scan_match_async(c["poses"])
        o["words"], o["scores"], o["scan_classes"] = e.scan_match_results(scores=True, classes=True)
        o["corrected"] = e.scan_match_poses()
        e.occupancy_update_async(o["corrected"])
        o["occ"] = e.occupancy_maps(logodds=True) + (e.occupancy_info(masked=True, classes=True),)
        o["tracks"] = e.track_update(c["dets"], c["n"], c["dt"], c["poses"])
        if mask:
            e.object_mask_async()
            o["behind"], _ = e.object_mask()
        o["cm"] = e.costmaps(counts=True)
        o["cm_classes"] = e.costmap_info(classes=True)["classes"]
        outs.append(o)
    return outs


def _blob(outs):
    return b"".join(a.tobytes() for o in outs for a in (o["words"], o["scores"], o["corrected"], *o["occ"][:3], *o["cm"]))


@pytest.fixture(scope="module")
def runs(pp, hip_lib):
    """Engines over the same three cycles: plain (never sets the stage), all three readers named, the costmap alone named,
    the costmap alone NOT named, all three named together with the object mask (twice, on two engines), and the engine of
    "all" again after set_ground(None)."""
    out = {}
    only_cm = dict(gc.CYCLE_GROUND, consumers=("costmap",))
    not_cm = dict(gc.CYCLE_GROUND, consumers=("occupancy", "scan_match"))
    for name, ground, mask in (("plain", None, None), ("all", gc.CYCLE_GROUND, None), ("costmap", only_cm, None), ("not_costmap", not_cm, None),
                               ("both", gc.CYCLE_GROUND, oc.CYCLE_MASK), ("both2", gc.CYCLE_GROUND, oc.CYCLE_MASK)):
        e = _engine(pp)
        try:
            _start(e, ground, mask)
            if ground:
                assert e.ground_config == pp.ground.GroundConfig(**ground)
            else:
                assert e.ground_config is None
            out[name] = _run_cycles(pp, e, ground, mask)
            if name == "all":
                _start(e, None, None)
                out["off_again"] = _run_cycles(pp, e, None, None)
        finally:
            e.close()
    return out


def test_handle_equals_the_restatement_and_the_standalone_call(pp, runs):
    """Planes, info, bits, sums and counts of every cycle: ground_np's under draw_triples(seed, call index), and the bytes of
    ground.ground on the same rows (one frame of the middle cycle is empty)."""
    g = pp.ground
    cfg = gc.CYCLE_GROUND
    ok = 0
    for i, o in enumerate(runs["all"]):
        t = g.draw_triples(cfg["seed"], i, S, cfg["hypotheses"])
        alone = g.ground(o["frames"], cfg, t)
        for b, f in enumerate(o["frames"]):
            want = g.ground_np(f, cfg, t[b])
            assert o["planes"][b].tobytes() == want["plane"].tobytes() == alone["planes"][b].tobytes(), (i, b)
            assert [int(o["ginfo"][k][b]) for k in g.INFO] == want["info"].tolist() == alone["info"][b].tolist(), (i, b)
            assert np.array_equal(o["gnd"][b], want["ground"]) and np.array_equal(o["obs"][b], want["obstacle"]), (i, b)
            assert np.array_equal(alone["ground"][b], want["ground"]) and np.array_equal(alone["obstacle"][b], want["obstacle"]), (i, b)
            assert o["sums"][b].tolist() == want["sums"].tolist() and o["counts"][b].tolist() == want["counts"].tolist(), (i, b)
            ok += int(want["info"][0] == g.OK and want["info"][10] == 1)
    assert ok >= 6                   # most frames fit and refit; the empty one falls back
    assert runs["all"][1]["ginfo"]["status"][1] == g.FALLBACK and runs["all"][1]["ginfo"]["rows"][1] == 0


def _check_downstream(pp, outs, scan_named, occ_named, cm_named, masked):
    maps = [pp.occupancy.OccupancyMap(oc.CYCLE_OCC) for _ in range(S)]
    hits = 0
    for i, (c, o) in enumerate(zip(oc.cycles(pp), outs)):
        grid, org, lo, info = o["occ"]
        tr, nt, _ = o["tracks"]
        assert o["scan_classes"] == scan_named and info["classes"] == occ_named and o["cm_classes"] == cm_named
        for b in range(S):
            f = o["frames"][b]
            gnd = (o["gnd"][b], o["obs"][b]) if "gnd" in o else None
            front, behind = (o["front"][b], o["behind"][b]) if masked else (None, None)
            w, s = pp.scan_match.match_np(maps[b], f, c["poses"][b], oc.CYCLE_SCAN, mask=front, ground=gnd if scan_named else None)
            assert np.array_equal(o["words"][b], w) and np.array_equal(o["scores"][b], s), (i, b)
            want = maps[b].update(f, o["corrected"][b], mask=front, ground=gnd if occ_named else None)
            assert np.array_equal(grid[b], maps[b].grid()) and np.array_equal(lo[b], maps[b].logodds()), (i, b)
            assert {k: int(v[b]) for k, v in info.items() if k != "classes" and (masked or k != "masked")} == want, (i, b)
            assert np.array_equal(org[b], maps[b].origin)
            hits += want["hits"]
            gm, km = pp.costmap.costmap_np(f, oc.CYCLE_COSTMAP, tracks=tr[b], n_tracks=nt[b], mask=behind, ground=gnd if cm_named else None)
            assert np.array_equal(o["cm"][0][b], gm) and np.array_equal(o["cm"][1][b], km), (i, b)
    assert hits > 100
    return hits


def test_named_readers_equal_the_restatements_on_the_gpus_own_bits(pp, runs):
    """Scan-match words and all scores, occupancy grid, log-odds and info, costmap grid and counts: EQUAL to match_np,
    OccupancyMap.update and costmap_np fed the classes the GPU computed."""
    _check_downstream(pp, runs["all"], True, True, True, False)
    assert _blob(runs["all"]) != _blob(runs["plain"])       # the comparison sees the stage


def test_a_reader_not_named_runs_as_with_the_stage_off(pp, runs):
    """Each reader left out of `consumers` while the stage is on and has classes: the bytes of the engine that never set
    the stage (occupancy and scan match in the run that names the costmap alone, the costmap in the run that names the
    other two)."""
    _check_downstream(pp, runs["plain"], False, False, False, False)
    _check_downstream(pp, runs["costmap"], False, False, True, False)
    for o, w in zip(runs["costmap"], runs["plain"]):
        assert all(a.tobytes() == x.tobytes() for a, x in zip((o["words"], o["scores"], *o["occ"][:3]), (w["words"], w["scores"], *w["occ"][:3])))
        assert o["cm"][1].tobytes() != w["cm"][1].tobytes()
    # ... and the costmap not named while the other two are, classes computed: its grid and counts are the plain run's
    # bytes, the other two readers' results those of the run that names all three
    _check_downstream(pp, runs["not_costmap"], True, True, False, False)
    for o, w, a in zip(runs["not_costmap"], runs["plain"], runs["all"]):
        assert o["cm_classes"] is False and "gnd" in o
        assert o["cm"][0].tobytes() == w["cm"][0].tobytes() and o["cm"][1].tobytes() == w["cm"][1].tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip((o["words"], o["scores"], *o["occ"][:3]), (a["words"], a["scores"], *a["occ"][:3])))


def test_classes_and_object_mask_together(pp, runs):
    """Both apply: a masked OBSTACLE row is a masked end, takes no part in the match and adds no count."""
    _check_downstream(pp, runs["both"], True, True, True, True)
    masked = sum(int(o["occ"][3]["masked"].sum()) for o in runs["both"])
    assert masked > 20
    assert _blob(runs["both"]) != _blob(runs["all"])


def test_stage_off_again_and_two_runs(pp, runs):
    """set_ground(None) after use: every reader's outputs are the bytes of a handle that never had the stage.  The
    three-cycle run with every stage on, twice with the same seed: the same bytes."""
    assert _blob(runs["off_again"]) == _blob(runs["plain"])
    assert _blob(runs["both"]) == _blob(runs["both2"])
    for a, b in zip(runs["both"], runs["both2"]):
        assert a["planes"].tobytes() == b["planes"].tobytes() and a["counts"].tobytes() == b["counts"].tobytes()


def test_refusals_and_stale_classes(pp, hip_lib):
    """Each of the three named readers refuses without classes of the resident frames, and again after an upload, a crop
    and a sweep accumulation (an ingest: the next test).  Explicit triples; batch 1."""
    import nav_cycle_cases as nc
    g = pp.ground
    c0, c1 = oc.cycles(pp)[:2]
    e = _engine(pp)
    try:
        with pytest.raises(RuntimeError, match="ground_async: the ground stage is not configured"):
            e.ground_async()
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*pp_set_ground: hypotheses = 513"):
            bad = g.GroundConfig()
            bad.hypotheses = 513
            e.set_ground(bad)
        with pytest.raises(ValueError, match="refine needs max_range"):
            e.set_ground(dict(max_range=100.0))
        _start(e, gc.CYCLE_GROUND, None)
        e.set_sweeps(nc.SWEEPS)
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_ground_async: no frames are resident"):
            e.ground_async()
        frames = _frames(0)
        e.upload(frames)
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_get_ground: no ground plane has been computed"):
            e.ground()
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_occupancy_update_async: the ground stage names this stage"):
            e.occupancy_update_async(c0["poses"])
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_scan_match_async: the ground stage names this stage"):
            e.scan_match_async(c0["poses"])
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_costmap_async: the ground stage names this stage"):
            e.costmap_async()
        with pytest.raises(ValueError, match="triples must be uint32"):
            e.ground_async(np.zeros((S, 3, 3), np.uint32))
        t = g.draw_triples(99, 0, S, gc.CYCLE_GROUND["hypotheses"])
        e.ground_async(t)
        planes, info = e.ground()
        for b in range(S):
            assert planes[b].tobytes() == g.ground_np(frames[b], gc.CYCLE_GROUND, t[b])["plane"].tobytes()
        e.occupancy_update_async(c0["poses"])
        stamps = np.arange(S, dtype=np.float64)
        for stale in (lambda: e.upload(_frames(2)), lambda: e.crop_to_image(nc.planes(pp)), lambda: e.accumulate_sweeps(c1["poses"], stamps + 0.1)):
            e.ground_async()
            e.scan_match_async(c1["poses"])
            e.costmaps()
            assert e.costmap_info(classes=True)["classes"] is True
            stale()
            with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_costmap_async: the ground stage names this stage"):
                e.costmap_async()
            with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_occupancy_update_async: the ground stage names this stage"):
                e.occupancy_update_async(c1["poses"])
            with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_scan_match_async: the ground stage names this stage"):
                e.scan_match_async(c1["poses"])
            with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_get_ground: the frames the last classes belong to are gone"):
                e.ground()
        # a new configuration makes the last classes stale; the same one again does not
        e.ground_async()
        e.set_ground(gc.CYCLE_GROUND)
        e.scan_match_async(c1["poses"])
        e.set_ground(dict(gc.CYCLE_GROUND, consumers=("occupancy",), ground_dist=0.06))
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_occupancy_update_async: the ground stage names this stage"):
            e.occupancy_update_async(c1["poses"])
        # batch 1
        e.upload(frames[:1])
        e.ground_async(t[:1])
        planes, info, gnd, obs = e.ground(bits=True)
        want = g.ground_np(frames[0], dict(gc.CYCLE_GROUND, ground_dist=0.06), t[0])
        assert planes.shape == (1, 3) and planes[0].tobytes() == want["plane"].tobytes()
        assert np.array_equal(gnd[0], want["ground"]) and np.array_equal(obs[0], want["obstacle"])
        e.occupancy_update_async(c1["poses"][:1])
        assert e.occupancy_info(classes=True)["classes"] is True
    finally:
        e.close()


def test_an_ingest_makes_the_classes_stale(pp, hip_lib):
    """On a 3-feature engine (the depth ingest's), all three readers named: upload, classes, the readers run; an ingest of
    a depth image; each of them refuses until the stage has run again, and the costmap then equals the restatement on the
    ingested rows."""
    g = pp.ground
    e = pp.Engine(pp.config.tiny_config(1), max_batch=1, max_points_per_frame=2048)
    grid = dict(x_min=0.0, y_min=-1.0, resolution=0.05, width=40, height=40, z_min=-1.0, z_max=1.0, objects=0)
    cfg = dict(gc.CYCLE_GROUND, cand_z_max=2.0, h_max=3.0, fallback_c=-1.0)
    pose = pp.sweeps.pose_from_xyyaw(0.0, 0.0, 0.0)[None]
    try:
        e.set_costmap(grid)
        e.set_occupancy(oc.CYCLE_OCC)
        e.set_scan_match(oc.CYCLE_SCAN)
        e.set_ground(cfg)
        f = gc.cycle_frames(5, (300,), F=3)
        e.upload(f)
        e.ground_async()
        _, _, gnd, obs = e.ground(bits=True)
        gm, km = e.costmaps(counts=True)
        wg, wk = pp.costmap.costmap_np(f[0], grid, ground=(gnd[0], obs[0]))
        assert np.array_equal(gm[0], wg) and np.array_equal(km[0], wk) and wk.sum() > 50
        e.scan_match_async(pose)
        e.occupancy_update_async(pose)
        img, k = pp.synth.depth_image(3, 64, 48)
        rows = e.ingest_depth([img], k, return_points=True)
        for name, call in (("pp_costmap_async", e.costmap_async), ("pp_occupancy_update_async", lambda: e.occupancy_update_async(pose)),
                           ("pp_scan_match_async", lambda: e.scan_match_async(pose))):
            with pytest.raises(RuntimeError, match=f"PP_ERR_STATE.*{name}: the ground stage names this stage"):
                call()
        e.ground_async()
        planes, info, gnd, obs = e.ground(bits=True)
        want = g.ground_np(rows[0], cfg, g.draw_triples(cfg["seed"], 1, 1, cfg["hypotheses"])[0])
        assert planes[0].tobytes() == want["plane"].tobytes() and np.array_equal(obs[0], want["obstacle"])
        gm, km = e.costmaps(counts=True)
        wg, wk = pp.costmap.costmap_np(rows[0], grid, ground=(gnd[0], obs[0]))
        assert np.array_equal(gm[0], wg) and np.array_equal(km[0], wk)
        e.scan_match_async(pose)
        e.occupancy_update_async(pose)
        assert e.occupancy_info(classes=True)["classes"] is True and e.scan_match_results(classes=True)[1] is True
        # the same seed and K given again: the call index goes on, the next drawn triples are call 2's
        e.set_ground(cfg)
        e.ground_async()
        want = g.ground_np(rows[0], cfg, g.draw_triples(cfg["seed"], 2, 1, cfg["hypotheses"])[0])
        assert e.ground()[0][0].tobytes() == want["plane"].tobytes()
    finally:
        e.close()
