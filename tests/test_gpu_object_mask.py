"""The per-point object mask on the GPU (csrc/object_mask.hip: k_objmask_table, k_objmask_rows; the readers' side of it in
k_occ_endpoints, k_scan_cells, k_costmap_points) against object_mask.py's restatement.  The stand-alone entry must EQUAL the
restatement (np.array_equal): the rule is float64 + - * and comparisons and the library is built without contraction; only
the cos / sin of a footprint's yaw may differ in the last place between the two, so the seeded cases are those that leave
no row within 1e-9 m of a footprint's edge (asserted), and the boundary cases use yaw 0.  On a handle the downstream maps are
compared with NO tolerance: the host restatements are fed the GPU's own bits."""
import ctypes
import math

import numpy as np
import pytest

import object_mask_cases as oc

pytestmark = pytest.mark.gpu

S = oc.CYCLE_STREAMS
NMAX = 512


def _config(pp, B=S):
    import nav_cycle_cases as nc
    assert nc.STREAMS == S and nc.F == oc.CYCLE_F
    return nc.config(pp)


def _engine(pp):
    return pp.Engine(_config(pp), max_batch=S, max_points_per_frame=NMAX)


# ---- 1. the stand-alone entry ----
def _standalone(pp, frames, rects, pad, what):
    om = pp.object_mask
    masks, words, info = om.object_mask(frames, rects, pad)
    for b, (f, r) in enumerate(zip(frames, rects)):
        fp = om.rect_footprints_np(r, pad)
        assert not (om.point_margins_np(f, fp) < oc.MARGIN).any(), (what, b)
        want = om.object_mask_np(f, fp)
        assert np.array_equal(masks[b], want), (what, b)
        assert info[b].tolist() == [len(fp), int(want.sum()), len(f), 0], (what, b)
        assert np.array_equal(words[b], om.pack_words(want, words.shape[1])), (what, b)      # zero past the frame's rows
    return words, info


def test_standalone_sizes(pp, hip_lib):
    """Every row count of {0, 1, 63, 64, 65, 257} and every footprint count of {0, 1, 63, 64, 65, 128}, as the frames of one
    call; two runs give the same bytes."""
    rng = np.random.default_rng(77)
    sizes = oc.size_cases()
    frames = [oc.seeded_rows(rng, r, F=3) for r, _ in sizes]
    rects = [oc.seeded_rects(rng, k) for _, k in sizes]
    words, info = _standalone(pp, frames, rects, 0.0, "sizes")
    assert words.shape == (len(sizes), 5) and info[:, 1].sum() > 100
    w2, i2 = _standalone(pp, frames, rects, 0.0, "sizes again")
    assert w2.tobytes() == words.tobytes() and i2.tobytes() == info.tobytes()
    # one frame on its own is the frame in the batch
    k = next(i for i, (r, q) in enumerate(sizes) if r == 257 and q == 128)
    w1, _ = _standalone(pp, [frames[k]], [rects[k]], 0.0, "alone")
    assert w1[0].tobytes() == words[k].tobytes()


@pytest.mark.parametrize("seed", oc.SEEDS)
def test_standalone_unequal_frames(pp, hip_lib, seed):
    frames, rects, pad = oc.seeded_case(seed)
    _, info = _standalone(pp, frames, rects, pad, f"seed {seed}")
    assert info[:, 1].sum() > 0


def test_standalone_boundary_and_refusals(pp, hip_lib):
    om = pp.object_mask
    rows, inside = oc.boundary_rows()
    masks, _, info = om.object_mask([rows], [oc.BOUNDARY_RECT])
    assert np.array_equal(masks[0], inside) and info[0].tolist() == [1, int(inside.sum()), len(rows), 0]
    masks, _, info = om.object_mask([rows], [np.array([[1.0, 2.0, np.nan, 0.5, 0.0], [1.0, np.inf, 1.0, 0.5, 0.0]])])
    assert not masks[0].any() and info[0].tolist() == [0, 0, len(rows), 0]
    bad = np.array([[np.nan, 2.0, 0], [1.0, np.nan, 0], [np.inf, 2.0, 0]], np.float32)
    assert not om.object_mask([bad], [oc.BOUNDARY_RECT])[0][0].any()
    with pytest.raises(RuntimeError, match=r"pp_object_mask_points failed \(1\).*counts\[0\] = 129"):
        om.object_mask([rows], [np.tile(oc.BOUNDARY_RECT, (129, 1))])
    with pytest.raises(RuntimeError, match=r"pp_object_mask_points failed \(1\).*pad"):
        om.object_mask([rows], [oc.BOUNDARY_RECT], pad=-1.0)


# ---- 2. on a handle ----
def _start(pp, e, mask=oc.CYCLE_MASK):
    e.set_tracking(oc.CYCLE_TRACK)
    e.set_tracking(None)                    # the stage needs the configuration, not the switch
    e.track_reset()
    e.set_occupancy(oc.CYCLE_OCC)
    e.occupancy_reset()
    e.set_scan_match(oc.CYCLE_SCAN)
    e.set_costmap(oc.CYCLE_COSTMAP)
    e.set_object_mask(mask)


def _occ_fetch(e):
    grid, org, lo = e.occupancy_maps(logodds=True)
    return grid, org, lo, e.occupancy_info(masked=True)


def _psi(P):
    return math.atan2(float(P[1, 0]), float(P[0, 0]))


def _run_cycles(pp, e, masked, consumers_on=True):
    """The cycle of the README on hand-fed track rows: upload, the mask in front (poses, dt), scan match and occupancy
    update, the tracking step, the mask behind it, the costmap.  Returns everything fetched, cycle by cycle."""
    outs, prev = [], None
    for c in oc.cycles(pp):
        o = {}
        e.upload(c["frames"])
        if masked:
            before = tuple(a.tobytes() for a in e.tracks(S)) if prev is not None else None
            e.object_mask_async(c["poses"], c["dt"])
            o["front"], o["front_info"] = e.object_mask()
            o["prev"] = prev
            if before is not None:
                assert tuple(a.tobytes() for a in e.tracks(S)) == before                   # a peek, not a step
        e.scan_match_async(c["poses"])
        o["words"], o["scores"] = e.scan_match_results(scores=True)
        o["corrected"] = e.scan_match_poses()
        e.occupancy_update_async(o["corrected"])
        o["occ"] = _occ_fetch(e)
        o["tracks"] = e.track_update(c["dets"], c["n"], c["dt"], c["poses"])
        prev = c["poses"]
        if masked:
            e.object_mask_async()
            o["behind"], o["behind_info"] = e.object_mask()
        o["cm"] = e.costmaps(counts=True)
        outs.append(o)
    return outs


@pytest.fixture(scope="module")
def runs(pp, hip_lib):
    """Two engines over the same three cycles: one never sets the stage, one masks all three readers."""
    out = []
    for masked in (False, True):
        e = _engine(pp)
        try:
            _start(pp, e, oc.CYCLE_MASK if masked else None)
            if masked:
                assert e.object_mask_config == pp.object_mask.ObjectMaskConfig(**oc.CYCLE_MASK)
            else:
                assert e.object_mask_config is None
            out.append(_run_cycles(pp, e, masked))
        finally:
            e.close()
    return out


def test_tracks_masks_equal_the_restatement(pp, runs):
    """In front of the scan match (poses and dt bring a copy of the tracks to now) and behind the tracking step (the slots
    as they stand, yaw 0): the bits are the restatement's, and the tracking steps are those of the engine that never
    masked."""
    om = pp.object_mask
    plain, masked = runs
    some = 0
    for i, (c, o) in enumerate(zip(oc.cycles(pp), masked)):
        tr_prev = masked[i - 1]["tracks"] if i else None
        for b in range(S):
            f = c["frames"][b]
            if tr_prev is None:
                fp = np.zeros((0, 6))
            else:
                prev = o["prev"][b]
                fp = om.footprints_np(oc.CYCLE_MASK, tracks=tr_prev[0][b], n_tracks=tr_prev[1][b], pose=c["poses"][b],
                                      prev=(prev, _psi(prev)), dt=c["dt"][b])
            assert not (om.point_margins_np(f, fp) < oc.MARGIN).any(), (i, b)
            want = om.object_mask_np(f, fp)
            assert np.array_equal(o["front"][b], want), (i, b)
            assert [o["front_info"][k][b] for k in om.INFO] == [len(fp), int(want.sum()), len(f), 0], (i, b)
            tr, nt, _ = o["tracks"]
            fp = om.footprints_np(oc.CYCLE_MASK, tracks=tr[b], n_tracks=nt[b])
            assert len(fp) == 2 and not (om.point_margins_np(f, fp) < oc.MARGIN).any()
            want = om.object_mask_np(f, fp)
            assert np.array_equal(o["behind"][b], want), (i, b)
            some += int(want.sum())
        for a, w in zip(o["tracks"], plain[i]["tracks"]):
            assert a.tobytes() == w.tobytes(), i                                            # the tracker never noticed
    assert some > 300 and masked[0]["front_info"]["footprints"].tolist() == [0] * S


def test_downstream_maps_equal_the_restatements_on_the_gpus_own_bits(pp, runs):
    """Scan-match words and all scores, occupancy grid, log-odds and info with `masked`, costmap grid and counts: EQUAL to
    match_np, OccupancyMap.update and costmap_np fed the bits the GPU computed."""
    _, masked = runs
    maps = [pp.occupancy.OccupancyMap(oc.CYCLE_OCC) for _ in range(S)]
    seen = 0
    for i, (c, o) in enumerate(zip(oc.cycles(pp), masked)):
        grid, org, lo, info = o["occ"]
        tr, nt, _ = o["tracks"]
        for b in range(S):
            f = c["frames"][b]
            w, s = pp.scan_match.match_np(maps[b], f, c["poses"][b], oc.CYCLE_SCAN, mask=o["front"][b])
            assert np.array_equal(o["words"][b], w) and np.array_equal(o["scores"][b], s), (i, b)
            want = maps[b].update(f, o["corrected"][b], mask=o["front"][b])
            assert np.array_equal(grid[b], maps[b].grid()) and np.array_equal(lo[b], maps[b].logodds()), (i, b)
            assert {k: int(v[b]) for k, v in info.items()} == want, (i, b)
            assert np.array_equal(org[b], maps[b].origin)
            seen += want["masked"]
            g, k = pp.costmap.costmap_np(f, oc.CYCLE_COSTMAP, tracks=tr[b], n_tracks=nt[b], mask=o["behind"][b])
            und = pp.costmap.decision_margins(oc.CYCLE_COSTMAP, pp.costmap.footprints_np(oc.CYCLE_COSTMAP, tracks=tr[b], n_tracks=nt[b])) < oc.MARGIN
            assert not und.any()
            assert np.array_equal(o["cm"][0][b], g) and np.array_equal(o["cm"][1][b], k), (i, b)
    assert seen > 100          # masked ends did reach the maps


def test_stage_off_is_todays_chain(pp, runs):
    """The engine that never set the stage: its matches, maps and costmaps over the three cycles are the bytes of the
    restatements without a mask; and they differ from the masked engine's, so the comparison sees the stage."""
    plain, masked = runs
    maps = [pp.occupancy.OccupancyMap(oc.CYCLE_OCC) for _ in range(S)]
    for i, (c, o) in enumerate(zip(oc.cycles(pp), plain)):
        grid, org, lo, info = o["occ"]
        assert info["masked"].tolist() == [0] * S
        tr, nt, _ = o["tracks"]
        for b in range(S):
            f = c["frames"][b]
            w, s = pp.scan_match.match_np(maps[b], f, c["poses"][b], oc.CYCLE_SCAN)
            assert np.array_equal(o["words"][b], w) and np.array_equal(o["scores"][b], s), (i, b)
            want = maps[b].update(f, o["corrected"][b])
            assert np.array_equal(grid[b], maps[b].grid()) and np.array_equal(lo[b], maps[b].logodds()), (i, b)
            assert {k: int(v[b]) for k, v in info.items() if k != "masked"} == want, (i, b)
            g, k = pp.costmap.costmap_np(f, oc.CYCLE_COSTMAP, tracks=tr[b], n_tracks=nt[b])
            assert np.array_equal(o["cm"][0][b], g) and np.array_equal(o["cm"][1][b], k), (i, b)
    assert plain[2]["occ"][2].tobytes() != masked[2]["occ"][2].tobytes()
    assert plain[2]["cm"][1].tobytes() != masked[2]["cm"][1].tobytes()


def test_validity_refusals_and_reconfiguration(pp, hip_lib):
    """A mask goes stale with the frames it belongs to (upload, crop, sweeps): a named reader then refuses, a reader that
    is not named runs unmasked.  Every refusal leaves the last mask where it was.  set_occupancy to another width between
    two masked updates."""
    import nav_cycle_cases as nc
    om = pp.object_mask
    cyc = oc.cycles(pp)
    c0, c1 = cyc[0], cyc[1]
    e = _engine(pp)
    try:
        # the stage off, and tracks before any pp_set_tracking
        e.upload(c0["frames"])
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_object_mask_async: the object mask is not configured"):
            e.object_mask_async()
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_get_object_mask: no mask has been computed"):
            e.object_mask()
        e.set_object_mask(dict(oc.CYCLE_MASK, consumers=("occupancy", "scan_match")))
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_object_mask_async: objects = tracks and pp_set_tracking has given no configuration"):
            e.object_mask_async()
        _start(pp, e, dict(oc.CYCLE_MASK, consumers=("occupancy", "scan_match")))
        e.set_sweeps(nc.SWEEPS)
        e.upload(c0["frames"])
        e.track_update(c0["dets"], c0["n"], c0["dt"], c0["poses"])
        # a named reader without a mask refuses; the costmap is not named and runs unmasked
        for call, who in ((lambda: e.occupancy_update_async(c0["poses"]), "pp_occupancy_update_async"),
                          (lambda: e.scan_match_async(c0["poses"]), "pp_scan_match_async")):
            with pytest.raises(RuntimeError, match=f"PP_ERR_STATE.*{who}: the object mask names this stage.*pp_object_mask_async first"):
                call()
        tr, nt, _ = e.tracks(S)
        g, k = e.costmaps(counts=True)
        for b in range(S):
            wg, wk = pp.costmap.costmap_np(c0["frames"][b], oc.CYCLE_COSTMAP, tracks=tr[b], n_tracks=nt[b])
            assert np.array_equal(g[b], wg) and np.array_equal(k[b], wk)
        e.object_mask_async()
        masks, info = e.object_mask()
        last = (b"".join(m.tobytes() for m in masks), {k: v.tobytes() for k, v in info.items()})
        same = lambda: (lambda m, i: (b"".join(x.tobytes() for x in m), {k: v.tobytes() for k, v in i.items()}))(*e.object_mask()) == last   # noqa: E731
        assert info["masked"].sum() > 50
        # ---- refusals, each leaving the last mask as it is ----
        bad_pose = c0["poses"].copy()
        bad_pose[1, 0, 0] = 2.0
        nan_pose = c0["poses"].copy()
        nan_pose[2, 1, 3] = np.nan
        L, h = e._lib, e._h
        P, t = np.ascontiguousarray(c0["poses"]), np.ascontiguousarray(c0["dt"])
        for call, code, text in (
                (lambda: e.object_mask_async(dt=[0.1, -0.1, 0.1]), "PP_ERR_ARG", "dt of stream 1 is -0.1"),
                (lambda: e.object_mask_async(dt=[0.1, 0.1, np.nan]), "PP_ERR_ARG", "dt of stream 2 is nan"),
                (lambda: e.object_mask_async(poses=bad_pose), "PP_ERR_ARG", "the rotation of stream 1 is not orthonormal"),
                (lambda: e.object_mask_async(poses=nan_pose), "PP_ERR_ARG", "stream 2: row 1, column 3 is not finite"),
                (lambda: e._check(L.pp_object_mask_async(h, P.ctypes.data, t.ctypes.data, 2), "pp_object_mask_async"), "PP_ERR_ARG",
                 "3 frames are resident, batch is 2"),
                (lambda: e._check(L.pp_object_mask_async(h, None, None, S + 1), "pp_object_mask_async"), "PP_ERR_ARG", "batch 4 outside"),
                (lambda: e._check(L.pp_get_object_mask(h, None, None, 2), "pp_get_object_mask"), "PP_ERR_ARG", "the last mask had 3 frames, batch is 2")):
            with pytest.raises(RuntimeError, match=f"{code}.*{text}"):
                call()
            assert same(), text
        pc = pp._lib.PPObjectMaskConfig()
        for field, value in (("pad", -0.5), ("min_speed", -1.0), ("min_score", math.nan), ("objects", 0), ("objects", 3), ("consumers", 8),
                             ("reserved", 1), ("pad", math.inf)):
            for f, v in om.ObjectMaskConfig(**oc.CYCLE_MASK).to_dict().items():
                setattr(pc, f, v)
            pc.reserved = 0
            setattr(pc, field, value)
            assert L.pp_set_object_mask(h, ctypes.byref(pc)) == 1, field
            assert field.encode() in L.pp_last_error(h), (field, L.pp_last_error(h))
            assert same(), field
        assert e.object_mask_config.consumers == ("occupancy", "scan_match")
        # objects = detections: no pass has run on these frames, and it takes neither poses nor dt
        e.set_object_mask(dict(oc.CYCLE_MASK, objects="detections"))
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*objects = detections and no pass has run on the resident frames"):
            e.object_mask_async()
        with pytest.raises(RuntimeError, match="PP_ERR_ARG.*objects = detections takes neither poses nor dt"):
            e.object_mask_async(dt=c0["dt"])
        e.set_object_mask(dict(oc.CYCLE_MASK, consumers=("occupancy", "scan_match")))
        # ---- validity: upload, crop, sweeps ----
        e.object_mask_async()
        e.occupancy_update_async(c0["poses"])                  # runs: the mask is of these frames
        stamps = np.arange(S, dtype=np.float64)
        for k, stale in enumerate((lambda: e.upload(c1["frames"]), lambda: e.crop_to_image(nc.planes(pp)),
                                   lambda: e.accumulate_sweeps(c1["poses"], stamps + 0.1))):
            e.object_mask_async()
            e.scan_match_async(c1["poses"])
            stale()
            with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_occupancy_update_async: the object mask names this stage"):
                e.occupancy_update_async(c1["poses"])
            with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_scan_match_async: the object mask names this stage"):
                e.scan_match_async(c1["poses"])
            with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_get_object_mask: the frames the last mask belongs to are gone"):
                e.object_mask()
            e.costmap_async()                                  # not named: runs
            e.costmaps()
        # ---- reconfiguration: another width between two masked updates ----
        e.upload(c1["frames"])
        e.object_mask_async(c1["poses"], c1["dt"])
        bits, _ = e.object_mask()
        e.occupancy_update_async(c1["poses"])
        wide = dict(oc.CYCLE_OCC, width=41)
        e.set_occupancy(wide)                                  # forgets every map; the mask is still the frames'
        e.occupancy_update_async(c1["poses"])
        grid, org, lo, info = _occ_fetch(e)
        assert grid.shape == (S, 29, 41)
        for b in range(S):
            m = pp.occupancy.OccupancyMap(wide)
            want = m.update(c1["frames"][b], c1["poses"][b], mask=bits[b])
            assert np.array_equal(grid[b], m.grid()) and np.array_equal(lo[b], m.logodds())
            assert {k: int(v[b]) for k, v in info.items()} == want
        # off again: the readers run unmasked
        e.set_object_mask(None)
        assert e.object_mask_config is None
        e.upload(c1["frames"])
        e.occupancy_update_async(c1["poses"])
        assert e.occupancy_info(masked=True)["masked"].tolist() == [0] * S
        assert list(e.occupancy_info()) == list(nc.OCC_INFO)
    finally:
        e.close()


def _weights(pp, d, seed=7):
    w = dict(pp.weights.init_weights(d, seed=seed))
    w["rpn/conv_cls/bias"] = np.array(w["rpn/conv_cls/bias"], np.float32) + np.float32(0.6)
    return w


def _pass_frames(B):
    """The seeded clouds of tests/test_gpu_costmap.py, for which the passes on the weights above keep rows."""
    out = []
    for b in range(B):
        rng = np.random.default_rng(300 + b)
        out.append(rng.uniform([0.05, -0.6, -2.5], [1.3, 0.6, 2.5], (700 + 150 * b, 3)).astype(np.float32))
    return out


def test_detections_behind_a_real_pass(pp, hip_lib):
    om = pp.object_mask
    B = 2
    e = pp.Engine(pp.config.tiny_config(B), max_batch=B, max_points_per_frame=4096)
    try:
        e.load_weights(_weights(pp, e.d))
        rect, trv, _ = pp.synth.default_calib()
        frames = _pass_frames(B)
        dets, n = e.detect(frames, np.stack([rect] * B), np.stack([trv] * B))
        plain = (dets.tobytes(), n.tobytes())
        assert int(n.min()) >= 2, n
        cfg = dict(objects="detections", min_score=float(np.median(dets["score"][0, :n[0]])), pad=0.02, consumers=("costmap",))
        e.set_object_mask(cfg)
        e.object_mask_async()
        masks, info = e.object_mask()
        left_out = total = 0
        for b in range(B):
            fp = om.footprints_np(cfg, dets=dets[b], n_dets=n[b])
            und = om.point_margins_np(frames[b], fp) < oc.MARGIN
            want = om.object_mask_np(frames[b], fp)
            assert np.array_equal(masks[b][~und], want[~und]), b
            assert info["footprints"][b] == len(fp) and info["rows"][b] == len(frames[b]) and info["flagged"][b] == 0
            assert info["masked"][b] == int(masks[b].sum())
            left_out += int(und.sum())
            total += len(frames[b])
        cap = int(oc.UNDECIDED_CAP * total)
        print(f"detections behind a pass: {left_out} of {total} rows undecided (cap {cap}); masked {info['masked'].tolist()}, "
              f"footprints {info['footprints'].tolist()}")
        assert left_out <= cap
        assert 1 <= info["footprints"][0] < n[0] and info["masked"].sum() > 0
        d2, n2 = e.detections()
        assert (d2.tobytes(), n2.tobytes()) == plain           # the results are the same bytes after the stage
        # the costmap on the GPU's own bits: the points of the detected objects are out of the point layer
        grid = dict(x_min=-0.5, y_min=-1.0, resolution=0.05, width=51, height=43, z_min=-3.0, z_max=3.0, point_cost=40)
        e.set_costmap(grid)
        g, k = e.costmaps(counts=True)
        for b in range(B):
            wg, wk = pp.costmap.costmap_np(frames[b], grid, mask=masks[b])
            assert np.array_equal(g[b], wg) and np.array_equal(k[b], wk), b
            assert wk.sum() == pp.costmap.costmap_np(frames[b], grid)[1].sum() - masks[b].sum()    # (every row lies in the grid and the band)
        # a new pass on new frames: the mask of the old ones is stale
        e.upload([f[::2] for f in frames])
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*pp_costmap_async: the object mask names this stage"):
            e.costmap_async()
        with pytest.raises(RuntimeError, match="PP_ERR_STATE.*no pass has run on the resident frames"):
            e.object_mask_async()
    finally:
        e.close()


def test_refusals_while_a_training_step_is_in_flight(pp, hip_lib):
    B = 2
    cfg = pp.config.tiny_config(B)
    tr = pp.Trainer(cfg, pp.weights.init_weights(pp.config.Derived(cfg), seed=7), max_batch=B, max_points_per_frame=4096,
                    learning_rate=2e-4, weight_decay=1e-4)
    e = tr.engine
    try:
        e.set_tracking(oc.CYCLE_TRACK)
        e.set_tracking(None)
        mask = dict(oc.CYCLE_MASK, consumers=("costmap",))
        e.set_object_mask(mask)
        frames = _pass_frames(B)
        e.upload(frames)
        e.object_mask_async()
        gts = [np.array([[0.8, 0.2 * b, 0.0, 0.6, 0.8, 1.73, 0.1]], np.float32) for b in range(B)]
        e.train_step_gt_async(tr.params.data_ptr(), tr.grads.data_ptr(), tr.state.data_ptr(), *e.pack_gt(gts))
        for call, what in ((lambda: e.set_object_mask(dict(mask, pad=0.1)), "pp_set_object_mask"), (lambda: e.set_object_mask(None), "pp_set_object_mask"),
                           (lambda: e.object_mask_async(), "pp_object_mask_async")):
            with pytest.raises(RuntimeError, match=f"PP_ERR_STATE.*{what}: a training step is in flight"):
                call()
        assert np.isfinite(e.train_step_wait()["loss"])
        assert e.object_mask_config == pp.object_mask.ObjectMaskConfig(**mask)
        e.upload(frames)
        e.object_mask_async()
        masks, info = e.object_mask()
        assert info["footprints"].tolist() == [0, 0] and not any(m.any() for m in masks)
    finally:
        tr.close()
