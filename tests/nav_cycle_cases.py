"""One navigation cycle with every resident-frame stage on: the scenario, the chain of the package's own numpy restatements
(HostChain / host_chain) and the comparison both tests/test_nav_cycle_host.py and tests/test_gpu_nav_cycle.py hold a run to.
Pure numpy up to `configure`; the functions below it drive an Engine and are shared by the GPU tests and by the child process
one of them starts (python tests/nav_cycle_cases.py).

A cycle is a dict: frames [B x [n, 4] float32], poses [B, 3, 4], stamps [B], planes [B, 6, 4]; the tracker's dt comes from
the stamps (tracking.stamps_to_dt).  What a cycle gives is a dict as well: HostChain.step fills every key, a GPU run the
keys it fetched (fetch_all), and same_as_chain / same_bytes compare the keys they find."""
import copy
import hashlib
import os
import re

import numpy as np

STREAMS = 3
NMAX = 512
F = 4
MARGIN = 1e-9        # metres: under it a costmap cell's membership is undecided (tests/test_gpu_costmap.py)
UNDECIDED_CAP = 0.001

# ---- stage configurations, each the one its own test file uses ----
SWEEPS = {"history": 2, "capacity": 200, "history_decimate": 1, "max_age": 0.25, "time_feature": 3}
TRACK = dict(gate=1.25, birth_score=0.3, max_misses=2, min_hits=2, q_acc=4.0, r_pos=0.01)
GRID = dict(x_min=-0.5, y_min=-1.0, resolution=0.05, width=51, height=43, z_min=-1.0, z_max=1.0)
COSTMAP = dict(GRID, objects="tracks", horizon_steps=2)
OCC = dict(resolution=0.1, z_min=0.0, z_max=1.0, max_range=2.5, width=37, height=29)
INFL_COSTMAP = dict(resolution=0.05, inscribed_radius=0.05, inflation_radius=0.2, cost_scaling_factor=8.0)          # 4 cells
INFL_OCC = dict(resolution=0.1, inscribed_radius=0.1, inflation_radius=0.5, cost_scaling_factor=4.0, lethal_threshold=65)   # 5 cells
IMAGE_SHAPES = [(8, 4), (6, 5), (10, 3)]      # (height, width) per stream under default_calib's identity camera matrix

# rows of stream 0, 1, 2 per cycle, from {0, 1, 63, 64, 65, 257}: empty, a single row, a wave and one row either side of
# it, two chunks of 256 rows (tests/test_gpu_sweeps.py); every stream sees all six, cycle 0 has no empty frame, and
# stream 0's three 257s in a row overflow both the sweeps' capacity (200) and the frame (512)
SIZES = [[257, 64, 65], [257, 65, 1], [257, 63, 257], [0, 257, 64], [65, 1, 257], [63, 0, 65], [257, 257, 0], [64, 257, 257],
         [1, 65, 63]]
GAP_AFTER = 4        # the stamps jump by more than max_age between cycles 4 and 5

OCC_INFO = ("hits", "ground", "ignored", "cells_hit", "cells_free", "cleared")
SWEEP_INFO = ("count", "used", "truncated", "push_truncated")
TRACK_FIELDS = ("state", "size", "yaw", "score", "id", "label", "hits", "misses", "confirmed", "det_row", "reserved")


def ring_turn(pp):
    """2 * OFF_RING + 1 calls: one more than two turns of a call ring, with the depth read from csrc/pp_ring.h."""
    with open(os.path.join(os.path.dirname(pp._lib.__file__), "csrc", "pp_ring.h")) as f:
        depth = int(re.search(r"constexpr\s+int\s+OFF_RING\s*=\s*(\d+)\s*;", f.read()).group(1))
    return 2 * depth + 1


def config(pp):
    cfg = copy.deepcopy(pp.config.tiny_config(STREAMS))
    cfg["model"]["second"]["num_point_features"] = F
    for reader in ("eval_input_reader", "train_input_reader"):
        if reader in cfg:
            cfg[reader]["num_point_features"] = F
    return cfg


def weights(pp, d):
    w = dict(pp.weights.init_weights(d, seed=7))
    w["rpn/conv_cls/bias"] = np.array(w["rpn/conv_cls/bias"], np.float32) + np.float32(0.6)     # the passes keep rows
    return w


def calib(pp, B=STREAMS):
    rect, trv, p2 = pp.synth.default_calib()
    return np.stack([rect] * B), np.stack([trv] * B), np.asarray(p2, np.float64)


def planes(pp):
    rect, trv, p2 = pp.synth.default_calib()
    return np.stack([pp.frustum.frustum_planes(rect, trv, p2, shp) for shp in IMAGE_SHAPES])


def _frame(rng, n):
    """n rows inside the tiny range (x 0 .. 1.6, y -0.64 .. 0.64).  The camera of default_calib looks along +x and its
    image holds y < 0, z < 0 only, so nine rows in ten are drawn there (the crop keeps most of them, and drops those too
    close to the sensor for the image); the others, 0 < z < 1, are what the crop drops and the occupancy map counts as hits."""
    seen = rng.random(n) < 0.9
    x = rng.uniform(0.05, 1.55, n)
    y = np.where(seen, rng.uniform(-0.6, -0.01, n), rng.uniform(-0.6, 0.6, n))
    z = np.where(seen, rng.uniform(-1.0, -0.01, n), rng.uniform(0.05, 1.0, n))
    return np.ascontiguousarray(np.stack([x, y, z, rng.random(n)], 1).astype(np.float32))


def sequence(pp, cycles=None, seed=11):
    """`cycles` (default: ring_turn) cycles of STREAMS frames: a slow planar ego motion per stream that carries the
    occupancy window over cell borders, stamps 0.1 s apart (stream b offset by b seconds) with one gap of 0.5 s."""
    cycles = ring_turn(pp) if cycles is None else cycles
    rng = np.random.default_rng(seed)
    pl = planes(pp)
    out = []
    for i in range(cycles):
        row = SIZES[i % len(SIZES)]
        frames = [_frame(rng, n) for n in row]
        poses = np.stack([pp.sweeps.pose_from_xyyaw(0.04 * i + rng.normal() * 0.004, 0.03 * i * (b - 1) + rng.normal() * 0.004,
                                                    0.03 * i * (b + 1)) for b in range(STREAMS)])
        t = 0.1 * i + (0.4 if i > GAP_AFTER else 0.0)
        out.append(dict(frames=frames, poses=poses, stamps=np.array([t + b for b in range(STREAMS)]), planes=pl))
    return out


def short_at(cycles):
    """The cycle that runs with 2 of the 3 streams in the stream-independence cases: two thirds through, behind the stamp
    gap, where stream 1 holds two young sweeps again (a reset that did nothing would show) and the next cycles' frames
    of streams 1 and 2 are not empty."""
    return (2 * cycles) // 3


def short(cycle, B):
    """The cycle for streams 0 .. B - 1 only."""
    return dict(frames=cycle["frames"][:B], poses=cycle["poses"][:B], stamps=cycle["stamps"][:B], planes=cycle["planes"][:B])


# ---- the host chain ----
class HostChain:
    """The restatements in the order the engine documents; `detect(frames) -> (dets [B, rows], n [B], bboxes or None)`."""

    def __init__(self, pp, detect):
        self.pp, self.detect = pp, detect
        self.maps = [pp.occupancy.OccupancyMap(OCC) for _ in range(STREAMS)]
        self.acc = pp.sweeps.SweepAccumulator(SWEEPS, STREAMS, F, NMAX)
        self.tracker = pp.tracking.Tracker(pp.tracking.TrackConfig(**TRACK), STREAMS)
        self.last = np.full(STREAMS, np.nan)
        self.cm = pp.costmap.CostmapConfig.from_any(COSTMAP)
        self.ic = pp.inflation.InflationConfig(**INFL_COSTMAP)
        self.io = pp.inflation.InflationConfig(**INFL_OCC)

    def reset(self, stream):
        """What sweeps_reset, occupancy_reset and track_reset of one stream do together."""
        self.maps[stream].reset()
        self.acc.reset(stream)
        self.tracker.reset(stream)
        self.last[stream] = np.nan

    def step(self, cycle):
        pp, B = self.pp, len(cycle["frames"])
        out = {}
        # 1. the occupancy maps, from the frames as they arrive
        info = [self.maps[b].update(cycle["frames"][b], cycle["poses"][b]) for b in range(B)]
        out["occ_grid"] = np.stack([self.maps[b].grid() for b in range(B)])
        out["occ_logodds"] = np.stack([self.maps[b].logodds() for b in range(B)])
        out["occ_origin"] = np.array([self.maps[b].origin for b in range(B)], np.float64)
        out["occ_info"] = {k: np.array([w[k] for w in info], np.int32) for k in OCC_INFO}
        # 2. the crop, 3. the sweeps
        out["cropped"] = [pp.frustum.crop_np(cycle["frames"][b], cycle["planes"][b]) for b in range(B)]
        out["kept"] = np.array([len(c) for c in out["cropped"]], np.int32)
        out["accumulated"], out["sweeps_info"] = self.acc.accumulate(out["cropped"], cycle["poses"], cycle["stamps"])
        # 4. the pass, 5. its tracking step
        dets, n, bboxes = self.detect(out["accumulated"])
        out["dets"], out["n"], out["bboxes"] = dets[:B].copy(), np.asarray(n[:B], np.int32).copy(), bboxes
        dt, new_last = pp.tracking.stamps_to_dt(self.last[:B], cycle["stamps"], B, self.tracker.cfg.period)
        self.last[:B] = new_last
        out["dt"] = dt
        out["tracks"] = self.tracker.step(out["dets"], out["n"], dt, poses=cycle["poses"])
        out["tracks_fixed"] = self.tracker.tracks_fixed(B)
        out["track_info"] = self.tracker.info()
        # 6. the costmap of the accumulated frames and the tracks
        tr, nt, _ = out["tracks"]
        C = pp.costmap
        grids, counts, und, fps = [], [], [], []
        for b in range(B):
            g, k = C.costmap_np(out["accumulated"][b], self.cm, tracks=tr[b], n_tracks=int(nt[b]))
            fp = C.footprints_np(self.cm, tracks=tr[b], n_tracks=int(nt[b]))
            grids.append(g)
            counts.append(k)
            fps.append(len(fp))
            und.append(C.decision_margins(self.cm, fp) < MARGIN)
        out["cm_grid"], out["cm_counts"], out["cm_undecided"] = np.stack(grids), np.stack(counts), np.stack(und)
        a = out["accumulated"]
        with np.errstate(invalid="ignore"):
            ing = [int((((f[:, 0].astype(np.float64) - GRID["x_min"]) / GRID["resolution"] >= 0)
                        & (np.floor((f[:, 0].astype(np.float64) - GRID["x_min"]) / GRID["resolution"]) < GRID["width"])
                        & ((f[:, 1].astype(np.float64) - GRID["y_min"]) / GRID["resolution"] >= 0)
                        & (np.floor((f[:, 1].astype(np.float64) - GRID["y_min"]) / GRID["resolution"]) < GRID["height"])).sum())
                   for f in a]
        out["cm_info"] = {"points_in_grid": np.array(ing, np.int32), "footprints": np.array(fps, np.int32)}
        # 7. both inflations
        out["infl_cm"] = inflate_all(pp, out["cm_grid"], self.ic)
        out["infl_occ"] = inflate_all(pp, out["occ_grid"], self.io)
        return out


def inflate_all(pp, grids, cfg):
    """inflate_np per grid -> (grids, dist2, {"lethal", "raised"} int32 [B])."""
    res = [pp.inflation.inflate_np(g, cfg, clearance=True, info=True) for g in grids]
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]),
            {k: np.array([r[2][k] for r in res], np.int32) for k in ("lethal", "raised")})


def host_chain(seq, detect, pp=None):
    """Per cycle, everything the GPU is to produce."""
    if pp is None:
        import pp_amd as pp
    chain = HostChain(pp, detect)
    return [chain.step(c) for c in seq]


def oracle_detector(pp):
    """detect() for the host test: the CPU oracle's pass (tests/util_ref.oracle_detect) as Engine.detections() rows."""
    import util_ref
    from pp_amd.engine import DET_DTYPE
    d = pp.config.Derived(config(pp))
    w = weights(pp, d)
    rect, trv, p2 = pp.synth.default_calib()
    rows = d.nms_dict()["nms_post_max_size"]

    def detect(frames):
        ref = util_ref.oracle_detect(d, w, [np.ascontiguousarray(f) for f in frames], rect, trv, p2)
        dets, n = np.zeros((len(frames), rows), DET_DTYPE), np.zeros(len(frames), np.int32)
        for b, r in enumerate(ref["dets"]):
            k = 0 if r["scores"] is None else len(r["scores"])
            n[b] = k
            if k:
                dets["box3d_lidar"][b, :k] = r["box3d_lidar"]
                dets["box3d_camera"][b, :k] = r["box3d_camera"]
                dets["score"][b, :k] = r["scores"]
                dets["label"][b, :k] = r["label_preds"]
        return dets, n, None
    return detect


# ---- the comparison ----
def dets_bytes(dets, n):
    return [dets[b, :n[b]].tobytes() for b in range(len(n))]


def same_tracks(got, want, what):
    (gt, gn, go), (wt, wn, wo) = got, want
    assert np.array_equal(gn, wn), (what, gn, wn)
    assert np.array_equal(go, wo), (what, go, wo)
    for f in TRACK_FIELDS:
        assert np.array_equal(gt[f], wt[f]), (what, f)
    assert gt.tobytes() == wt.tobytes(), what


def same_as_chain(got, want, what, streams=None):
    """Everything a run fetched (the keys of `got`) against the chain's cycle `want`.  streams: the streams to hold (all)."""
    ss = list(range(len(want["n"]))) if streams is None else list(streams)
    if "kept" in got:
        assert np.array_equal(got["kept"][ss], want["kept"][ss]), (what, "kept", got["kept"], want["kept"])
    if "sweeps_info" in got:
        for k in SWEEP_INFO:
            assert np.array_equal(got["sweeps_info"][k][ss], want["sweeps_info"][k][ss]), (what, "sweeps_info", k)
    for key in ("cropped", "accumulated"):
        if key in got:
            for b in ss:
                assert got[key][b].shape == want[key][b].shape and got[key][b].tobytes() == want[key][b].tobytes(), (what, key, b)
    if "dets" in got:
        assert np.array_equal(got["n"][ss], want["n"][ss]), (what, "n", got["n"], want["n"])
        g, w = dets_bytes(got["dets"], got["n"]), dets_bytes(want["dets"], want["n"])
        assert [g[b] for b in ss] == [w[b] for b in ss], (what, "detections")
    if "bboxes" in got and want["bboxes"] is not None:
        assert np.array_equal(got["bboxes"][ss], want["bboxes"][ss]), (what, "bboxes")
    if "tracks" in got:
        pick = lambda t: tuple(a[ss] for a in t)
        same_tracks(pick(got["tracks"]), pick(want["tracks"]), (what, "tracks"))
        (ft, fn), (rt, rn) = pick(got["tracks_fixed"]), pick(want["tracks_fixed"])
        same_tracks((ft, fn, fn), (rt, rn, rn), (what, "fixed tracks"))
        for k in ("live", "next_id", "overflow"):
            assert np.array_equal(got["track_info"][k][ss], want["track_info"][k][ss]), (what, "track_info", k)
    und = want["cm_undecided"]
    if "cm_grid" in got:
        assert int(und.sum()) <= UNDECIDED_CAP * und.size, (what, "undecided cells", int(und.sum()))
        assert np.array_equal(got["cm_counts"][ss], want["cm_counts"][ss]), (what, "costmap counts")
        for b in ss:
            assert np.array_equal(got["cm_grid"][b][~und[b]], want["cm_grid"][b][~und[b]]), (what, "costmap", b)
        for k in ("points_in_grid", "footprints"):
            assert np.array_equal(got["cm_info"][k][ss], want["cm_info"][k][ss]), (what, "costmap_info", k)
    if "occ_grid" in got:
        for k in ("occ_logodds", "occ_grid", "occ_origin"):
            assert np.array_equal(got[k][ss], want[k][ss]), (what, k)
        for k in OCC_INFO:
            assert np.array_equal(got["occ_info"][k][ss], want["occ_info"][k][ss]), (what, "occupancy_info", k)
    for key in ("infl_cm", "infl_occ"):
        if key in got:
            for b in ss:
                if key == "infl_cm" and und[b].any():
                    continue                          # (held to inflate_np of the run's own grid instead: same_inflation)
                assert np.array_equal(got[key][1][b], want[key][1][b]), (what, key, "dist2", b)
                assert np.array_equal(got[key][0][b], want[key][0][b]), (what, key, b)
                for k in ("lethal", "raised"):
                    assert got[key][2][k][b] == want[key][2][k][b], (what, key, k, b)


def same_inflation(pp, got, what):
    """Both inflated grids of a run against inflate_np of that run's own source grids."""
    for key, src, cfg in (("infl_cm", "cm_grid", INFL_COSTMAP), ("infl_occ", "occ_grid", INFL_OCC)):
        if key not in got:
            continue
        grid, d2, info = got[key]
        assert grid.dtype == np.int8 and d2.dtype == np.uint16
        wg, wd2, winfo = inflate_all(pp, got[src], pp.inflation.InflationConfig(**cfg))
        assert np.array_equal(d2, wd2), (what, key, "dist2")
        assert np.array_equal(grid, wg), (what, key)
        for k in ("lethal", "raised"):
            assert np.array_equal(info[k], winfo[k]), (what, key, k)


def _blobs(out):
    """The bytes of everything a run fetched, in a fixed order."""
    parts = []
    for key in sorted(out):
        v = out[key]
        if key == "dets":
            parts += dets_bytes(out["dets"], out["n"])
        elif isinstance(v, dict):
            parts += [np.ascontiguousarray(v[k]).tobytes() for k in sorted(v)]
        elif isinstance(v, (tuple, list)):
            for a in v:
                parts += [np.ascontiguousarray(a[k]).tobytes() for k in sorted(a)] if isinstance(a, dict) else [np.ascontiguousarray(a).tobytes()]
        else:
            parts.append(np.ascontiguousarray(v).tobytes())
    return parts


def digest(out):
    h = hashlib.sha256()
    for p in _blobs(out):
        h.update(len(p).to_bytes(8, "little"))
        h.update(p)
    return h.hexdigest()


def same_bytes(got, want, what):
    """Two runs' fetched outputs, byte for byte (the keys both hold)."""
    for key in sorted(set(got) & set(want)):
        a, b = _blobs({key: got[key], "n": got["n"]}), _blobs({key: want[key], "n": want["n"]})
        assert a == b, (what, key)


# ---- driving an Engine (GPU) ----
def configure(pp, eng):
    """Every stage of the cycle on one handle."""
    eng.load_weights(weights(pp, eng.d))
    eng.set_projection(calib(pp)[2])
    eng.set_sweeps(SWEEPS)
    eng.set_tracking(pp.tracking.TrackConfig(**TRACK))
    eng.set_track_ego(True)
    eng.set_costmap(COSTMAP)
    eng.set_occupancy(OCC)
    eng.set_inflation(INFL_COSTMAP, "costmap")
    eng.set_inflation(INFL_OCC, "occupancy")
    rect, trv, _ = calib(pp)
    eng.set_calib(rect, trv, STREAMS)


def engine(pp):
    eng = pp.Engine(config(pp), max_batch=STREAMS, max_points_per_frame=NMAX)
    configure(pp, eng)
    return eng


def plain_engine(pp):
    """The callback's engine: no stage but the same projection, fed synchronously."""
    eng = pp.Engine(config(pp), max_batch=STREAMS, max_points_per_frame=NMAX)
    eng.load_weights(weights(pp, eng.d))
    eng.set_projection(calib(pp)[2])
    return eng


def plain_detector(pp, plain):
    rect, trv, _ = calib(pp)

    def detect(frames):
        B = len(frames)
        dets, n = plain.detect([np.ascontiguousarray(f) for f in frames], rect[:B], trv[:B])
        return dets[:B].copy(), n[:B].copy(), plain.bboxes(B).copy()
    return detect


def reset_all(eng):
    eng.sync()
    eng.sweeps_reset()
    eng.occupancy_reset()
    eng.track_reset()


def reset_stream(eng, stream):
    eng.sweeps_reset(stream)
    eng.occupancy_reset(stream)
    eng.track_reset(stream)


class Dt:
    """The tracker's dt of a run from the cycles' stamps, as HostChain works it out."""

    def __init__(self, pp, eng):
        self.pp, self.last, self.period = pp, np.full(STREAMS, np.nan), eng.tracking.period

    def __call__(self, stamps):
        B = len(stamps)
        dt, self.last[:B] = self.pp.tracking.stamps_to_dt(self.last[:B], stamps, B, self.period)
        return dt

    def reset(self, stream):
        self.last[stream] = np.nan


# THE CALL ORDER OF ONE CYCLE: INTEGRATION.md, "One navigation cycle", lists these nine steps, and
# tests/test_nav_cycle_host.py holds both that listing and run_queued's own calls to this tuple
CYCLE_CALLS = ("upload_async", "occupancy_update_async", "crop_to_image_async", "accumulate_sweeps_async", "set_track_dt",
               "set_track_pose", "detect_async", "costmap_async", 'inflate_async("costmap")', 'inflate_async("occupancy")')


def queue_stages(eng, cycle, dt):
    """Steps 2 .. 9 behind a feed, nothing waited for."""
    eng.occupancy_update_async(cycle["poses"])                      # 2. before crop and sweeps: the frames as they arrived
    eng.crop_to_image_async(cycle["planes"])                        # 3.
    queue_behind_crop(eng, cycle, dt)


def queue_behind_crop(eng, cycle, dt):
    eng.accumulate_sweeps_async(cycle["poses"], cycle["stamps"])    # 4.
    eng.set_track_dt(dt)                                            # 5.
    eng.set_track_pose(cycle["poses"])
    eng.detect_async()                                              # 6.
    eng.costmap_async()                                             # 7.
    eng.inflate_async("costmap")                                    # 8.
    eng.inflate_async("occupancy")                                  # 9.


def fetch_pass(eng, B):
    """What step 6 leaves."""
    out = {}
    dets, n = eng.detections()
    out["dets"], out["n"] = dets[:B].copy(), n[:B].copy()
    out["bboxes"] = eng.bboxes(B).copy()
    out["tracks"] = eng.tracks(B)
    out["tracks_fixed"] = eng.tracks_fixed(B)
    out["track_info"] = eng.track_info()
    return out


def fetch_costmap(eng):
    out = {}
    out["cm_grid"], out["cm_counts"] = eng.costmaps(counts=True)
    out["cm_info"] = eng.costmap_info()
    return out


def fetch_occupancy(eng):
    out = {}
    out["occ_grid"], out["occ_origin"], out["occ_logodds"] = eng.occupancy_maps(logodds=True)
    out["occ_info"] = eng.occupancy_info()
    return out


def fetch_inflated(eng):
    return {"infl_cm": eng._inflated(0, None, True) + (eng.inflation_info("costmap"),),
            "infl_occ": eng._inflated(1, None, True) + (eng.inflation_info("occupancy"),)}


def fetch_all(eng, B, crop=True):
    out = {"sweeps_info": eng.sweeps_info()}
    if crop:
        out["kept"] = eng.crop_info()
    out.update(fetch_pass(eng, B))
    out.update(fetch_costmap(eng))
    out.update(fetch_occupancy(eng))
    out.update(fetch_inflated(eng))
    return out


def run_queued(pp, eng, seq):
    """Every cycle fed by upload_async of a staging and queued with no host wait; fetched at the end of the cycle."""
    reset_all(eng)
    dts, outs, stagings = Dt(pp, eng), [], []
    for cycle in seq:
        st = eng.staging(cycle["frames"])
        stagings.append(st)
        eng.upload_async(st)                                        # 1.
        queue_stages(eng, cycle, dts(cycle["stamps"]))
        outs.append(fetch_all(eng, len(cycle["frames"])))
    eng.sync()
    for st in stagings:
        st.close()
    return outs


def child_main():
    """The queued run of the whole sequence in this process; one digest per cycle on stdout."""
    import json
    import pp_amd as pp
    eng = engine(pp)
    try:
        outs = run_queued(pp, eng, sequence(pp))
    finally:
        eng.close()
    found = int(sum(o["n"].sum() for o in outs))
    print("NAV_CYCLE_DIGESTS " + json.dumps({"digests": [digest(o) for o in outs], "detections": found,
                                             "no_graph": os.environ.get("PP_NO_GRAPH", "")}))


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    child_main()
