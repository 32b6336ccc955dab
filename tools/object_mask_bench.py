"""Times of the per-point object mask on the GPU.  Reads nothing outside the repository.

    python tools/object_mask_bench.py [--runs 50] [--blocks 5]

On tools/costmap_bench.py's scene -- a 640 x 480 depth frame (synth.depth_image, every 4th valid pixel kept) at batch 1,
cfg-A, tracking on -- with the mask on the streams' tracks:
  check    the stage is first held to the restatement at that shape (rows within 1e-9 m of an edge left out, and counted)
  kernels  k_objmask_table and k_objmask_rows from Engine.kernel_times() (a device event pair around each launch), the rows
           kernel against the time the bytes it must touch take at the device's copy rate
  wall     from the end of ingest (synced) to the info words in host memory: object_mask_async() + object_mask()
  readers  k_occ_endpoints, k_scan_cells and k_costmap_points with the mask named in `consumers` and without
Prints one JSON line per row.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pp_amd as pp  # noqa: E402

GRID = dict(x_min=0.0, y_min=-5.0, resolution=0.05, width=200, height=200, z_min=-0.8, z_max=1.0, objects="tracks",
            horizon_steps=4, horizon_dt=0.25)
OCC = dict(resolution=0.05, z_min=-0.8, z_max=1.0, max_range=12.0, width=400, height=400)
SCAN = dict(nx=4, ny=4, nt=4, xy_step=1024, theta_step=8, min_cells=50, min_mean=0)
MASK = dict(objects="tracks", pad=0.05)
READERS = {"occupancy": "k_occ_endpoints", "scan_match": "k_scan_cells", "costmap": "k_costmap_points"}


def stats(us):
    return {"median_us": round(float(np.median(us)), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}


def p50_blocks(fn, runs, blocks):
    p = [float(np.median([fn() for _ in range(runs)])) for _ in range(blocks)]
    return {"p50_us": round(float(np.median(p)), 1), "p50_min_us": round(min(p), 1), "p50_max_us": round(max(p), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    om = pp.object_mask
    B = 1
    rect, trv, _ = pp.synth.default_calib()
    eng = pp.Engine(pp.config.pedestrian_d435i_config(B), max_batch=B, max_points_per_frame=pp.ingest.depth_kept_bound(640, 480))
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    eng.set_tracking(pp.tracking.TrackConfig(birth_score=0.0))
    eng.set_costmap(GRID)
    eng.set_occupancy(OCC)
    eng.set_scan_match(SCAN)
    imgs, intr = zip(*[pp.synth.depth_image(i) for i in range(B)])
    imgs, intr = list(imgs), list(intr)
    eng.set_calib(np.stack([rect] * B), np.stack([trv] * B), B)
    pose = np.stack([pp.sweeps.pose_from_xyyaw(0.0, 0.0, 0.0)] * B)
    for _ in range(3):
        pts = eng.ingest_depth(imgs, intr, return_points=True)
        eng.detect_async()
        eng.sync()
    tr, nt, _ = eng.tracks()
    n_pts = int(sum(len(p) for p in pts))
    base = {"batch": B, "points": n_pts, "tracks": nt.tolist(), "runs": a.runs, "blocks": a.blocks}

    # ---- the stage against the restatement at this shape ----
    eng.set_object_mask(dict(MASK, consumers=()))
    eng.object_mask_async()
    masks, info = eng.object_mask()
    left_out = 0
    for b in range(B):
        fp = om.footprints_np(MASK, tracks=tr[b], n_tracks=nt[b])
        und = om.point_margins_np(pts[b], fp) < om.MARGIN
        want = om.object_mask_np(pts[b], fp)
        assert np.array_equal(masks[b][~und], want[~und]), b
        assert info["footprints"][b] == len(fp) and info["rows"][b] == len(pts[b])
        left_out += int(und.sum())
    print(json.dumps({"what": "check: the stage equals the restatement", **base, "undecided_rows": left_out,
                      "masked_rows": info["masked"].tolist(), "footprints": info["footprints"].tolist()}), flush=True)

    # ---- the two kernels ----
    eng.set_profiling(True)
    per = {}
    for _ in range(a.runs):
        eng.object_mask_async()
        eng.sync()
        for tag, ms in eng.kernel_times():
            per.setdefault(tag, []).append(1e3 * ms)
    eng.set_profiling(False)
    rate = eng.device_copy_GBps()
    nbytes = {"k_objmask_table": B * 64 * (136 + 64), "k_objmask_rows": n_pts * eng.d.num_point_features * 4 + (n_pts + 7) // 8}
    for tag, us in per.items():
        print(json.dumps({"what": tag, "batch": B, **stats(us), "bytes": nbytes.get(tag), "copy_rate_GBps": round(rate, 1),
                          "copy_rate_us": round(nbytes.get(tag, 0) / (rate * 1e3), 3)}), flush=True)

    # ---- end of ingest -> the info words on the host ----
    def wall():
        eng.ingest_depth(imgs, intr)
        eng.sync()
        t0 = time.perf_counter()
        eng.object_mask_async()
        eng.object_mask()
        return 1e6 * (time.perf_counter() - t0)

    print(json.dumps({"what": "wall: end of ingest -> bits and info words on the host", **base, **p50_blocks(wall, a.runs, a.blocks)}), flush=True)

    # ---- the three readers' kernels with the mask and without ----
    calls = {"occupancy": lambda: eng.occupancy_update_async(pose), "scan_match": lambda: eng.scan_match_async(pose),
             "costmap": lambda: eng.costmap_async()}
    eng.ingest_depth(imgs, intr)
    eng.occupancy_update_async(pose)          # a map for the scan match
    for masked in (False, True, False, True):
        eng.set_object_mask(dict(MASK, consumers=tuple(READERS) if masked else ()))
        eng.object_mask_async()
        eng.set_profiling(True)
        per = {}
        for _ in range(a.runs):
            for name, call in calls.items():
                call()
                eng.sync()
                for tag, ms in eng.kernel_times():
                    if tag == READERS[name]:
                        per.setdefault(tag, []).append(1e3 * ms)
        eng.set_profiling(False)
        for tag, us in per.items():
            print(json.dumps({"what": tag, "masked": masked, "batch": B, **stats(us)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
