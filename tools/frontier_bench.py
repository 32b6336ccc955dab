"""Times of the frontier stage on the GPU.  Reads nothing outside the repository.

    python tools/frontier_bench.py [--runs 50] [--blocks 5] [--updates 12]

Two scenes on a 400 x 400 window of 0.1 m cells at batch 1:
  room        the rolling occupancy map of tools/occupancy_bench.py's scene (one 640 x 480 depth frame per update, the
              pose moving 5 cm and turning 0.01 rad per frame) after --updates updates, behind the default inflation
  serpentine  a one-cell free corridor through unknown space, every second row of the window, painted through the costmap's
              point layer (a point above z_max per free cell): ONE cluster that crosses every tile, the worst case of the
              merge phase
Measured from the end of the inflation (synced):
  gpu      wall time to the ranked goals in host memory: Engine.frontier_async + frontiers() -- with use_field,
           navfn_async from the sensor's cell in front.  p50 of --runs, repeated --blocks times: the median of the blocks'
           p50 with their min - max.
  host     the route the stage replaces, on the same commit: the inflated grid fetched (and the field, under use_field),
           then scipy.ndimage.label and numpy statistics -- a restatement with scipy's C labelling underneath, not a
           tuned CPU pipeline.
  kernels  the five kernels from Engine.kernel_times() (a device event pair around each launch), median of --runs.
Every scene's result is first held to frontier.frontier_np.  Prints one JSON line per row.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pp_amd as pp  # noqa: E402

W = H = 400
OCC = dict(resolution=0.1, width=W, height=H, z_min=-0.8, z_max=1.0, max_range=20.0)
COSTMAP = dict(x_min=-20.0, y_min=-20.0, resolution=0.1, width=W, height=H, z_min=-0.8, z_max=1.0)
KERNELS = ("k_frontier_mark", "k_frontier_label", "k_frontier_stats", "k_frontier_rep", "k_frontier_select")


def p50_blocks(fn, runs, blocks):
    p = []
    for _ in range(blocks):
        p.append(float(np.median([fn() for _ in range(runs)])))
    return {"p50_us": round(float(np.median(p)), 1), "p50_min_us": round(min(p), 1), "p50_max_us": round(max(p), 1)}


def serpentine_points():
    """A point above z_max at the centre of every free cell of the serpentine: float32 [n, 3] in the costmap's frame."""
    g = np.full((H, W), -1, np.int8)
    rows = list(range(1, H - 1, 2))
    for k, y in enumerate(rows):
        g[y, 1:W - 1] = 0
        if k + 1 < len(rows):
            g[y + 1, W - 2 if k % 2 == 0 else 1] = 0
    ys, xs = np.nonzero(g == 0)
    pts = np.stack([COSTMAP["x_min"] + (xs + 0.5) * 0.1, COSTMAP["y_min"] + (ys + 0.5) * 0.1, np.full(len(xs), 2.0)], axis=1)
    return pts.astype(np.float32), g


def host_frontiers(grid, cfg, ref, pot):
    """frontier.py's rule with scipy's labelling and numpy statistics: the words of the returned frontiers."""
    F = pp.frontier
    front = F.frontier_cells_np(grid, cfg)
    structure = np.ones((3, 3), int) if cfg.connectivity == 8 else None
    comp, n = ndimage.label(front, structure=structure)
    if n == 0:
        return np.zeros((0, 8), np.int64)
    ys, xs = np.nonzero(front)
    k = comp[ys, xs] - 1
    idx = ys * grid.shape[1] + xs
    cnt = np.bincount(k, minlength=n)
    sx, sy = np.bincount(k, xs, n).astype(np.int64), np.bincount(k, ys, n).astype(np.int64)
    cx, cy = (2 * sx + cnt) // (2 * cnt), (2 * sy + cnt) // (2 * cnt)
    label = np.full(n, 1 << 62, np.int64)
    np.minimum.at(label, k, idx)
    key = (((xs - cx[k]) ** 2 + (ys - cy[k]) ** 2).astype(np.int64) << 20) | idx
    rep = np.full(n, 1 << 62, np.int64)
    np.minimum.at(rep, k, key)
    rx, ry = (rep & 0xFFFFF) % grid.shape[1], (rep & 0xFFFFF) // grid.shape[1]
    D = pot[ry, rx].astype(np.int64) if cfg.use_field else (rx - ref[0]) ** 2 + (ry - ref[1]) ** 2
    keep = cnt >= cfg.min_size
    if cfg.use_field:
        keep &= D != F.UNREACHED
    order = ((D if cfg.rank == 0 else (1 << 20) - cnt) << 20) | label
    sel = np.nonzero(keep)[0]
    sel = sel[np.argsort(order[sel])][:cfg.max_frontiers]
    return np.stack([rx[sel], ry[sel], cx[sel], cy[sel], cnt[sel], label[sel], D[sel] & 0xFFFFFFFF, D[sel] >> 32], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--updates", type=int, default=12)
    a = ap.parse_args()
    F = pp.frontier
    spts, _ = serpentine_points()
    cap = max(pp.ingest.depth_kept_bound(640, 480), len(spts))
    eng = pp.Engine(pp.config.pedestrian_d435i_config(1), max_batch=1, max_points_per_frame=cap)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    eng.set_occupancy(OCC)
    eng.set_costmap(COSTMAP)
    for source in ("occupancy", "costmap"):
        eng.set_inflation(True, source)
        eng.set_navfn(True, source)
    img, intr = pp.synth.depth_image(0)
    for step in range(1, a.updates + 1):
        eng.ingest_depth([img], [intr])
        eng.occupancy_update_async(pp.sweeps.pose_from_xyyaw(0.05 * step, -0.02 * step, 0.01 * step)[None])
    eng.sync()
    sensor = np.array([[W // 2, H // 2]], np.int32)

    def inflated(source):
        """The inflation of the scene's grids, finished."""
        if source == "costmap":
            eng.costmap_async()
        eng.inflate_async(source)
        eng._costmap_queued = False
        eng.sync()

    for scene, source in (("room", "occupancy"), ("serpentine", "costmap")):
        k = 1 if source == "occupancy" else 0
        if scene == "serpentine":
            eng.upload([spts])
        for use_field in (0, 1):
            if scene == "serpentine" and use_field:
                continue                                 # (unknown cells are blocked: the corridor is one long field, navfn's own worst case)
            eng.set_frontier(dict(use_field=use_field), source)
            cfg = eng.frontier_config(source)

            def run():
                if use_field:
                    eng._navfn_cells_async(k, sensor, None)
                eng.frontier_async(source, refs=sensor)
                return eng.frontiers(source)

            inflated(source)
            fr, info = run()
            grid = eng._inflated(k, None, False)[0][0]
            pot = eng.navfn_fields(source)[0] if use_field else None
            _, ww, wi = F.frontier_np(grid, cfg, sensor[0], pot)
            assert [int(info[n][0]) for n in F.INFO] == wi.tolist(), "the stage does not equal frontier_np"
            assert fr[0]["label"].tolist() == ww[:, 5].tolist() and fr[0]["cost"].tolist() == F.cost_of(ww)
            assert np.array_equal(host_frontiers(grid, cfg, sensor[0], pot), ww.view(np.uint32).astype(np.int64)), "the host route does not equal frontier_np"

            def gpu():
                inflated(source)
                t0 = time.perf_counter()
                run()
                return 1e6 * (time.perf_counter() - t0)

            def host():
                inflated(source)
                if use_field:
                    eng._navfn_cells_async(k, sensor, None)
                    eng.navfn_info(source)               # (the field settled: the host route is not charged for making it)
                t0 = time.perf_counter()
                g = eng._inflated(k, None, False)[0][0]
                p = eng.navfn_fields(source)[0] if use_field else None
                host_frontiers(g, cfg, sensor[0], p)
                return 1e6 * (time.perf_counter() - t0)

            base = {"scene": scene, "use_field": use_field, "window": [W, H], "info": {n: int(v[0]) for n, v in info.items()},
                    "runs": a.runs, "blocks": a.blocks}
            print(json.dumps({"what": "gpu: end of the inflation -> goals on the host", **base, **p50_blocks(gpu, a.runs, a.blocks)}), flush=True)
            print(json.dumps({"what": "host: fetch the grid" + (" and the field" if use_field else "") + " + scipy.ndimage.label + numpy",
                              **base, **p50_blocks(host, a.runs, a.blocks)}), flush=True)
            if use_field:
                continue
            # ---- the kernels, profiled in runs of their own ----
            inflated(source)
            eng.set_profiling(True)
            per = {n: [] for n in KERNELS}
            for _ in range(a.runs):
                eng.frontier_async(source, refs=sensor)
                eng.sync()
                for tag, ms in eng.kernel_times():
                    if tag in per:
                        per[tag].append(1e3 * ms)
            eng.set_profiling(False)
            print(json.dumps({"what": "kernels", **base, **{n + "_median_us": round(float(np.median(v)), 2) for n, v in per.items()}}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
