"""Grid shapes that take the shape-dependent branches of the detector's front end (voxeliser, PFN, anchor mask), of the
first backbone layer and of the costmap, shared by tests/test_grid_shape_cases_host.py (which asserts, from the constants
read out of the sources, that every case lands on the side of each launch predicate it is listed for) and
tests/test_gpu_grid_shapes.py (which runs them on the GPU against the oracle).

The branches, by the number the case table refers to:
   1  csrc/pfn.hip k_pfn_canvas2, stage (0): `lane / nz` with nz >= 3 (not a power of two: z3; a full wave of 64 slots: z8)
   2  launch_pfn_t / pfn_can_carry_anchor_mask: PFN2_CW * nz > 64 falls to k_pfn_canvas, the mask gets its own launch
   3  k_pfn_canvas2<.., PIL> with z cells: primary / z0 / the `z > zc` cell-map lookups
   4  csrc/backbone.hip, sparse block1.0 without the bitmap: the occ_nz loop over the cell map
   5  csrc/anchor_mask_dev.h, the scalar occupancy load (nz > 2 or ny * nx % 4 != 0)
   6  same, the 16-byte load whose four cells straddle two rows (nx % 4 != 0, ny * nx % 4 == 0)
   7  same, the second trip of the scan along y (ny > 64) and the third along x (nx > 128)
   8  launch_anchor_mask / pfn_can_carry_anchor_mask: ny * (nx | 1) <= AM_MAX_CELLS on both sides
   9  csrc/anchor_mask.hip k_colscan, the tail loop (ny % 8 != 0)
  10  k_anchor_lookup_bits at a second width (256 cells: 6 bitmap words a row; the KITTI-shaped grid has 8)

Every case is pedestrian_d435i_config(2) edited the way test_gpu_parity._random_config edits it: 0.08 m cells, x from 0,
y centred, z from -3.0 in nz cells of Z_CELL metres, anchor strides and offsets after the first layer stride (1 everywhere
here), one layer per block."""
import collections
import copy

import numpy as np

import pp_amd as pp

CELL = 0.08
Z_MIN, Z_CELL = -3.0, 1.0
B = 2
NMAX = 8192                      # max_points_per_frame of the engines
ROWS = (4000, 300)               # rows of the two frames, about
SIGMA = 0.12                     # of a blob, metres

NARROW = {"pfn": 32, "filters": [32, 32, 64], "up": 32}
SHIPPED = {"pfn": 128, "filters": [64, 128, 256], "up": 128}

Case = collections.namedtuple("Case", "name nx ny nz strides widths max_voxels blobs seed rows")

CASES = [
    Case("z3", 36, 28, 3, (1, 2, 2), NARROW, 2000, 5, 301, (1, 5)),
    Case("z8", 24, 16, 8, (1, 2, 2), NARROW, 2000, 3, 302, (1,)),
    Case("z9", 24, 16, 9, (1, 2, 2), NARROW, 2000, 3, 303, (2,)),
    Case("odd", 27, 21, 1, (1, 1, 1), NARROW, 2000, 4, 304, (5,)),
    Case("straddle", 26, 22, 2, (1, 1, 1), NARROW, 2000, 4, 305, (6,)),
    Case("tall", 72, 96, 2, (1, 2, 2), NARROW, 3000, 14, 306, (7,)),
    Case("wide", 136, 56, 2, (1, 2, 2), NARROW, 3000, 14, 307, (7,)),
    Case("lds-in", 127, 64, 1, (1, 1, 1), NARROW, 3000, 14, 308, (8,)),
    Case("lds-out", 128, 64, 2, (1, 2, 2), NARROW, 3000, 14, 409, (8,)),
    Case("col-tail", 100, 84, 2, (1, 2, 2), NARROW, 3000, 14, 310, (9,)),
    Case("sparse-z2", 256, 128, 2, (1, 2, 2), SHIPPED, 8192, 40, 411, (3, 4)),
    Case("sparse-z1", 256, 128, 1, (1, 2, 2), SHIPPED, 8192, 40, 312, (10,)),
]
# (seed: of the frames and of init_weights.  309 and 311 gave lds-out and sparse-z2 weights under which the oracle keeps boxes
# 61 m and 746 m long -- the exponential of a large size logit -- which the 1e-4 absolute bar of _assert_dets cannot resolve
# in float32; test_grid_shape_cases_host.py states the condition, on the oracle's values alone.)
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


def config(case):
    cfg = copy.deepcopy(pp.config.pedestrian_d435i_config(B))
    nx, ny, nz = case.nx, case.ny, case.nz
    s1, s2, s3 = case.strides
    x0, y0 = 0.0, -ny * CELL / 2
    cfg["eval_input_reader"].update(batch_size=B, feature_map_size=[1, ny // s1, nx // s1])
    s = cfg["model"]["second"]
    s["voxel_generator"].update(point_cloud_range=[x0, y0, Z_MIN, x0 + nx * CELL, y0 + ny * CELL, Z_MIN + nz * Z_CELL],
                                voxel_size=[CELL, CELL, Z_CELL], max_number_of_voxels=case.max_voxels)
    s["voxel_feature_extractor"]["num_filters"] = case.widths["pfn"]
    s["rpn"].update(layer_nums=[1, 1, 1], layer_strides=[s1, s2, s3], num_filters=list(case.widths["filters"]),
                    upsample_strides=[1, s2, s2 * s3], num_upsample_filters=[case.widths["up"]] * 3)
    s["target_assigner"]["anchor_generators"]["anchor_generator_stride"].update(
        strides=[CELL * s1, CELL * s1, 0.0], offsets=[x0 + CELL * s1, y0, -1.465])
    return cfg


def frames(case):
    """Two seeded frames: x, y around blob centres inside the range (uniform clouds turn every anchor on and test nothing
    of the mask), z uniform over the range and 0.1 m beyond both ends, and one column with a point in every z cell."""
    rng = np.random.default_rng(case.seed)
    xr, yr = case.nx * CELL, case.ny * CELL
    zr = (Z_MIN, Z_MIN + case.nz * Z_CELL)
    out = []
    for n, blobs in zip(ROWS, (case.blobs, 2)):
        n = int(n + rng.integers(0, 50))
        cx = rng.uniform(0.15 * xr, 0.85 * xr, blobs)
        cy = rng.uniform(-0.35 * yr, 0.35 * yr, blobs)
        which = rng.integers(0, blobs, n)
        xyz = np.stack([cx[which] + SIGMA * rng.standard_normal(n), cy[which] + SIGMA * rng.standard_normal(n),
                        rng.uniform(zr[0] - 0.1, zr[1] + 0.1, n)], axis=1)
        # the full column: the centre of a cell next to the first blob, a point at the middle of every z cell
        col = np.array([(np.floor(cx[0] / CELL) + 0.5) * CELL, (np.floor(cy[0] / CELL) + 0.5) * CELL])
        full = np.concatenate([np.tile(col, (case.nz, 1)), (zr[0] + (np.arange(case.nz) + 0.5) * Z_CELL)[:, None]], axis=1)
        at = int(rng.integers(0, n))
        out.append(np.concatenate([xyz[:at], full, xyz[at:]], axis=0).astype(np.float32))
    return out


_REF = {}


def reference(case):
    """(Derived, weights, frames, oracle result) of a case, computed once and shared; nobody writes into it."""
    import util_ref
    if case.name not in _REF:
        d = pp.config.Derived(config(case))
        w = pp.weights.init_weights(d, seed=case.seed)
        fr = frames(case)
        rect, trv, p2 = pp.synth.default_calib()
        _REF[case.name] = (d, w, fr, util_ref.oracle_detect(d, w, fr, rect, trv, p2))
    return _REF[case.name]


# ---- the launch predicates, restated (the constants come from the sources: test_grid_shape_cases_host.py) ----
def lds_image_fits(nx, ny, am_max_cells):
    return ny * (nx | 1) <= am_max_cells


def pfn_second_generation(nz, pfn2_cw):
    return pfn2_cw * nz <= 64


def sparse_canvas(nx, ny, max_voxels, min_cells, voxel_factor):
    return nx * ny >= min_cells and voxel_factor * max_voxels <= nx * ny


def mask_vector_load(nx, ny, nz):
    return (nx * ny) % 4 == 0 and nz <= 2


# ---- wide costmaps (branch 11: csrc/costmap.hip k_costmap_compose, a wave inside one row past column 0) ----
# More than 64 quads of four cells a row, so some waves of the compose kernel lie inside one row and cull records by their
# columns too.  w300: 75 quads a row, 11 waves, 3 of them in one row, 2 of those starting past column 0; w257: 65 quads a
# row, three padding cells, the 65th quad of row 0 in the wave that goes on into row 1.
WIDE_COSTMAPS = {
    "w300": dict(width=300, height=9, resolution=0.1, x_min=-15.0, y_min=-0.9),
    "w257": dict(width=257, height=5, resolution=0.1, x_min=-12.85, y_min=-0.9),
}
WIDE_STREAMS = 3
WIDE_ROWS = 1500                 # seeded rows per frame
WIDE_GATE = 0.4
WIDE_MOVE = (0.04, -0.03)        # the second track_update: 0.05 m on


def compose_waves(width, height, wave=64):
    """k_costmap_compose's waves that hold a cell, as (first row, last row, first column, last column): a row holds
    pitch / 4 quads, pitch = the width rounded up to a multiple of 4, and a wave takes `wave` consecutive quads (a workgroup
    is a whole number of waves).  The columns are the wave's own only when it lies in one row (else the whole row)."""
    pitch = (width + 3) & ~3
    qrow = pitch // 4
    total = qrow * height
    out = []
    for q0 in range(0, total, wave):
        q1 = min(q0 + wave, total) - 1
        r0, r1 = q0 // qrow, q1 // qrow
        out.append((r0, r1, 4 * (q0 - r0 * qrow), 4 * (q1 - r1 * qrow) + 3) if r0 == r1 else (r0, r1, 0, pitch - 1))
    return out


def wide_costmap_config(name, steps, z_range=(-1.0, 1.0)):
    return dict(WIDE_COSTMAPS[name], z_min=z_range[0], z_max=z_range[1], objects="tracks", horizon_steps=steps, horizon_dt=0.5,
                object_cost=100, predict_cost=[70, 60][:max(steps, 1)])


def wide_track_rows(name, stream):
    """24 rows (x, y, w, l, yaw, score) of a stream: 18 centres evenly along x, two on the columns where the first wave of a
    row ends (cells 255 / 256), one inside the first wave's columns only, one across each of the left and right edges of
    the grid, one anywhere; y uniform in +-0.8 (drawn again while two centres lie within gate + 0.1 m of each other: every
    row must open, and keep, a track of its own), sizes 0.3 - 1.2 m, any yaw."""
    g = WIDE_COSTMAPS[name]
    rng = np.random.default_rng(700 + 10 * stream + len(name) + g["width"])
    x0, res = g["x_min"], g["resolution"]
    x1 = x0 + g["width"] * res
    xs = list(np.linspace(x0 + 0.8, x1 - 0.8, 18))
    xs += [x0 + 255.5 * res, x0 + 256.5 * res, x0 + 100.5 * res, x0 + 0.05, x1 - 0.05, float(rng.uniform(x0 + 1, x1 - 1))]
    xs = np.array(xs)
    while True:
        ys = rng.uniform(-0.8, 0.8, len(xs))
        dist = np.hypot(xs[:, None] - xs[None], ys[:, None] - ys[None]) + 10.0 * np.eye(len(xs))
        if dist.min() > WIDE_GATE + 0.1:
            break
    return [(float(x), float(y), float(rng.uniform(0.3, 1.2)), float(rng.uniform(0.3, 1.2)), float(rng.uniform(-3.1, 3.1)), 0.9)
            for x, y in zip(xs, ys)]


def wide_moved(rows):
    return [(r[0] + WIDE_MOVE[0], r[1] + WIDE_MOVE[1]) + r[2:] for r in rows]


def wide_det_rows(per_stream, rows=64):
    """per stream a list of (x, y, w, l, yaw, score) -> (dets [streams, rows] of the engine's detection dtype, n)."""
    d = np.zeros((len(per_stream), rows), pp.Engine.det_dtype())
    n = np.zeros(len(per_stream), np.int32)
    for s, rr in enumerate(per_stream):
        n[s] = len(rr)
        for i, r in enumerate(rr):
            d["box3d_lidar"][s, i] = (r[0], r[1], 0.0, r[2], r[3], 1.6, r[4])
            d["score"][s, i] = r[5]
    return d, n


def wide_frames(name):
    g = WIDE_COSTMAPS[name]
    rng = np.random.default_rng(40 + g["width"])
    x0, y0 = g["x_min"], g["y_min"]
    x1, y1 = x0 + g["width"] * g["resolution"], y0 + g["height"] * g["resolution"]
    return [rng.uniform([x0 - 0.5, y0 - 0.2, -1.5], [x1 + 0.5, y1 + 0.2, 1.5], (WIDE_ROWS + 7 * b, 3)).astype(np.float32)
            for b in range(WIDE_STREAMS)]


def wide_track_config():
    return pp.tracking.TrackConfig(gate=WIDE_GATE, birth_score=0.3, max_misses=2, min_hits=2, q_acc=4.0, r_pos=0.01)
