"""Correlative scan-to-map matching: the resident points of a frame, under the caller's PRIOR sensor-to-fixed pose, are
matched against the stream's rolling occupancy map (occupancy.py) BEFORE the frame is fused into it -- a brute-force
search over a window of translations and headings around the prior (Olson 2009, the front end of Cartographer), scored on
the map's own integer log-odds.  The answer is eight integers per stream; `corrected_pose` turns them into the pose to hand
to `occupancy_update_async` and every other fixed-frame stage.

The reference has no such path, so nothing here is parity with it.  This module STATES the rule: `scan_cells_np`,
`score_np` (one candidate, cell by cell in Python ints), `scores_np` (all candidates as numpy arrays, an independent second
statement), `best_np` and `match_np` are the restatement that the GPU (csrc/scan_match.hip behind Engine.set_scan_match /
scan_match_async / localize, and `scan_match_grids`) equals with no tolerance.  Apart from one float64 rotation per row
(+ * / and floor) and the sensor's sub-cell position (float64 on the host), everything is integer arithmetic.

UNITS, as local_planner.py: SUB = 1024 sub-cells per cell, HEADINGS = 4096 ticks per revolution, (C, S)[h] =
`local_planner.trig_table()`, 2^14 its 1.0.  Resolution, window, z_min, z_max and max_range are the OccupancyConfig's.

1 SCAN CELLS (`scan_cells_np`).  Per row, x y z widened from float32 to float64; only the prior's rotation rows are used, no
  translation: dx = ((R00 * x + R01 * y) + R02 * z), dy likewise with row 1; gx = floor(dx / resolution) + W // 2, gy =
  floor(dy / resolution) + H // 2.  The row is USED iff gx >= 0, gx < W, gy >= 0, gy < H, (x * x + y * y) <= max_range *
  max_range, z <= z_max (the occupancy rule's tests) AND z >= z_min: ground returns take no part; a NaN fails.  The others
  are IGNORED.  Every distinct (gx, gy) is ONE scan cell however many rows fall in it, represented by its centre in
  sub-cells from the sensor: ux = (gx - W // 2) * 1024 + 512, uy likewise.  n_scan is their number.

2 SENSOR.  With the map's CURRENT window origin cell (ox, oy) -- the one the stream's last update left; the match does not
  move it -- sx = floor((t_x / resolution - ox) * 1024), sy likewise, float64 on the host (`sensor_subcells`).  No map:
  status NO_MAP.  The sensor's cell (sx >> 10, sy >> 10) outside the window: status OUTSIDE.  In both cases nothing is
  scored: every score reads 0, and step 4 runs on those zeros (it picks the centre candidate).

3 CANDIDATES.  c = (it * (2 ny + 1) + iy) * (2 nx + 1) + ix, it in 0 .. 2 nt and so on.  dh = (it - nt) * theta_step,
  (C, S) = trig[dh & 4095].  Every scan cell is rotated in int64 with a rounding arithmetic shift (floor):
  rx = (C * ux - S * uy + 8192) >> 14, ry = (S * ux + C * uy + 8192) >> 14.  Its map cell: cx = (sx + (ix - nx) * xy_step +
  rx) >> 10, cy = (sy + (iy - ny) * xy_step + ry) >> 10.  score[c] = the sum over the scan cells of L[cy, cx] where (cx, cy)
  lies inside the window and the cell is known; any other cell adds 0.  L is the stream's int16 log-odds as it stands
  BEFORE this frame is fused.  Negative log-odds count: a scan cell that lands in known free space costs.  The map is NOT
  smoothed: a 3 x 3 max over the clamped log-odds flattens the peak into a plateau and loses exact recovery.
  |score| < 2^30: at most 2^20 scan cells weighed by |L| <= 1000.

4 BEST.  d = |it - nt| + |iy - ny| + |ix - nx|; key = ((2^30 - score) << 32) | (d << 16) | c as uint64; the LEAST key wins:
  the highest score, then the smallest motion, then the lowest index.  Result words int32 [8] (WORDS): status, ix - nx,
  iy - ny, it - nt, the best score, the score of the prior (the centre candidate), n_scan, rows ignored.  Status bits:
  1 NO_MAP, 2 OUTSIDE, 4 FEW_CELLS (n_scan < min_cells), 8 LOW_SCORE (best * 100 < min_mean * n_scan, in int64),
  16 EDGE (the best lies on a face of a search axis whose half-width is > 0: a wider window might do better).

5 POSE (`corrected_pose`, host float64).  status & 15 set: the prior, unchanged.  Otherwise R' = Rz(2 pi dh / 4096) R and
  t' = t + ((ix - nx), (iy - ny)) * xy_step * resolution / 1024; the third row and t_z are untouched (Rz leaves them).  The
  device never forms a pose.

The stage relies on one property of the occupancy state: L = 0 wherever a cell is not known (occupancy.py step 1 and 4: a
cell starts as L = 0, unknown, and only a hit or a pass, which make it known, change L), so the device adds L alone.  The
restatement writes the `known` test out; `scan_match_grids` zeroes L where not known before it uploads.

OBJECT MASK (object_mask.py; scan_cells_np / match_np(..., mask=)): a row whose mask bit is set takes no part in step 1
and is counted with the ignored rows, so a person close to the sensor contributes no scan cell.  Without a mask the rule
is what it was.  GROUND CLASSES (ground.py; scan_cells_np / match_np(..., ground=)): a row takes part iff its class is
OBSTACLE (and it is not object-masked), in the place of the z band.

Out of scope: multi-resolution branch and bound, sub-cell refinement, a covariance from the score volume, loop closure,
any correction of roll, pitch or z.  (No longer in that list: removing tracked objects' points from the scan, which is
the object mask above, a stage of its own in front of this one.)
"""
import ctypes
import dataclasses
import math

import numpy as np

from . import _lib
from . import occupancy as _occ
from . import sweeps as _swp
from .local_planner import HEADINGS, ONE, SUB, trig_table
from ._lib import PP_OCC_MAX_CELLS, PP_SCAN_MAX_CANDIDATES, PP_SCAN_RESULT

NO_MAP, OUTSIDE, FEW_CELLS, LOW_SCORE, EDGE = 1, 2, 4, 8, 16
REJECT = NO_MAP | OUTSIDE | FEW_CELLS | LOW_SCORE          # `corrected_pose` returns the prior under any of these
WORDS = ("status", "dx", "dy", "dt", "best", "prior", "n_scan", "ignored")
MAX_HALF = 127                          # nx, ny, nt at most
MAX_XY_STEP, MAX_THETA_STEP = 4096, 512
MAX_MIN_MEAN = 100000                   # |min_mean| at most: a mean of |L| = 1000, the log-odds clamp
SCORE_BIAS = 1 << 30                    # a key's high word is SCORE_BIAS - score
_RANGES = (("nx", 0, MAX_HALF), ("ny", 0, MAX_HALF), ("nt", 0, MAX_HALF), ("xy_step", 1, MAX_XY_STEP),
           ("theta_step", 1, MAX_THETA_STEP), ("min_cells", 0, PP_OCC_MAX_CELLS), ("min_mean", -MAX_MIN_MEAN, MAX_MIN_MEAN))
_TRIG = trig_table()
_TRIG.setflags(write=False)
assert SUB == 1 << 10 and HEADINGS == 1 << 12 and ONE == 1 << 14 and len(WORDS) == PP_SCAN_RESULT
assert PP_SCAN_MAX_CANDIDATES == 1 << 16 and 3 * MAX_HALF < 1 << 16          # c and d are 16 bits of the key each
assert PP_OCC_MAX_CELLS * 1000 < SCORE_BIAS                                   # |score| < 2^30
# sx < W * 1024, |rx| <= (W // 2 + H // 2 + 2) * 1024 and the shift stay inside int32: W * H <= 2^20
assert (PP_OCC_MAX_CELLS + PP_OCC_MAX_CELLS // 2 + 4) * SUB + MAX_HALF * MAX_XY_STEP < 2 ** 31


@dataclasses.dataclass
class ScanMatchConfig:
    """nx, ny, nt      0 .. 127: half-widths of the search window in steps; (2 nx + 1)(2 ny + 1)(2 nt + 1) <= 65536
    xy_step         1 .. 4096: sub-cells (1 / 1024 cell) per translation step
    theta_step      1 .. 512: heading ticks (1 / 4096 revolution) per rotation step
    min_cells       0 .. 1048576: fewer scan cells raise FEW_CELLS
    min_mean        -100000 .. 100000, hundredths of the map's log-odds unit (itself 0.01 nat) per scan cell: a best
                    score below min_mean * n_scan / 100 raises LOW_SCORE"""
    nx: int = 10
    ny: int = 10
    nt: int = 10
    xy_step: int = 1024
    theta_step: int = 8
    min_cells: int = 50
    min_mean: int = 0

    def __post_init__(self):
        for f, lo, hi in _RANGES:
            v = getattr(self, f)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"ScanMatchConfig: {f} must be an integer, got {v!r}")
            if int(v) < lo or int(v) > hi:
                raise ValueError(f"ScanMatchConfig: {f} = {v} outside [{lo}, {hi}]")
            setattr(self, f, int(v))
        if self.candidates > PP_SCAN_MAX_CANDIDATES:
            raise ValueError(f"ScanMatchConfig: (2 nx + 1)(2 ny + 1)(2 nt + 1) = {self.candidates} candidates, at most "
                             f"PP_SCAN_MAX_CANDIDATES = {PP_SCAN_MAX_CANDIDATES}")

    @property
    def candidates(self):
        return (2 * self.nx + 1) * (2 * self.ny + 1) * (2 * self.nt + 1)

    def to_dict(self):
        return dataclasses.asdict(self)

    @classmethod
    def from_any(cls, cfg):
        """A ScanMatchConfig, a dict of its fields (unknown keys raise, naming them) or True (the defaults)."""
        if isinstance(cfg, cls):
            return cfg
        if cfg is True:
            return cls()
        if isinstance(cfg, dict):
            unknown = set(cfg) - {f.name for f in dataclasses.fields(cls)}
            if unknown:
                raise ValueError(f"scan_match: unknown keys {sorted(unknown)}")
            return cls(**cfg)
        raise ValueError(f"scan_match: a ScanMatchConfig, a dict of its fields or True, got {cfg!r}")


def scan_cells_np(occ_cfg, points, pose, mask=None, ground=None):
    """Step 1 for one frame: (cells int64 [n_scan, 2] = (ux, uy) in ascending (gy, gx), (rows used, rows ignored,
    n_scan)) of rows float32 [n, F >= 3] under the rotation of pose [3, 4].  mask: bool [n], the rows' object mask
    (object_mask.py) -- a masked row takes no part and is counted with the ignored rows.  ground: the pair (ground bool [n],
    obstacle bool [n]) of the rows' classes (ground.py) -- OBSTACLE stands in the place of the z band."""
    c = _occ.OccupancyConfig.from_any(occ_cfg)
    p, P = np.asarray(points), np.asarray(pose, np.float64)
    if p.dtype != np.float32 or p.ndim != 2 or p.shape[1] < 3:
        raise ValueError(f"scan_match: points must be float32 [n, F >= 3], got {p.dtype} {p.shape}")
    W, H = c.width, c.height
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        dx = (P[0, 0] * x + P[0, 1] * y) + P[0, 2] * z
        dy = (P[1, 0] * x + P[1, 1] * y) + P[1, 2] * z
        gx = np.floor(dx / c.resolution) + float(W // 2)
        gy = np.floor(dy / c.resolution) + float(H // 2)
        if ground is None:
            band = (z <= c.z_max) & (z >= c.z_min)
        else:
            from . import ground as _gr
            band = _gr.check_classes(ground, len(p), "scan_match")[1]
        used = (gx >= 0) & (gx < W) & (gy >= 0) & (gy < H) & ((x * x + y * y) <= c.max_range * c.max_range) & band
    if mask is not None:
        m = np.asarray(mask, bool).reshape(-1)
        if m.shape != (len(p),):
            raise ValueError(f"scan_match: mask must be bool [{len(p)}], got {m.shape}")
        used = used & ~m
    flat = np.unique(gy[used].astype(np.int64) * W + gx[used].astype(np.int64))
    cells = np.stack([(flat % W - W // 2) * SUB + SUB // 2, (flat // W - H // 2) * SUB + SUB // 2], axis=1)
    return cells.astype(np.int64), (int(used.sum()), int(len(p) - used.sum()), int(len(flat)))


def sensor_subcells(occ_cfg, pose, origin_cell):
    """Step 2: (sx, sy), the sensor's position in sub-cells of the window whose origin cell is `origin_cell`."""
    c = _occ.OccupancyConfig.from_any(occ_cfg)
    P = np.asarray(pose, np.float64)
    return tuple(int(math.floor((float(P[k, 3]) / c.resolution - float(origin_cell[k])) * float(SUB))) for k in range(2))


def _delta(cfg, c):
    """(ix - nx, iy - ny, it - nt) of candidate index c."""
    wx, wy = 2 * cfg.nx + 1, 2 * cfg.ny + 1
    return c % wx - cfg.nx, (c // wx) % wy - cfg.ny, c // (wx * wy) - cfg.nt


def score_np(L, known, cells, sensor, cfg, c):
    """Step 3 for candidate c, cell by cell in Python ints: L int16 [H, W], known bool [H, W], cells [n, 2] (ux, uy),
    sensor (sx, sy)."""
    cfg = ScanMatchConfig.from_any(cfg)
    H, W = L.shape
    ddx, ddy, ddt = _delta(cfg, int(c))
    C, S = (int(v) for v in _TRIG[(ddt * cfg.theta_step) & (HEADINGS - 1)])
    total = 0
    for ux, uy in np.asarray(cells, np.int64).tolist():
        rx = (C * ux - S * uy + ONE // 2) >> 14
        ry = (S * ux + C * uy + ONE // 2) >> 14
        cx = (int(sensor[0]) + ddx * cfg.xy_step + rx) >> 10
        cy = (int(sensor[1]) + ddy * cfg.xy_step + ry) >> 10
        if 0 <= cx < W and 0 <= cy < H and known[cy, cx]:
            total += int(L[cy, cx])
    return total


def scores_np(L, known, cells, sensor, cfg):
    """Step 3 for every candidate at once: int64 [candidates]."""
    cfg = ScanMatchConfig.from_any(cfg)
    H, W = L.shape
    Lk = np.where(known, L, 0).astype(np.int64).reshape(-1)
    u = np.asarray(cells, np.int64).reshape(-1, 2)
    wx, wy, wt = 2 * cfg.nx + 1, 2 * cfg.ny + 1, 2 * cfg.nt + 1
    out = np.zeros((wt, wy, wx), np.int64)
    bx = int(sensor[0]) + (np.arange(wx, dtype=np.int64) - cfg.nx) * cfg.xy_step          # [wx]
    by = int(sensor[1]) + (np.arange(wy, dtype=np.int64) - cfg.ny) * cfg.xy_step          # [wy]
    for it in range(wt):
        C, S = (int(v) for v in _TRIG[((it - cfg.nt) * cfg.theta_step) & (HEADINGS - 1)])
        rx = (C * u[:, 0] - S * u[:, 1] + ONE // 2) >> 14
        ry = (S * u[:, 0] + C * u[:, 1] + ONE // 2) >> 14
        cx = (bx[:, None] + rx[None, :]) >> 10                   # [wx, n]
        cy = (by[:, None] + ry[None, :]) >> 10                   # [wy, n]
        okx, oky = (cx >= 0) & (cx < W), (cy >= 0) & (cy < H)
        cxc, cyc = np.where(okx, cx, 0), np.where(oky, cy, 0)
        for iy in range(wy):
            v = Lk[cyc[iy][None, :] * W + cxc]                   # [wx, n]
            out[it, iy] = np.where(okx & oky[iy][None, :], v, 0).sum(axis=1)
    return out.reshape(-1)


def best_np(scores, cfg, n_scan, ignored, status=0):
    """Step 4: the result words int32 [8] from all candidates' scores and the status bits already known (NO_MAP, OUTSIDE)."""
    cfg = ScanMatchConfig.from_any(cfg)
    s = np.asarray(scores, np.int64).reshape(-1)
    if s.shape != (cfg.candidates,):
        raise ValueError(f"best_np: {s.shape[0]} scores, the configuration has {cfg.candidates} candidates")
    best_key, best_c = None, -1
    for c in range(cfg.candidates):
        ddx, ddy, ddt = _delta(cfg, c)
        key = ((SCORE_BIAS - int(s[c])) << 32) | ((abs(ddt) + abs(ddy) + abs(ddx)) << 16) | c
        if best_key is None or key < best_key:
            best_key, best_c = key, c
    ddx, ddy, ddt = _delta(cfg, best_c)
    best = int(s[best_c])
    centre = (cfg.nt * (2 * cfg.ny + 1) + cfg.ny) * (2 * cfg.nx + 1) + cfg.nx
    status = int(status)
    if n_scan < cfg.min_cells:
        status |= FEW_CELLS
    if best * 100 < cfg.min_mean * int(n_scan):
        status |= LOW_SCORE
    if any(n > 0 and abs(d) == n for d, n in ((ddx, cfg.nx), (ddy, cfg.ny), (ddt, cfg.nt))):
        status |= EDGE
    return np.array([status, ddx, ddy, ddt, best, int(s[centre]), int(n_scan), int(ignored)], np.int32)


def match_grid_np(occ_cfg, logodds, known, origin_cell, points, pose, cfg, mask=None, ground=None):
    """Steps 1 .. 4 on a map given as arrays: logodds int16 [H, W], known bool [H, W], origin_cell (ox, oy) or None (no
    map) -> (words int32 [8], scores int64 [candidates]).  mask as scan_cells_np takes it."""
    oc = _occ.OccupancyConfig.from_any(occ_cfg)
    cfg = ScanMatchConfig.from_any(cfg)
    L, K = np.asarray(logodds), np.asarray(known, bool)
    if L.shape != (oc.height, oc.width) or K.shape != L.shape:
        raise ValueError(f"scan_match: logodds and known must be [{oc.height}, {oc.width}], got {L.shape} and {K.shape}")
    P = _swp.check_poses(np.asarray(pose, np.float64)[None], 1)[0]
    cells, (_, ignored, n_scan) = scan_cells_np(oc, points, P, mask, ground)
    status, sensor = 0, (0, 0)
    if origin_cell is None:
        status = NO_MAP
    else:
        sensor = sensor_subcells(oc, P, origin_cell)
        if not (0 <= sensor[0] >> 10 < oc.width and 0 <= sensor[1] >> 10 < oc.height):
            status = OUTSIDE
    scores = np.zeros(cfg.candidates, np.int64) if status else scores_np(L, K, cells, sensor, cfg)
    return best_np(scores, cfg, n_scan, ignored, status), scores


def match_np(occupancy_map, points, pose, cfg, mask=None, ground=None):
    """Steps 1 .. 4 against an occupancy.OccupancyMap as it stands -> (words int32 [8], scores int64 [candidates])."""
    m = occupancy_map
    return match_grid_np(m.cfg, m._L, m._known, m.origin_cell, points, pose, cfg, mask, ground)


def corrected_pose(pose, words, occ_cfg, cfg):
    """Step 5: the pose [3, 4] float64 the words correct the prior to (the prior itself under NO_MAP, OUTSIDE, FEW_CELLS
    or LOW_SCORE)."""
    oc = _occ.OccupancyConfig.from_any(occ_cfg)
    cfg = ScanMatchConfig.from_any(cfg)
    P = np.array(pose, np.float64)
    w = [int(v) for v in np.asarray(words).reshape(-1)]
    if P.shape != (3, 4) or len(w) != PP_SCAN_RESULT:
        raise ValueError(f"corrected_pose: a pose [3, 4] and {PP_SCAN_RESULT} words, got {P.shape} and {len(w)}")
    if w[0] & REJECT:
        return P
    a = 2.0 * math.pi * float(w[3] * cfg.theta_step) / float(HEADINGS)
    Rz = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    out = P.copy()
    out[:, :3] = Rz @ P[:, :3]
    out[0, 3] = P[0, 3] + float(w[1] * cfg.xy_step) * oc.resolution / float(SUB)
    out[1, 3] = P[1, 3] + float(w[2] * cfg.xy_step) * oc.resolution / float(SUB)
    return out


def scan_match_grids(logodds, known, points, poses, origin_cells, occ_cfg, cfg, device=0):
    """The GPU stage without an engine (pp_scan_match_grids): logodds int16 [B, H, W], known bool [B, H, W], points a list
    of B float32 [n, F >= 3] arrays (one F), poses float64 [B, 3, 4], origin_cells a list of B (ox, oy) or None (no map)
    -> (words int32 [B, 8], scores int32 [B, candidates])."""
    oc = _occ.OccupancyConfig.from_any(occ_cfg)
    cfg = ScanMatchConfig.from_any(cfg)
    L = np.ascontiguousarray(logodds, np.int16)
    K = np.ascontiguousarray(np.asarray(known, bool), np.uint8)
    if L.ndim != 3 or L.shape[1:] != (oc.height, oc.width) or K.shape != L.shape:
        raise ValueError(f"scan_match_grids: logodds and known must be [B, {oc.height}, {oc.width}], got {L.shape} and {K.shape}")
    B = L.shape[0]
    frames = [np.asarray(f) for f in points]
    if len(frames) != B or any(f.dtype != np.float32 or f.ndim != 2 or f.shape[1] < 3 or f.shape[1] != frames[0].shape[1] for f in frames):
        raise ValueError(f"scan_match_grids: points must be {B} float32 [n, F >= 3] arrays of one F")
    P = _swp.check_poses(poses, B)
    if len(origin_cells) != B:
        raise ValueError(f"scan_match_grids: {len(origin_cells)} origin cells for {B} grids")
    has = np.array([o is not None for o in origin_cells], np.int32)
    org = np.array([(0, 0) if o is None else (int(o[0]), int(o[1])) for o in origin_cells], np.int32).reshape(B, 2)
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum([len(f) for f in frames])
    F = frames[0].shape[1]
    flat = np.ascontiguousarray(np.concatenate(frames, axis=0) if off[-1] else np.zeros((0, F), np.float32))
    trig = np.ascontiguousarray(_TRIG)
    words = np.zeros((B, PP_SCAN_RESULT), np.int32)
    scores = np.zeros((B, cfg.candidates), np.int32)
    L_ = _lib.lib()
    po, pc = _lib.PPOccupancyConfig(), _lib.PPScanMatchConfig()
    for k, v in oc.to_dict().items():
        setattr(po, k, v)
    for k, v in cfg.to_dict().items():
        setattr(pc, k, v)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    st = L_.pp_scan_match_grids(int(device), vp(L), vp(K), B, oc.height, oc.width, vp(flat), vp(off), F, vp(P), vp(org), vp(has),
                                ctypes.byref(po), ctypes.byref(pc), vp(trig), len(trig), vp(words), vp(scores))
    if st != 0:
        msg = L_.pp_last_error(None)
        raise RuntimeError(f"pp_scan_match_grids failed ({st}): {msg.decode() if msg else ''}")
    return words, scores
