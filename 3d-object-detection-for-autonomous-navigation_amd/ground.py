"""Ground plane per frame: one plane z = a x + b y + c fitted by RANSAC, and per row a class from its vertical residual to
that plane -- so that "floor" and "obstacle" no longer hang on two fixed z numbers of a level sensor.

The reference has no such path, so nothing here is parity with it.  This module STATES the rule: `ground_np` is the numpy
restatement that the GPU stage (csrc/ground.hip behind Engine.set_ground / ground_async / ground) mirrors operation for
operation.  All arithmetic is float64 with + - * / and comparisons, every operation written out in its order below; there
is no sqrt and no transcendental call, and the library is built without contraction, so the stage EQUALS the restatement
bit for bit: the plane's three doubles, every count, every word.  No margin set is needed.

Rows are float32 [n, F >= 3], widened to float64.

1. CANDIDATES.  A row is a candidate iff x, y and z are finite, (x * x + y * y) <= max_range * max_range and
   z <= cand_z_max.  A NaN fails.

2. HYPOTHESES.  K = hypotheses, 1 <= K <= PP_GROUND_MAX_HYP.  The host draws `triples` uint32 [K, 3] per frame
   (`draw_triples`: a counter-based generator, a function of (seed, call_index) alone); entry u names row
   j = (u * n) >> 32 in 64-bit integers, n the frame's row count.  For the rows p0, p1, p2:
       e1 = p1 - p0, e2 = p2 - p0                                   (component by component)
       nx = (e1y * e2z) - (e1z * e2y);  ny = (e1z * e2x) - (e1x * e2z);  nz = (e1x * e2y) - (e1y * e2x)
   INVALID if n == 0, if any of the three rows is no candidate, or if nz == 0.  Otherwise
       a = -nx / nz;  b = -ny / nz;  c = z0 - ((a * x0) + (b * y0))
   and INVALID unless (a * a + b * b) <= max_slope * max_slope and h_min <= -c and -c <= h_max (-c is the sensor's height
   over the plane; a NaN fails).

3. SCORE.  count[k] = the candidate rows with |z - (((a * x) + (b * y)) + c)| <= inlier_dist.  The winner is the least key
   ((2^31 - count) << 32) | k over the valid hypotheses: most inliers, then the least k.  Without a valid hypothesis, or
   with count < min_inliers, the frame takes the FALLBACK plane (0, 0, fallback_c) and status FALLBACK.

4. REFIT (refine = 1, status OK), over the winner's inliers only.  q(v) = floor(v * 256) as int64 of x, y and z; the nine
   integer sums N, Sx, Sy, Sz, Sxx, Sxy, Syy, Sxz, Syz of qx, qy, qz (`SUMS` names their order).  `check_refine` holds the
   configuration to bounds under which every |q| <= 2^14 and every sum is exact as int64 and as float64.  Then, each sum
   as a float64:
       cxx = (N * Sxx) - (Sx * Sx);  cxy = (N * Sxy) - (Sx * Sy);  cyy = (N * Syy) - (Sy * Sy)
       cxz = (N * Sxz) - (Sx * Sz);  cyz = (N * Syz) - (Sy * Sz)
       det = (cxx * cyy) - (cxy * cxy)
       a = ((cxz * cyy) - (cyz * cxy)) / det;  b = ((cyz * cxx) - (cxz * cxy)) / det
       c = (((Sz - (a * Sx)) - (b * Sy)) / N) / 256
   The refit stands only if det > 0 and it passes the slope and height tests of step 2; otherwise the hypothesis's own
   plane stands.  The info word `refit` says which.  (The floor of q shifts c by at most 1 / 256 m; that is the price of
   sums that are exact in any order, which is what lets the device add them with integer atomics.)

5. CLASSES.  Per row r = z - (((a * x) + (b * y)) + c) with the frame's final plane: a NaN gives IGNORED;
   |r| <= ground_dist GROUND; ground_dist < r <= overhead_max OBSTACLE; r > overhead_max OVERHEAD; r < -ground_dist BELOW.
   The device writes two bit planes per frame in the object mask's word layout (bit i & 63 of word i >> 6, zero past the
   frame's rows): `ground` and `obstacle`; a row with both bits clear is ignored by the readers.  PP_GROUND_INFO int32
   words per frame (`INFO`): status, winner, inliers, candidates, valid, ground, obstacle, overhead, below, ignored, refit,
   rows.  winner is -1 and inliers 0 without a valid hypothesis.

READERS, while their name is in `consumers` (each restatement takes ground=None and is unchanged without it; ground is the
pair (ground bool [n], obstacle bool [n])):
  occupancy   OccupancyMap.update(points, pose, mask, ground): the z <= z_max test and the z >= z_min split are dropped; an
              in-window, in-range row is a HIT iff OBSTACLE, a GROUND return iff GROUND, ignored otherwise.  An object-mask
              bit still turns a hit into a masked end.
  scan_match  scan_cells_np(..., ground=): a row takes part iff OBSTACLE and not object-masked.
  costmap     point_layer_np / costmap_np(..., ground=): an in-grid row marks its cell observed, as now, and adds to the
              count iff OBSTACLE and not object-masked.

`attitude(plane)` gives roll, pitch and height of the sensor over the plane (atan on the host only).

Out of scope: a plane carried from the previous frame as an extra hypothesis; several planes, kerbs and stairs; negative
obstacles (BELOW rows are ignored); a perpendicular distance instead of the vertical residual; levelling the detector's
own input; the sweeps stage.
"""
import ctypes
import dataclasses
import math

import numpy as np

from . import _lib
from ._lib import PP_GROUND_MAX_HYP as MAX_HYP, PP_GROUND_INFO
from .object_mask import pack_words, unpack_words  # noqa: F401  (the bit planes share the object mask's word layout)

CONSUMERS = {"occupancy": _lib.PP_GROUND_OCCUPANCY, "scan_match": _lib.PP_GROUND_SCAN_MATCH, "costmap": _lib.PP_GROUND_COSTMAP}
INFO = ("status", "winner", "inliers", "candidates", "valid", "ground", "obstacle", "overhead", "below", "ignored", "refit", "rows")
SUMS = ("N", "Sx", "Sy", "Sz", "Sxx", "Sxy", "Syy", "Sxz", "Syz")
OK, FALLBACK = 0, 1
IGNORED, GROUND, OBSTACLE, OVERHEAD, BELOW = 0, 1, 2, 3, 4      # classify_np's codes
Q = 256.0                  # q(v) = floor(v * Q)
REFINE_LIMIT = 64.0        # metres: |x|, |y|, |z| of a refit's inlier stay under it, so |q| <= 2^14
assert len(INFO) == PP_GROUND_INFO

_FLOATS = ("max_range", "cand_z_max", "max_slope", "h_min", "h_max", "inlier_dist", "ground_dist", "overhead_max", "fallback_c")


@dataclasses.dataclass
class GroundConfig:
    """hypotheses     K, 1 .. PP_GROUND_MAX_HYP planes through three drawn rows each
    seed           of `draw_triples` (a 64-bit unsigned integer)
    max_range      metres, > 0: a candidate has (x * x + y * y) <= max_range * max_range
    cand_z_max     metres: ... and z <= cand_z_max (sensor frame; rows above it cannot be floor)
    max_slope      >= 0: a plane stands only if (a * a + b * b) <= max_slope * max_slope
    h_min, h_max   metres, h_min <= h_max: ... and h_min <= -c <= h_max, the sensor's height over the plane
    inlier_dist    metres, >= 0: the vertical residual of an inlier
    min_inliers    >= 1: a winner with fewer gives the fallback plane
    refine         1: the least-squares refit over the winner's inliers (step 4); 0 skips it
    ground_dist    metres, >= 0: |r| <= ground_dist is GROUND
    overhead_max   metres, >= ground_dist: ground_dist < r <= overhead_max is OBSTACLE
    fallback_c     metres: the plane (0, 0, fallback_c) of a frame without a fit
    consumers      the readers that use the classes: names out of "occupancy", "scan_match", "costmap" (or their
                   PP_GROUND_* bits as an int)"""
    hypotheses: int = 128
    seed: int = 0
    max_range: float = 20.0
    cand_z_max: float = 0.0
    max_slope: float = 0.3
    h_min: float = 0.2
    h_max: float = 3.0
    inlier_dist: float = 0.05
    min_inliers: int = 64
    refine: int = 1
    ground_dist: float = 0.1
    overhead_max: float = 2.0
    fallback_c: float = -1.4
    consumers: object = ("occupancy", "scan_match", "costmap")

    def __post_init__(self):
        for f in _FLOATS:
            v = getattr(self, f)
            try:
                if isinstance(v, bool):
                    raise TypeError
                v = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"GroundConfig: {f} must be a number, got {getattr(self, f)!r}")
            if not math.isfinite(v):
                raise ValueError(f"GroundConfig: {f} = {v} is not finite")
            setattr(self, f, v)
        for f, lo, hi in (("hypotheses", 1, MAX_HYP), ("seed", 0, 2 ** 64 - 1), ("min_inliers", 1, 2 ** 31 - 1), ("refine", 0, 1)):
            v = getattr(self, f)
            if isinstance(v, bool) and f == "refine":
                v = int(v)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"GroundConfig: {f} = {v!r} outside [{lo}, {hi}]")
            setattr(self, f, int(v))
        if not self.max_range > 0.0:
            raise ValueError(f"GroundConfig: max_range = {self.max_range} must be > 0")
        for f in ("max_slope", "inlier_dist", "ground_dist"):
            if not getattr(self, f) >= 0.0:
                raise ValueError(f"GroundConfig: {f} = {getattr(self, f)} must be >= 0")
        if not self.h_min <= self.h_max:
            raise ValueError(f"GroundConfig: h_min = {self.h_min} above h_max = {self.h_max}")
        if not self.overhead_max >= self.ground_dist:
            raise ValueError(f"GroundConfig: overhead_max = {self.overhead_max} under ground_dist = {self.ground_dist}")
        c = self.consumers
        if isinstance(c, bool):
            raise ValueError(f"GroundConfig: consumers = {c!r}")
        if isinstance(c, (int, np.integer)):
            bits = int(c)
            if bits < 0 or bits & ~sum(CONSUMERS.values()):
                raise ValueError(f"GroundConfig: consumers = {bits} holds bits outside {sum(CONSUMERS.values())}")
        else:
            names = [c] if isinstance(c, str) else list(c)
            unknown = [n for n in names if n not in CONSUMERS]
            if unknown:
                raise ValueError(f"GroundConfig: consumers {unknown!r} are none of {sorted(CONSUMERS)}")
            bits = 0
            for n in names:
                bits |= CONSUMERS[n]
        self.consumers = tuple(n for n, b in CONSUMERS.items() if bits & b)

    @property
    def consumer_bits(self):
        return sum(CONSUMERS[n] for n in self.consumers)

    def to_dict(self):
        """The fields as pp_ground_config holds them: consumers as its bits."""
        d = dataclasses.asdict(self)
        d["consumers"] = self.consumer_bits
        return d

    @classmethod
    def from_any(cls, cfg):
        """A GroundConfig, a dict of its fields (unknown keys raise, naming them) or True (the defaults)."""
        if isinstance(cfg, cls):
            return cfg
        if cfg is True:
            return cls()
        if isinstance(cfg, dict):
            unknown = set(cfg) - {f.name for f in dataclasses.fields(cls)}
            if unknown:
                raise ValueError(f"ground: unknown keys {sorted(unknown)}")
            return cls(**cfg)
        raise ValueError(f"ground: a GroundConfig, a dict of its fields or True, got {cfg!r}")


def refine_reach(cfg):
    """The largest |z| an inlier of a valid plane can have, up to rounding: |a x + b y| <= max_slope * max_range by
    Cauchy-Schwarz, |c| <= max(|h_min|, |h_max|), and the inlier band."""
    c = GroundConfig.from_any(cfg)
    return c.max_slope * c.max_range + max(abs(c.h_min), abs(c.h_max)) + c.inlier_dist


def check_refine(cfg, max_rows):
    """What set_ground refuses of refine = 1 (ValueError naming the bound): max_range <= 64 and |cand_z_max| <= 64, the
    inliers' reach in z (`refine_reach`) at most 63 -- a metre of slack over the rounding of the residual -- and
    max_rows * 2^28 < 2^53.  Then |q| <= 2^14 for x, y and z of every inlier, every product of two q is at most 2^28, and
    every sum is below 2^53: exact as int64 in any order, and exact as float64."""
    c = GroundConfig.from_any(cfg)
    if not c.refine:
        return
    if not c.max_range <= REFINE_LIMIT:
        raise ValueError(f"ground: refine needs max_range <= {REFINE_LIMIT:g}, got {c.max_range}")
    if not abs(c.cand_z_max) <= REFINE_LIMIT:
        raise ValueError(f"ground: refine needs |cand_z_max| <= {REFINE_LIMIT:g}, got {c.cand_z_max}")
    if not refine_reach(c) <= REFINE_LIMIT - 1.0:
        raise ValueError(f"ground: refine needs max_slope * max_range + max(|h_min|, |h_max|) + inlier_dist <= {REFINE_LIMIT - 1.0:g}, "
                         f"got {refine_reach(c)}")
    if not int(max_rows) * 2 ** 28 < 2 ** 53:
        raise ValueError(f"ground: refine needs rows per frame * 2^28 < 2^53, got {max_rows} rows")


def draw_triples(seed, call_index, batch, K):
    """uint32 [batch, K, 3]: the triples of call `call_index` under `seed` -- a Philox stream keyed by the seed with the
    call index as its counter's high word, so a call's triples are a function of (seed, call_index) alone."""
    seed, call_index = int(seed), int(call_index)
    if not 0 <= seed < 2 ** 64 or not 0 <= call_index < 2 ** 64:
        raise ValueError(f"draw_triples: seed = {seed} and call_index = {call_index} must be 64-bit unsigned integers")
    bg = np.random.Philox(key=np.array([seed, 0x67726F756E64], np.uint64), counter=np.array([0, 0, 0, call_index], np.uint64))
    return np.random.Generator(bg).integers(0, 2 ** 32, size=(int(batch), int(K), 3), dtype=np.uint64).astype(np.uint32)


def _xyz(points):
    p = np.asarray(points)
    if p.dtype != np.float32 or p.ndim != 2 or p.shape[1] < 3:
        raise ValueError(f"ground: points must be float32 [n, F >= 3], got {p.dtype} {p.shape}")
    return p[:, 0].astype(np.float64), p[:, 1].astype(np.float64), p[:, 2].astype(np.float64)


def _triples(triples, K):
    t = np.asarray(triples)
    if t.dtype != np.uint32 or t.shape != (K, 3):
        raise ValueError(f"ground: triples must be uint32 [{K}, 3], got {t.dtype} {t.shape}")
    return t.astype(np.uint64)


def candidates_np(points, cfg):
    """bool [n]: step 1."""
    c = GroundConfig.from_any(cfg)
    x, y, z = _xyz(points)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ((x * x + y * y) <= c.max_range * c.max_range)
                & (z <= c.cand_z_max))


def _plane_ok(a, b, c0, c):
    return (a * a + b * b) <= c.max_slope * c.max_slope and c.h_min <= -c0 and -c0 <= c.h_max


def hypotheses_np(points, triples, cfg):
    """Step 2 for one frame: (planes float64 [K, 3] = a b c (zeros where invalid), valid bool [K])."""
    c = GroundConfig.from_any(cfg)
    x, y, z = _xyz(points)
    n, K = len(x), c.hypotheses
    t = _triples(triples, K)
    cand = candidates_np(points, c)
    planes, valid = np.zeros((K, 3), np.float64), np.zeros(K, bool)
    if n == 0:
        return planes, valid
    rows = ((t * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    with np.errstate(all="ignore"):
        for k in range(K):
            j0, j1, j2 = (int(v) for v in rows[k])
            if not (cand[j0] and cand[j1] and cand[j2]):
                continue
            e1x, e1y, e1z = x[j1] - x[j0], y[j1] - y[j0], z[j1] - z[j0]
            e2x, e2y, e2z = x[j2] - x[j0], y[j2] - y[j0], z[j2] - z[j0]
            nx = (e1y * e2z) - (e1z * e2y)
            ny = (e1z * e2x) - (e1x * e2z)
            nz = (e1x * e2y) - (e1y * e2x)
            if nz == 0.0:
                continue
            a = -nx / nz
            b = -ny / nz
            c0 = z[j0] - ((a * x[j0]) + (b * y[j0]))
            if _plane_ok(a, b, c0, c):
                planes[k] = (a, b, c0)
                valid[k] = True
    return planes, valid


def _inliers(x, y, z, cand, plane, dist):
    a, b, c0 = (np.float64(v) for v in plane)
    with np.errstate(invalid="ignore", over="ignore"):
        return cand & (np.abs(z - (((a * x) + (b * y)) + c0)) <= dist)


def counts_np(points, planes, valid, cfg):
    """Step 3's counts for one frame, int32 [K] (0 where invalid)."""
    c = GroundConfig.from_any(cfg)
    x, y, z = _xyz(points)
    cand = candidates_np(points, c)
    out = np.zeros(len(planes), np.int32)
    for k in np.nonzero(valid)[0]:
        out[k] = int(_inliers(x, y, z, cand, planes[k], c.inlier_dist).sum())
    return out


def pick_np(counts, valid):
    """(winner k or -1, its count): the least key ((2^31 - count) << 32) | k over the valid hypotheses."""
    ks = np.nonzero(valid)[0]
    if len(ks) == 0:
        return -1, 0
    keys = [(((1 << 31) - int(counts[k])) << 32) | int(k) for k in ks]
    k = min(keys) & 0xFFFFFFFF
    return int(k), int(counts[k])


def moments_np(points, plane, cfg):
    """Step 4's nine sums over the inliers of `plane`, int64 [9] in SUMS' order."""
    c = GroundConfig.from_any(cfg)
    x, y, z = _xyz(points)
    m = _inliers(x, y, z, candidates_np(points, c), plane, c.inlier_dist)
    qx, qy, qz = (np.floor(v[m] * Q).astype(np.int64) for v in (x, y, z))
    return np.array([int(m.sum()), qx.sum(), qy.sum(), qz.sum(), (qx * qx).sum(), (qx * qy).sum(), (qy * qy).sum(),
                     (qx * qz).sum(), (qy * qz).sum()], np.int64)


def fit_np(sums, cfg):
    """Step 4's plane from the nine sums: (plane float64 [3], stands bool).  stands False: det <= 0 (or a NaN), or the
    plane fails the slope or height test -- the hypothesis's own plane then stands."""
    c = GroundConfig.from_any(cfg)
    N, Sx, Sy, Sz, Sxx, Sxy, Syy, Sxz, Syz = (np.float64(int(v)) for v in sums)
    with np.errstate(all="ignore"):
        cxx = (N * Sxx) - (Sx * Sx)
        cxy = (N * Sxy) - (Sx * Sy)
        cyy = (N * Syy) - (Sy * Sy)
        cxz = (N * Sxz) - (Sx * Sz)
        cyz = (N * Syz) - (Sy * Sz)
        det = (cxx * cyy) - (cxy * cxy)
        if not det > 0.0:
            return np.zeros(3), False
        a = ((cxz * cyy) - (cyz * cxy)) / det
        b = ((cyz * cxx) - (cxz * cxy)) / det
        c0 = (((Sz - (a * Sx)) - (b * Sy)) / N) / Q
    if not _plane_ok(a, b, c0, c):
        return np.zeros(3), False
    return np.array([a, b, c0], np.float64), True


def classify_np(points, plane, cfg):
    """Step 5 for one frame: int8 [n] of IGNORED, GROUND, OBSTACLE, OVERHEAD, BELOW."""
    c = GroundConfig.from_any(cfg)
    x, y, z = _xyz(points)
    a, b, c0 = (np.float64(v) for v in plane)
    with np.errstate(invalid="ignore", over="ignore"):
        r = z - (((a * x) + (b * y)) + c0)
        cls = np.full(len(x), IGNORED, np.int8)
        cls[np.abs(r) <= c.ground_dist] = GROUND
        cls[(r > c.ground_dist) & (r <= c.overhead_max)] = OBSTACLE
        cls[r > c.overhead_max] = OVERHEAD
        cls[r < -c.ground_dist] = BELOW
    return cls


def ground_np(points, cfg, triples):
    """One frame, steps 1 .. 5: a dict of plane float64 [3], info int32 [PP_GROUND_INFO] (INFO's order), ground and
    obstacle bool [n], classes int8 [n], sums int64 [9] (zeros unless the refit ran), and the steps' own results
    planes [K, 3], valid [K], counts [K]."""
    c = GroundConfig.from_any(cfg)
    planes, valid = hypotheses_np(points, triples, c)
    counts = counts_np(points, planes, valid, c)
    k, inl = pick_np(counts, valid)
    status = OK if k >= 0 and inl >= c.min_inliers else FALLBACK
    plane = planes[k].copy() if status == OK else np.array([0.0, 0.0, c.fallback_c])
    sums, refit = np.zeros(9, np.int64), 0
    if status == OK and c.refine:
        sums = moments_np(points, plane, c)
        fitted, stands = fit_np(sums, c)
        if stands:
            plane, refit = fitted, 1
    cls = classify_np(points, plane, c)
    info = np.array([status, k, inl, int(candidates_np(points, c).sum()), int(valid.sum()),
                     int((cls == GROUND).sum()), int((cls == OBSTACLE).sum()), int((cls == OVERHEAD).sum()),
                     int((cls == BELOW).sum()), int((cls == IGNORED).sum()), refit, len(cls)], np.int32)
    return {"plane": plane, "info": info, "ground": cls == GROUND, "obstacle": cls == OBSTACLE, "classes": cls, "sums": sums,
            "planes": planes, "valid": valid, "counts": counts}


def attitude(plane):
    """(roll, pitch, height) of the sensor over the plane z = a x + b y + c, radians and metres: pitch = atan(a) (positive:
    the floor rises ahead, the sensor's nose is down), roll = -atan(b), height = -c along the sensor's z.  Host only."""
    a, b, c0 = (float(v) for v in plane)
    return -math.atan(b), math.atan(a), -c0


def check_classes(ground, n, who):
    """The (ground bool [n], obstacle bool [n]) pair the readers' restatements take."""
    try:
        g, o = ground
    except (TypeError, ValueError):
        raise ValueError(f"{who}: ground must be the pair (ground bool [n], obstacle bool [n])")
    g, o = np.asarray(g, bool).reshape(-1), np.asarray(o, bool).reshape(-1)
    if g.shape != (n,) or o.shape != (n,):
        raise ValueError(f"{who}: ground must be two bool [{n}], got {g.shape} and {o.shape}")
    return g, o


def ground(points, cfg, triples, device=0):
    """The GPU stage without an engine (pp_ground_points): points a list of B float32 [n, F >= 3] arrays (one F), triples
    uint32 [B, K, 3] -> a dict of planes float64 [B, 3], info int32 [B, PP_GROUND_INFO], ground and obstacle (lists of B
    bool [n]), ground_words and obstacle_words uint64 [B, ceil(max n / 64)], sums int64 [B, 9], counts int32 [B, K]."""
    c = GroundConfig.from_any(cfg)
    frames = [np.asarray(f) for f in points]
    B = len(frames)
    if B < 1 or any(f.dtype != np.float32 or f.ndim != 2 or f.shape[1] < 3 or f.shape[1] != frames[0].shape[1] for f in frames):
        raise ValueError("ground: points must be a list of float32 [n, F >= 3] arrays of one F")
    t = np.ascontiguousarray(triples)
    if t.dtype != np.uint32 or t.shape != (B, c.hypotheses, 3):
        raise ValueError(f"ground: triples must be uint32 [{B}, {c.hypotheses}, 3], got {t.dtype} {t.shape}")
    check_refine(c, max(len(f) for f in frames))
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum([len(f) for f in frames])
    F = frames[0].shape[1]
    flat = np.ascontiguousarray(np.concatenate(frames, axis=0) if off[-1] else np.zeros((0, F), np.float32))
    wpf = max((max(len(f) for f in frames) + 63) // 64, 1)
    gw, ow = np.zeros((B, wpf), np.uint64), np.zeros((B, wpf), np.uint64)
    planes, info = np.zeros((B, 3), np.float64), np.zeros((B, PP_GROUND_INFO), np.int32)
    sums, counts = np.zeros((B, 9), np.int64), np.zeros((B, c.hypotheses), np.int32)
    pc = _lib.PPGroundConfig(**c.to_dict())
    L_ = _lib.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    st = L_.pp_ground_points(int(device), vp(flat), vp(off), F, B, ctypes.byref(pc), vp(t), vp(planes), vp(info), vp(gw), vp(ow), wpf,
                             vp(sums), vp(counts))
    if st != 0:
        msg = L_.pp_last_error(None)
        raise RuntimeError(f"pp_ground_points failed ({st}): {msg.decode() if msg else ''}")
    return {"planes": planes, "info": info, "ground": [unpack_words(gw[b], len(frames[b])) for b in range(B)],
            "obstacle": [unpack_words(ow[b], len(frames[b])) for b in range(B)], "ground_words": gw, "obstacle_words": ow,
            "sums": sums, "counts": counts}
