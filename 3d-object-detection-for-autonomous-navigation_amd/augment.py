"""Training-time augmentation of a frame and its ground-truth boxes (SURVEY section 8f, row 15 -- prep_pointcloud's
training branch after GT-database sampling, load_data.py:2751-2866).

Stages, per frame, in the reference's order:
  1. noise_per_object_v3_   load_data.py:913-1006 (selection: noise_per_box :1137-1166 or noise_per_box_v2_ :41-94,
                            collision test box_collision_test :1248-1328, points_transform_ :1017-1033,
                            box3d_transform_ :1008-1015)
  2. drop the invalid boxes :2774-2778
  3. random_flip            :890-910
  4. global_rotation        :794-803   (turns points and centres by -theta, adds theta to the yaw: kept as is)
  5. global_scaling_v2      :883-888
  6. global_translate       :865-881   (the z shift draws with sigma0, not sigma2: kept as is)
  7. limit_period(yaw, 0.5, 2 pi)
  8. np.random.shuffle(points) -- here a keyed permutation, `shuffle_perm`, from one drawn seed
  9. filter_gt_box_outside_range_by_center :96-107

The random numbers are drawn on the host (`draw`) with the same numpy calls, arguments and order as the reference,
so a seeded RandomState is consumed exactly as the reference consumes it (the shuffle aside: one 32-bit seed
instead of N swaps).  The stages themselves run on the GPU (csrc/augment.hip: Engine.augment, Trainer(augment=...));
`augment_np` is their host float64 restatement, which the tests compare against.

Collision rule.  box_collision_test tests `ret[i, j] is False` / `is True` on a numpy bool, which Python never finds
identical to the bool singletons: executed as written, the containment test never runs and the edge loop's break
only leaves the inner loop.  Two boxes therefore collide when their standup boxes overlap (iw > 0 and ih > 0) AND
two of their edges properly cross.  A box inside another, or sharing collinear edges with it, does not collide.  That
is the rule implemented here and on the GPU; tests/golden/ref_augment.npz, produced by running the reference's own
functions, pins it.
"""
import numpy as np

PP_AUG_MAX_TRY = 128
PP_MAX_GT_PER_FRAME = 256

# configs/train.yaml, train_input_reader
_DEFAULTS = {
    "groundtruth_rotation_uniform_noise": [-0.39269908169, 0.39269908169],
    "groundtruth_localization_noise_std": [0.15, 0.15, 0.05],
    "global_random_rotation_range_per_object": [0.0, 0.0],
    "global_rotation_uniform_noise": [-0.178539816, 0.178539816],
    "global_scaling_uniform_noise": [0.95, 1.05],
    "global_loc_noise_std": [0.1, 0.1, 0.2],
}


def _pair(cfg, key):
    v = cfg.get(key, _DEFAULTS[key])
    try:
        a = [float(x) for x in v]
    except TypeError:
        raise ValueError(f"{key}: expected a list of 2 numbers, got {v!r}") from None
    if len(a) != 2:
        raise ValueError(f"{key}: expected 2 values, got {len(a)}")
    if not all(np.isfinite(a)):
        raise ValueError(f"{key}: values must be finite")
    if a[0] > a[1]:
        raise ValueError(f"{key}: lower bound {a[0]} > upper bound {a[1]}")
    return tuple(a)


def _stds(cfg, key):
    v = cfg.get(key, _DEFAULTS[key])
    try:
        a = [float(x) for x in v]
    except TypeError:
        raise ValueError(f"{key}: expected a list of 3 numbers, got {v!r}") from None
    if len(a) != 3:
        raise ValueError(f"{key}: expected 3 values, got {len(a)}")
    if not all(np.isfinite(a)) or min(a) < 0:
        raise ValueError(f"{key}: standard deviations must be finite and >= 0")
    return tuple(a)


class AugmentConfig:
    """The six augmentation keys of train_input_reader plus num_try (the loader passes 100)."""

    def __init__(self, rot_noise, loc_std, grot_range, global_rot, scaling, global_loc_std, num_try=100):
        self.rot_noise = tuple(rot_noise)
        self.loc_std = tuple(loc_std)
        self.grot_range = tuple(grot_range)
        self.global_rot = tuple(global_rot)
        self.scaling = tuple(scaling)
        self.global_loc_std = tuple(global_loc_std)
        self.num_try = int(num_try)

    @classmethod
    def from_input_reader(cls, cfg=None):
        cfg = dict(cfg or {})
        scaling = _pair(cfg, "global_scaling_uniform_noise")
        if scaling[0] <= 0:
            raise ValueError(f"global_scaling_uniform_noise: scale must be > 0, got {scaling}")
        num_try = cfg.get("num_try", 100)
        if isinstance(num_try, bool) or int(num_try) != num_try or not 1 <= int(num_try) <= PP_AUG_MAX_TRY:
            raise ValueError(f"num_try must be an integer in 1..{PP_AUG_MAX_TRY}, got {num_try!r}")
        return cls(_pair(cfg, "groundtruth_rotation_uniform_noise"), _stds(cfg, "groundtruth_localization_noise_std"),
                   _pair(cfg, "global_random_rotation_range_per_object"), _pair(cfg, "global_rotation_uniform_noise"),
                   scaling, _stds(cfg, "global_loc_noise_std"), int(num_try))

    @property
    def global_rot_per_object(self):
        """noise_per_object_v3_'s enable_grot (load_data.py:937-938): the v2 selection rule."""
        return bool(np.abs(self.grot_range[0] - self.grot_range[1]) >= 1e-3)


class Draws:
    """One batch's random numbers.  frames: structured per-frame (flip, theta, scale, t[3], seed); boxes: [sum G, T, 5]
    float64 (loc x y z, rot, grot) in the order of the concatenated boxes."""

    def __init__(self, flip, theta, scale, t, seed, boxes, counts, frames=None):
        self.flip = np.asarray(flip, np.int32)
        self.theta = np.asarray(theta, np.float64)
        self.scale = np.asarray(scale, np.float64)
        self.t = np.asarray(t, np.float64).reshape(-1, 3)
        self.seed = np.asarray(seed, np.uint32)
        self.boxes = np.ascontiguousarray(boxes, np.float64)
        self.counts = np.asarray(counts, np.int32)
        self._frames = frames          # a prepared pp_aug_frame array (page-locked: Trainer.stage_gt), or None

    def __len__(self):
        return len(self.flip)

    def frame(self, b):
        g0 = int(self.counts[:b].sum())
        return {"flip": bool(self.flip[b]), "theta": float(self.theta[b]), "scale": float(self.scale[b]),
                "t": self.t[b].copy(), "seed": int(self.seed[b]), "boxes": self.boxes[g0:g0 + int(self.counts[b])]}

    def frames_struct(self):
        """The pp_aug_frame array of the C-ABI (double theta, scale, t[3]; int32 flip; uint32 seed)."""
        if self._frames is not None:
            return self._frames
        a = np.zeros(len(self), dtype=FRAME_DTYPE)
        a["theta"], a["scale"], a["t"], a["flip"], a["seed"] = self.theta, self.scale, self.t, self.flip, self.seed
        return a


FRAME_DTYPE = np.dtype([("theta", "<f8"), ("scale", "<f8"), ("t", "<f8", (3,)), ("flip", "<i4"), ("seed", "<u4")])


def draw(rs, gt_boxes_per_frame, cfg):
    """The random numbers of one batch, drawn from the legacy RandomState `rs` with the reference's calls in the
    reference's order, frame by frame (noise_per_object_v3_ :952-962, random_flip :891-892, global_rotation :797,
    global_scaling_v2 :884, global_translate :874-876), then one 32-bit seed for the shuffle."""
    T = cfg.num_try
    flips, thetas, scales, ts, seeds, per_box, counts = [], [], [], [], [], [], []
    for g in gt_boxes_per_frame:
        g = np.asarray(g, np.float64).reshape(-1, 7)
        M = g.shape[0]
        loc = rs.normal(scale=np.array(cfg.loc_std, dtype=np.float64), size=[M, T, 3])
        rot = rs.uniform(cfg.rot_noise[0], cfg.rot_noise[1], size=[M, T])
        grots = np.arctan2(g[:, 0], g[:, 1])
        grot = rs.uniform((cfg.grot_range[0] - grots)[..., np.newaxis], (cfg.grot_range[1] - grots)[..., np.newaxis],
                          size=[M, T])
        per_box.append(np.concatenate([loc, rot[..., None], grot[..., None]], axis=2))
        counts.append(M)
        flips.append(bool(rs.choice([False, True], replace=False, p=[0.5, 0.5])))
        thetas.append(rs.uniform(cfg.global_rot[0], cfg.global_rot[1]))
        scales.append(rs.uniform(cfg.scaling[0], cfg.scaling[1]))
        s0, s1 = cfg.global_loc_std[0], cfg.global_loc_std[1]
        ts.append([rs.normal(0, s0, 1)[0], rs.normal(0, s1, 1)[0], rs.normal(0, s0, 1)[0]])
        seeds.append(int(rs.randint(0, 2 ** 32, dtype=np.int64)))
    boxes = np.concatenate(per_box, 0) if per_box else np.zeros((0, T, 5))
    return Draws(flips, thetas, scales, ts, seeds, boxes, counts)


# ---- the shuffle: a keyed bijection on [0, n) (the device twin is aug_perm in csrc/augment.hip) ----

_M32 = np.uint64(0xFFFFFFFF)


def _mix32(x):
    x = np.asarray(x, np.uint64) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def _perm_half_bits(n):
    bits = max(1, int(n - 1).bit_length()) if n > 1 else 1
    return (bits + 1) // 2


def shuffle_perm(seed, n):
    """Output point i is input point perm[i]: a 4-round Feistel network over 2^(2h) >= n values with cycle-walking,
    keyed by the 32-bit `seed`.  All arithmetic is unsigned 32-bit."""
    n = int(n)
    if n <= 0:
        return np.zeros(0, np.int64)
    h = _perm_half_bits(n)
    mask = np.uint64((1 << h) - 1)
    keys = [_mix32(np.uint64(seed) ^ np.uint64((0x9E3779B9 * (r + 1)) & 0xFFFFFFFF)) for r in range(4)]
    x = np.arange(n, dtype=np.uint64)
    todo = np.ones(n, bool)
    while todo.any():
        v = x[todo]
        left, right = v >> np.uint64(h), v & mask
        for k in keys:
            left, right = right, left ^ (_mix32(right ^ k) & mask)
        x[todo] = (left << np.uint64(h)) | right
        todo = x >= np.uint64(n)
    return x.astype(np.int64)


# ---- host float64 restatement of the stages ----

_NORM2 = np.array([[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]])
_NORM3 = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]],
                  np.float64) - np.array([0.5, 0.5, 0.0])
_FACES = np.array([[0, 1, 2, 3], [7, 6, 5, 4], [0, 3, 7, 4], [1, 5, 6, 2], [0, 4, 5, 1], [3, 2, 6, 7]])


def _rot2(px, py, c, s):
    """[px, py] @ [[c, -s], [s, c]], the products summed in that order (no fused multiply-add)."""
    return px * c + py * s, px * (-s) + py * c


def box_corners_2d(x, y, w, l, yaw):
    """box2d_to_corner_jit (load_data.py:1187-1205) of (x, y, w, l, yaw) arrays -> [..., 4, 2]."""
    x, y, w, l, yaw = (np.asarray(v, np.float64)[..., None] for v in (x, y, w, l, yaw))
    rx, ry = w * _NORM2[:, 0], l * _NORM2[:, 1]
    cx, cy = _rot2(rx, ry, np.cos(yaw), np.sin(yaw))
    return np.stack([cx + x, cy + y], -1)


def _standup(c):
    return c[..., 0].min(-1), c[..., 1].min(-1), c[..., 0].max(-1), c[..., 1].max(-1)


def collide(a, b):
    """The executed box_collision_test of corners a [..., 4, 2] against b [..., 4, 2] (broadcast): standup overlap and
    a proper crossing of two edges (see the module docstring)."""
    a0x, a0y, a1x, a1y = _standup(a)
    b0x, b0y, b1x, b1y = _standup(b)
    iw = np.minimum(a1x, b1x) - np.maximum(a0x, b0x)
    ih = np.minimum(a1y, b1y) - np.maximum(a0y, b0y)
    hit = np.zeros(np.broadcast(iw, ih).shape, bool)
    for k in range(4):
        A, B = a[..., k, :], a[..., (k + 1) % 4, :]
        for m in range(4):
            C, D = b[..., m, :], b[..., (m + 1) % 4, :]
            acd = (D[..., 1] - A[..., 1]) * (C[..., 0] - A[..., 0]) > (C[..., 1] - A[..., 1]) * (D[..., 0] - A[..., 0])
            bcd = (D[..., 1] - B[..., 1]) * (C[..., 0] - B[..., 0]) > (C[..., 1] - B[..., 1]) * (D[..., 0] - B[..., 0])
            abc = (C[..., 1] - A[..., 1]) * (B[..., 0] - A[..., 0]) > (B[..., 1] - A[..., 1]) * (C[..., 0] - A[..., 0])
            abd = (D[..., 1] - A[..., 1]) * (B[..., 0] - A[..., 0]) > (B[..., 1] - A[..., 1]) * (D[..., 0] - A[..., 0])
            hit |= (acd != bcd) & (abc != abd)
    return hit & (iw > 0) & (ih > 0)


def select_noise(boxes, valid, bd, grot_per_object):
    """noise_per_box / noise_per_box_v2_ on float64 boxes [M, 7] and draws bd [M, T, 5].  Returns the selected try per
    box (-1: none) and the selected transform [M, 4] (loc x y z, rot), zero where none."""
    M = boxes.shape[0]
    sel = -np.ones(M, np.int64)
    tr = np.zeros((M, 4))
    if M == 0:
        return sel, tr
    x, y, w, l, yaw = boxes[:, 0], boxes[:, 1], boxes[:, 3], boxes[:, 4], boxes[:, 6]
    corners = box_corners_2d(x, y, w, l, yaw)
    for i in range(M):
        if not valid[i]:
            continue
        loc, rot = bd[i, :, :3], bd[i, :, 3]
        if grot_per_object:
            radius = np.sqrt(x[i] ** 2 + y[i] ** 2)
            cg = np.arctan2(x[i], y[i])
            dg = cg + bd[i, :, 4]
            dx, dy = radius * np.sin(dg), radius * np.cos(dg)
            cand = box_corners_2d(dx, dy, w[i], l[i], yaw[i] + (dg - cg))
            px, py = dx, dy
        else:
            cand = np.broadcast_to(corners[i], (len(rot), 4, 2))
            px, py = np.full(len(rot), x[i]), np.full(len(rot), y[i])
        rx, ry = cand[..., 0] - px[:, None], cand[..., 1] - py[:, None]
        c, s = np.cos(rot)[:, None], np.sin(rot)[:, None]
        rx, ry = _rot2(rx, ry, c, s)
        cand = np.stack([rx + (px + loc[:, 0])[:, None], ry + (py + loc[:, 1])[:, None]], -1)
        hit = collide(cand[:, None], corners[None])            # [T, M]
        hit[:, i] = False
        ok = np.flatnonzero(~hit.any(1))
        if len(ok):
            j = int(ok[0])
            sel[i] = j
            corners[i] = cand[j]
            tr[i, :3] = loc[j]
            tr[i, 3] = rot[j]
            if grot_per_object:
                tr[i, 0] += px[j] - x[i]
                tr[i, 1] += py[j] - y[i]
                tr[i, 3] += dg[j] - cg
    return sel, tr


def box_planes(boxes):
    """Plane equations (normal [M, 6, 3], d [M, 6]) of the 3-D boxes as center_to_corner_box3d(origin=[.5, .5, 0],
    axis=2) -> corner_to_surfaces_3d_jit -> surface_equ_3d_jit build them; a point is outside when
    p . n + d >= 0 for some face."""
    dims = boxes[:, 3:6]
    rel = dims[:, None, :] * _NORM3[None]
    c, s = np.cos(boxes[:, 6])[:, None], np.sin(boxes[:, 6])[:, None]
    rx, ry = _rot2(rel[..., 0], rel[..., 1], c, s)
    corners = np.stack([rx, ry, rel[..., 2]], -1) + boxes[:, None, :3]
    sf = corners[:, _FACES]                                    # [M, 6, 4, 3]
    v0, v1 = sf[:, :, 0] - sf[:, :, 1], sf[:, :, 1] - sf[:, :, 2]
    n = np.stack([v0[..., 1] * v1[..., 2] - v0[..., 2] * v1[..., 1],
                  v0[..., 2] * v1[..., 0] - v0[..., 0] * v1[..., 2],
                  v0[..., 0] * v1[..., 1] - v0[..., 1] * v1[..., 0]], -1)
    p0 = sf[:, :, 0]
    d = -((n[..., 0] * p0[..., 0] + n[..., 1] * p0[..., 1]) + n[..., 2] * p0[..., 2])
    return n, d


def face_sign(xyz, n, d):
    """[N, M, 6] plane values of float64 points xyz [N, 3]."""
    p = xyz[:, None, None, :]
    return ((p[..., 0] * n[..., 0] + p[..., 1] * n[..., 1]) + p[..., 2] * n[..., 2]) + d


def in_range_by_center(x, y, pc_range):
    """filter_gt_box_outside_range_by_center: points_in_convex_polygon_jit of the centre against the clockwise
    rectangle minmax_to_corner_2d(pc_range[[0, 1, 3, 4]]); a centre on the border is outside."""
    x0, y0, x1, y1 = (float(pc_range[i]) for i in (0, 1, 3, 4))
    wx, wy = x1 - x0, y1 - y0
    poly = np.array([[x0 + wx * 0.0, y0 + wy * 0.0], [x0 + wx * 0.0, y0 + wy * 1.0],
                     [x0 + wx * 1.0, y0 + wy * 1.0], [x0 + wx * 1.0, y0 + wy * 0.0]])
    keep = np.ones(np.shape(x), bool)
    for k in range(4):
        v = poly[k] - poly[k - 1]
        cross = v[1] * (poly[k, 0] - x) - v[0] * (poly[k, 1] - y)
        keep &= ~(cross >= 0)
    return keep


def augment_np(points, gt_boxes, gt_classes, valid, draws, cfg, pc_range, return_info=False):
    """Stages 1-9 of one frame in float64.  points [N, F] (xyz + features), gt_boxes [M, 7], gt_classes [M] (or None),
    valid [M] bool (or None: all valid), draws: Draws.frame(b).  Returns (points float32 [N, F], boxes float64 [K, 7],
    classes [K]) and, with return_info, a dict of the decisions (selected try, point box, flip, kept boxes)."""
    pts = np.asarray(points, np.float32)
    boxes = np.asarray(gt_boxes, np.float64).reshape(-1, 7).copy()
    M = boxes.shape[0]
    cls = np.ones(M, np.int32) if gt_classes is None else np.asarray(gt_classes, np.int32).reshape(-1)
    valid = np.ones(M, bool) if valid is None else np.asarray(valid, bool).reshape(-1)
    bd = np.asarray(draws["boxes"], np.float64).reshape(M, -1, 5) if M else np.zeros((0, 1, 5))
    sel, tr = select_noise(boxes, valid, bd, cfg.global_rot_per_object)
    xyz = pts[:, :3].astype(np.float64)
    N = xyz.shape[0]
    owner = -np.ones(N, np.int64)
    if M and N:
        n, d = box_planes(boxes)
        inside = ~(face_sign(xyz, n, d) >= 0).any(-1) & valid[None, :]
        has = inside.any(1)
        owner[has] = inside[has].argmax(1)
        j = owner[has]
        c = boxes[j, :3]
        dx, dy, dz = xyz[has, 0] - c[:, 0], xyz[has, 1] - c[:, 1], xyz[has, 2] - c[:, 2]
        rx, ry = _rot2(dx, dy, np.cos(tr[j, 3]), np.sin(tr[j, 3]))
        xyz[has] = np.stack([(rx + c[:, 0]) + tr[j, 0], (ry + c[:, 1]) + tr[j, 1], (dz + c[:, 2]) + tr[j, 2]], -1)
    boxes[valid, :3] += tr[valid, :3]
    boxes[valid, 6] += tr[valid, 3]
    stages = {"s1": (xyz.copy(), boxes.copy())}
    boxes, cls = boxes[valid], cls[valid]
    flip = bool(draws["flip"])
    if flip:
        xyz[:, 1] = -xyz[:, 1]
        boxes[:, 1] = -boxes[:, 1]
        boxes[:, 6] = -boxes[:, 6]
    stages["s3"] = (xyz.copy(), boxes.copy())
    th = float(draws["theta"])
    c, s = np.cos(th), np.sin(th)
    xyz[:, 0], xyz[:, 1] = _rot2(xyz[:, 0], xyz[:, 1], c, s)
    boxes[:, 0], boxes[:, 1] = _rot2(boxes[:, 0], boxes[:, 1], c, s)
    boxes[:, 6] += th
    stages["s4"] = (xyz.copy(), boxes.copy())
    sc = float(draws["scale"])
    xyz *= sc
    boxes[:, :6] *= sc
    stages["s5"] = (xyz.copy(), boxes.copy())
    t = np.asarray(draws["t"], np.float64)
    xyz += t
    boxes[:, :3] += t
    stages["s6"] = (xyz.copy(), boxes.copy())
    boxes[:, 6] = boxes[:, 6] - np.floor(boxes[:, 6] / (2 * np.pi) + 0.5) * (2 * np.pi)
    stages["s7"] = (None, boxes.copy())
    out = pts.copy()
    out[:, :3] = xyz.astype(np.float32)
    perm = shuffle_perm(draws["seed"], N)
    out = out[perm]
    keep = in_range_by_center(boxes[:, 0], boxes[:, 1], pc_range)
    boxes, cls = boxes[keep], cls[keep]
    if return_info:
        return out, boxes, cls, {"selected": sel, "owner": owner, "flip": flip, "keep": keep, "perm": perm,
                                "stages": stages}
    return out, boxes, cls
