"""GT-database sampling: the first step of prep_pointcloud's training branch (SURVEY section 8f, row 15 --
load_data.py:2702-2751; sample_all :1690-1921, BatchSampler / DataBaseSamplerV2 :1344-1467).

Stored objects are pasted into a frame where they fit.  Per frame, as the reference executes it:
  1. per class of sample_classes, in order: num = sample_max_nums - (frame boxes of that class); if num > 0 the class's
     BatchSampler hands out the next `num` objects (cursor: `if idx + num >= n` the tail -- possibly fewer -- then a
     reshuffle);
  2. box test: box_collision_test (augment.collide: the rule as executed) of the frame's boxes + the objects accepted
     for earlier classes + the candidates, all against all; the candidates are walked in order, one whose row has a
     hit is dropped and its row AND column cleared -- so a candidate is dropped for a frame box, an accepted earlier
     object, or any LATER candidate of its group not yet walked;
  3. point test for every survivor, in order: c = frame points inside its 3-D box (augment.box_planes); one `low` coin
     (three getrandbits, short-circuit) per survivor; accepted iff
     c < max_point_collision and (c >= min_point_collision or (hypot(x, y) < 2.5 and low)) and the object has points;
  4. accepted objects' points (stored centred; float32 += float64 centre: one rounding) in front of the frame's points,
     their boxes / classes behind the frame's, valid;
  5. a frame without boxes repeats 1-4 until something is accepted -- here at most PP_GTS_MAX_ROUNDS rounds (the
     deviation: such a frame then stays without boxes).

The database (`GtDatabase`) is built once: objects of difficulty -1 and below the per-class minimum of points removed,
one `BatchSampler` per class, whose construction shuffles (numpy) and shifts every box ONCE (`random.uniform`, Python's
generator).  Candidates and coins are drawn on the host (`draw_candidates`) for every slot and round up front; the
decisions run on the GPU (csrc/gt_sample.hip: Engine.gt_sample); `sample_all_np` is their float64 host restatement,
pinned by tests/golden/ref_gt_sample.npz, which tools/gen_golden_gtsample.py produces by running the reference's own
classes.  The point test is the custom-dataset branch's (the shipped configuration); the KITTI branch has none.
"""
import pathlib
import pickle

import numpy as np

from . import augment

PP_GTS_MAX_CAND = 32
PP_GTS_MAX_ROUNDS = 4
ACCEPTED, BOX_COLLISION, TOO_MANY_POINTS, TOO_FEW_POINTS, EMPTY_OBJECT, ROUND_NOT_USED = range(6)
STATUS_NAMES = ("accepted", "box collision", "too many points", "too few points", "empty object", "round not used")

# pp_gts_cand / pp_gt_sample_config of the C-ABI
CAND_DTYPE = np.dtype([("object", "<i4"), ("group", "<i4"), ("low", "<i4"), ("reserved", "<i4")])
CONFIG_DTYPE = np.dtype([("max_point_collision", "<i4"), ("min_point_collision", "<i4"), ("reserved", "<i4", (2,))])

# configs/train.yaml, train_input_reader
_DEFAULTS = {
    "sample_classes": ["Pedestrian"],
    "sample_max_nums": [8],
    "sampler_max_point_collision": 500,
    "sampler_min_point_collision": 1,
    "sampler_noise_x_closer": [-0.8, 0.2],
    "sampler_noise_x_farther": [-0.2, 1.5],
    "sampler_noise_x_point": 2.5,
    "sampler_noise_y": [-1.25, 1.25],
}
MIN_GT_POINTS = {"Cyclist": 5}          # DataBaseSamplerV2's hard-coded table (load_data.py:1436)


def _interval(cfg, key):
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


def _count(cfg, key):
    v = cfg.get(key, _DEFAULTS[key])
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
        raise ValueError(f"{key} must be an integer >= 0, got {v!r}")
    return int(v)


class SamplerConfig:
    """The sample_classes / sample_max_nums / sampler_* keys of train_input_reader."""

    def __init__(self, sample_classes, sample_max_nums, max_point_collision, min_point_collision, noise_x_closer,
                 noise_x_farther, noise_x_point, noise_y):
        self.sample_classes = list(sample_classes)
        self.sample_max_nums = [int(n) for n in sample_max_nums]
        self.max_point_collision = int(max_point_collision)
        self.min_point_collision = int(min_point_collision)
        self.noise_x_closer = tuple(noise_x_closer)
        self.noise_x_farther = tuple(noise_x_farther)
        self.noise_x_point = float(noise_x_point)
        self.noise_y = tuple(noise_y)

    @classmethod
    def from_input_reader(cls, cfg=None):
        """None when the reader switches sampling off (sample_classes: None, the eval reader's setting)."""
        cfg = dict(cfg or {})
        if "sample_classes" in cfg and cfg["sample_classes"] is None:
            return None
        classes = cfg.get("sample_classes", _DEFAULTS["sample_classes"])
        if isinstance(classes, str) or not all(isinstance(c, str) for c in classes) or len(classes) == 0:
            raise ValueError(f"sample_classes: expected a list of class names, got {classes!r}")
        if len(set(classes)) != len(classes):
            raise ValueError(f"sample_classes: a class is listed twice: {classes!r}")
        nums = cfg.get("sample_max_nums", _DEFAULTS["sample_max_nums"])
        try:
            nums = list(nums)
        except TypeError:
            raise ValueError(f"sample_max_nums: expected a list, got {nums!r}") from None
        if len(nums) != len(classes):
            raise ValueError(f"sample_max_nums: {len(nums)} values for {len(classes)} sample_classes")
        for n in nums:
            if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
                raise ValueError(f"sample_max_nums: counts must be integers >= 0, got {n!r}")
        if sum(int(n) for n in nums) > PP_GTS_MAX_CAND:
            raise ValueError(f"sample_max_nums: {sum(nums)} candidates per frame > {PP_GTS_MAX_CAND}")
        xp = cfg.get("sampler_noise_x_point", _DEFAULTS["sampler_noise_x_point"])
        if isinstance(xp, bool) or not isinstance(xp, (int, float, np.number)) or not np.isfinite(xp):
            raise ValueError(f"sampler_noise_x_point must be a finite number, got {xp!r}")
        return cls(classes, nums, _count(cfg, "sampler_max_point_collision"), _count(cfg, "sampler_min_point_collision"),
                   _interval(cfg, "sampler_noise_x_closer"), _interval(cfg, "sampler_noise_x_farther"), float(xp),
                   _interval(cfg, "sampler_noise_y"))

    def struct(self):
        a = np.zeros(1, CONFIG_DTYPE)
        a["max_point_collision"], a["min_point_collision"] = self.max_point_collision, self.min_point_collision
        return a


class BatchSampler:
    """The reference's BatchSampler (load_data.py:1344-1409) over the boxes of one class: np.random.shuffle of the
    indices from `rs` (a numpy RandomState), random_translate from `pyrandom` (a random.Random), then the cursor."""

    def __init__(self, boxes, cfg, rs, pyrandom):
        self.boxes = np.array(boxes, np.float64).reshape(-1, 7)
        self._rs = rs
        self.indices = np.arange(len(self.boxes))
        rs.shuffle(self.indices)
        self.idx = 0
        noise_x = (0.0, 0.0)
        for i in range(len(self.boxes)):
            x = self.boxes[i, 0]
            if x < cfg.noise_x_point:
                noise_x = cfg.noise_x_closer
            if x >= cfg.noise_x_point:
                noise_x = cfg.noise_x_farther
            self.boxes[i, 0] += 0.0 + pyrandom.uniform(noise_x[0], noise_x[1])
            self.boxes[i, 1] += 0.0 + pyrandom.uniform(cfg.noise_y[0], cfg.noise_y[1])

    def sample(self, num):
        """_sample: the next `num` indices; at the end the tail (possibly fewer), then a reshuffle."""
        if self.idx + num >= len(self.boxes):
            ret = self.indices[self.idx:].copy()
            self._rs.shuffle(self.indices)
            self.idx = 0
        else:
            ret = self.indices[self.idx:self.idx + num].copy()
            self.idx += num
        return ret


class GtDatabase:
    """infos: {class name: [object dicts]} as kitti_dbinfos_train.pkl holds them (box3d_lidar x y z w l h r, difficulty,
    num_points_in_gt); points: {class name: [float32 [n_i, F] arrays]}, parallel to infos, centred on the box.  One
    BatchSampler per class of infos, in its order, consumes `rs` / `pyrandom` as DataBaseSamplerV2 consumes the global
    generators.  The sampled classes' objects are kept flat: `boxes` [n, 7] float64 (translated), `points` [P, F]
    float32 + `offsets` [n + 1], `classes` [n] (class_ids; default 1.. in sample_classes order), `base[name]` the
    first object of a class."""

    def __init__(self, infos, points, config, rs, pyrandom, num_point_features, class_ids=None, min_points=None):
        if not isinstance(config, SamplerConfig):
            raise ValueError("config: a SamplerConfig is required")
        F = int(num_point_features)
        min_points = dict(MIN_GT_POINTS if min_points is None else min_points)
        self.config = config
        self.num_point_features = F
        self.samplers, kept_points = {}, {}
        for name, objs in infos.items():
            pts = points[name]
            if len(pts) != len(objs):
                raise ValueError(f"{name}: {len(objs)} infos but {len(pts)} point arrays")
            keep = [i for i, o in enumerate(objs) if o["difficulty"] != -1
                    and o["num_points_in_gt"] >= min_points.get(name, 0)]
            boxes = np.array([np.asarray(objs[i]["box3d_lidar"], np.float64) for i in keep], np.float64).reshape(-1, 7)
            self.samplers[name] = BatchSampler(boxes, config, rs, pyrandom)
            kept_points[name] = [pts[i] for i in keep]
        ids = dict(class_ids) if class_ids is not None else {n: i + 1 for i, n in enumerate(config.sample_classes)}
        self.base, boxes, chunks, counts, classes = {}, [], [], [], []
        n = 0
        for name in config.sample_classes:
            if name not in self.samplers or len(self.samplers[name].boxes) == 0:
                raise ValueError(f"sample_classes: the database has no {name!r} objects")
            if name not in ids:
                raise ValueError(f"class_ids: no id for sampled class {name!r}")
            self.base[name] = n
            boxes.append(self.samplers[name].boxes)
            for k, a in enumerate(kept_points[name]):
                a = np.asarray(a)
                if a.ndim != 2 or a.shape[1] != F:
                    raise ValueError(f"{name} object {k}: points must be [n, {F}], got {a.shape}")
                chunks.append(np.asarray(a, np.float32))
                counts.append(len(a))
            classes += [int(ids[name])] * len(kept_points[name])
            n += len(kept_points[name])
        self.class_ids = ids
        self.boxes = np.ascontiguousarray(np.concatenate(boxes, 0))
        self.points = np.ascontiguousarray(np.concatenate(chunks, 0) if chunks else np.zeros((0, F), np.float32))
        self.offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.classes = np.asarray(classes, np.int32)

    def __len__(self):
        return len(self.boxes)

    def object_points(self, i):
        return self.points[self.offsets[i]:self.offsets[i + 1]]

    @classmethod
    def from_reference_files(cls, info_pkl, root, custom_dataset, config, rs, pyrandom, num_point_features, **kw):
        """kitti_dbinfos_train.pkl + the per-object files it names under `root`: `.pkl` (custom dataset; the name is the
        info's path with its last three characters replaced, load_data.py:1835) or `.bin` float32 [n, F]."""
        with open(info_pkl, "rb") as f:
            infos = pickle.load(f)
        points = {}
        for name, objs in infos.items():
            points[name] = []
            for o in objs:
                path = str(pathlib.Path(root) / o["path"])
                if custom_dataset:
                    with open(path[:-3] + "pkl", "rb") as f:
                        a = np.asarray(pickle.load(f, encoding="latin1"))
                else:
                    a = np.fromfile(path, dtype=np.float32, count=-1).reshape(-1, int(num_point_features))
                if a.ndim != 2 and a.size:
                    raise ValueError(f"{name} object {o['path']!r}: points must be a 2-D array [n, F], got shape {a.shape}")
                points[name].append(a if a.ndim == 2 else a.reshape(0, int(num_point_features)))
        return cls(infos, points, config, rs, pyrandom, num_point_features, **kw)

    @classmethod
    def from_frames(cls, engine, infos, clouds, config, rs, pyrandom, num_point_features, used_classes=None,
                    bev_only=False, coors_range=None, **kw):
        """From labelled frames, without the reference's files: gt_database.create_groundtruth_database (on the GPU of
        `engine`) over the frame infos and their float32 clouds, then the constructor."""
        from . import gt_database
        infos, points = gt_database.create_groundtruth_database(engine, infos, clouds, used_classes=used_classes,
                                                                bev_only=bev_only, coors_range=coors_range)
        return cls(infos, points, config, rs, pyrandom, num_point_features, **kw)


class Candidates:
    """One batch's candidate slots: cands [B, PP_GTS_MAX_CAND] CAND_DTYPE (a frame's rounds back to back), counts
    [B, PP_GTS_MAX_ROUNDS] slots per round."""

    def __init__(self, cands, counts):
        self.cands = np.ascontiguousarray(cands, CAND_DTYPE).reshape(-1, PP_GTS_MAX_CAND)
        self.counts = np.ascontiguousarray(counts, np.int32).reshape(-1, PP_GTS_MAX_ROUNDS)
        if len(self.cands) != len(self.counts):
            raise ValueError("cands / counts: different numbers of frames")

    def __len__(self):
        return len(self.cands)


def draw_low(pyrandom):
    """low_likelyhood (load_data.py:1851): three coins, short-circuit."""
    return bool(pyrandom.getrandbits(1)) and bool(pyrandom.getrandbits(1)) and bool(pyrandom.getrandbits(1))


def draw_candidates(db, gt_classes_per_frame, pyrandom, max_rounds=PP_GTS_MAX_ROUNDS):
    """Walks the frames in order.  Per frame: one round when it has boxes, else up to max_rounds; per round the cursor
    draws of every sampled class (num = max_num - boxes of that class), then one `low` coin per slot.  (The reference
    draws a round only when the one before failed, and a coin per survivor: a seeded generator pair is not consumed
    call for call as the reference consumes it.)"""
    cfg = db.config
    if not 1 <= max_rounds <= PP_GTS_MAX_ROUNDS:
        raise ValueError(f"max_rounds must be in 1..{PP_GTS_MAX_ROUNDS}")
    B = len(gt_classes_per_frame)
    cands = np.zeros((B, PP_GTS_MAX_CAND), CAND_DTYPE)
    counts = np.zeros((B, PP_GTS_MAX_ROUNDS), np.int32)
    for b, cls in enumerate(gt_classes_per_frame):
        cls = np.asarray(cls, np.int64).reshape(-1)
        want = [int(m - np.sum(cls == db.class_ids[n])) for n, m in zip(cfg.sample_classes, cfg.sample_max_nums)]
        per_round = sum(w for w in want if w > 0)
        if per_round > PP_GTS_MAX_CAND:
            raise ValueError(f"frame {b}: {per_round} candidates per round > {PP_GTS_MAX_CAND}")
        s = 0
        for r in range(1 if len(cls) else max_rounds):
            if s + per_round > PP_GTS_MAX_CAND:
                break
            s0 = s
            for g, (name, num) in enumerate(zip(cfg.sample_classes, want)):
                if num <= 0:
                    continue
                idx = db.samplers[name].sample(num)
                cands["object"][b, s:s + len(idx)] = db.base[name] + idx
                cands["group"][b, s:s + len(idx)] = g
                s += len(idx)
            for k in range(s0, s):
                cands["low"][b, k] = int(draw_low(pyrandom))
            counts[b, r] = s - s0
    return Candidates(cands, counts)


def sample_all_np(points, gt_boxes, gt_classes, gt_valid, db, cands, cand_counts, cfg=None, return_info=False):
    """Steps 2-5 of one frame in float64.  points [N, F] float32; gt_boxes [G, 7]; gt_classes [G] or None (all 1);
    gt_valid [G] bool or None; cands [PP_GTS_MAX_CAND] CAND_DTYPE and cand_counts [PP_GTS_MAX_ROUNDS]: the frame's row
    of a Candidates.  Returns (points float32 [N + pasted, F], boxes float64 [G + K, 7], classes [G + K], valid
    [G + K]) and, with return_info, a dict: status / point_counts per slot, round_used, accepted (object indices)."""
    cfg = db.config if cfg is None else cfg
    pts = np.asarray(points, np.float32)
    boxes = np.asarray(gt_boxes, np.float64).reshape(-1, 7)
    G = len(boxes)
    cls = np.ones(G, np.int32) if gt_classes is None else np.asarray(gt_classes, np.int32).reshape(-1)
    valid = np.ones(G, bool) if gt_valid is None else np.asarray(gt_valid, bool).reshape(-1)
    cands = np.asarray(cands, CAND_DTYPE).reshape(-1)
    cc = np.asarray(cand_counts, np.int64).reshape(-1)
    status = np.full(PP_GTS_MAX_CAND, ROUND_NOT_USED, np.int32)
    pcount = np.zeros(PP_GTS_MAX_CAND, np.int32)
    xyz = pts[:, :3].astype(np.float64)
    frame_corners = augment.box_corners_2d(boxes[:, 0], boxes[:, 1], boxes[:, 3], boxes[:, 4], boxes[:, 6])
    accepted, used, s0 = [], -1, 0
    for r in range(len(cc)):
        s1 = s0 + int(cc[r])
        if used >= 0 or (G > 0 and r > 0):
            s0 = s1
            continue
        obj = cands["object"][s0:s1]
        cb = db.boxes[obj]
        cc2 = augment.box_corners_2d(cb[:, 0], cb[:, 1], cb[:, 3], cb[:, 4], cb[:, 6])
        n = s1 - s0
        hit_frame = augment.collide(cc2[:, None], frame_corners[None]).any(1) if G and n else np.zeros(n, bool)
        row = augment.collide(cc2[:, None], cc2[None]) if n else np.zeros((0, 0), bool)
        row[np.arange(n), np.arange(n)] = False
        prev = np.zeros(n, bool)                     # accepted for the round's earlier groups
        survivors = []
        i = 0
        while i < n:
            e = i + 1
            while e < n and cands["group"][s0 + e] == cands["group"][s0 + i]:
                e += 1
            alive = np.zeros(n, bool)
            alive[i:e] = True
            for k in range(i, e):
                if hit_frame[k] or (row[k] & (prev | alive)).any():
                    alive[k] = False
                    status[s0 + k] = BOX_COLLISION
                else:
                    survivors.append(k)
            prev |= alive
            i = e
        acc = []
        if survivors:
            pn, pd = augment.box_planes(cb[survivors])
            inside = ~(augment.face_sign(xyz, pn, pd) >= 0).any(-1) if len(xyz) else np.zeros((0, len(survivors)), bool)
            cnt = inside.sum(0)
        for k_th, k in enumerate(survivors):
            c = int(cnt[k_th])
            pcount[s0 + k] = c
            low = bool(cands["low"][s0 + k_th])
            o = int(obj[k])
            dist = np.sqrt(np.abs(cb[k, 0]) ** 2 + np.abs(cb[k, 1]) ** 2)
            if not c < cfg.max_point_collision:
                status[s0 + k] = TOO_MANY_POINTS
            elif not (c >= cfg.min_point_collision or (dist < 2.5 and low)):
                status[s0 + k] = TOO_FEW_POINTS
            elif db.offsets[o + 1] - db.offsets[o] <= 0:
                status[s0 + k] = EMPTY_OBJECT
            else:
                status[s0 + k] = ACCEPTED
                acc.append(o)
        if acc:
            used, accepted = r, acc
        s0 = s1
    pasted = []
    for o in accepted:
        p = db.object_points(o).copy()
        p[:, :3] += db.boxes[o, :3]                  # float32 += float64: summed in float64, rounded once
        pasted.append(p)
    out = np.concatenate(pasted + [pts], 0) if pasted else pts.copy()
    if accepted:
        boxes = np.concatenate([boxes, db.boxes[accepted]], 0)
        cls = np.concatenate([cls, db.classes[accepted]]).astype(np.int32)
        valid = np.concatenate([valid, np.ones(len(accepted), bool)])
    if return_info:
        return out, boxes, cls, valid, {"status": status, "point_counts": pcount, "round_used": used,
                                        "accepted": np.asarray(accepted, np.int64)}
    return out, boxes, cls, valid
