"""Engine: one handle of the HIP library per GPU, numpy in / numpy out.

Thin host layer over the C-ABI (include/pp_hip.h).  Owns nothing numerical:
every stage runs in libpp_hip.so on the GPU; a failing call raises
RuntimeError carrying pp_last_error().
"""
import collections
import ctypes
import dataclasses
import operator
import weakref

import numpy as np

from . import _lib
from . import soft_nms as _soft
from . import tracking as _trk
from . import sweeps as _swp
from . import costmap as _cm
from . import occupancy as _occ
from . import inflation as _infl
from . import navfn as _nav
from . import local_planner as _loc
from . import scan_match as _scan
from . import frontier as _fr
from . import object_mask as _om
from . import ground as _gr
from .anchors import build_anchor_cells, build_anchors
from .config import Derived
from .weights import check_weights

_STATUS = {1: "PP_ERR_ARG", 2: "PP_ERR_STATE", 3: "PP_ERR_HIP", 4: "PP_ERR_SHAPE", 5: "PP_ERR_UNSUPPORTED",
           6: "PP_ERR_NUMERIC", 7: "PP_ERR_INTERNAL"}
PP_ERR_NUMERIC = 6
_PRECISIONS = {"split_f16": 0, "f32": 1}
_NMS_MODES = {"standup": _lib.PP_NMS_STANDUP, "rotated": _lib.PP_NMS_ROTATED, "soft": _lib.PP_NMS_SOFT}
_CLASS_NMS = {"joint": _lib.PP_CLASS_NMS_JOINT, "per_class": _lib.PP_CLASS_NMS_PER_CLASS}


class NumericError(RuntimeError):
    """PP_ERR_NUMERIC: a frame's head maps hold a non-finite value (an activation beyond the float16 operand pieces'
    range in the default arithmetic, or a network that overflows float32).  No detections were handed out."""

DET_DTYPE = np.dtype([
    ("box3d_camera", np.float64, (7,)), ("box3d_lidar", np.float32, (7,)), ("score", np.float32),
    ("label", np.int32), ("dir_label", np.int32), ("anchor_index", np.int32), ("reserved", np.int32)],
    align=True)
assert DET_DTYPE.itemsize == ctypes.sizeof(_lib.PPDetection)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _to_struct(ctype, cfg):
    """A stage's config dataclass as its ctypes mirror, by the struct's field types: an array field is filled element by
    element, an integer field takes the value's index (a bool counts, a float does not), the rest as they are."""
    pc, vals = ctype(), cfg.to_dict()
    for name, typ in ctype._fields_:
        if name not in vals:
            continue                                   # (a reserved word of the struct)
        if issubclass(typ, ctypes.Array):
            getattr(pc, name)[:] = vals[name]
        else:
            setattr(pc, name, operator.index(vals[name]) if typ is ctypes.c_int32 else vals[name])
    return pc


def _from_struct(cls, pc):
    """... and back: the dataclass `cls` from the struct the library filled (an array field as a tuple)."""
    vals = {f.name: getattr(pc, f.name) for f in dataclasses.fields(cls)}
    return cls(**{k: tuple(v) if isinstance(v, ctypes.Array) else v for k, v in vals.items()})


class Staging:
    """A page-locked host buffer (pp_host_alloc) viewed as a flat float32 numpy array."""

    def __init__(self, lib, nbytes):
        self._lib = lib
        p = ctypes.c_void_p()
        st = lib.pp_host_alloc(ctypes.c_int64(nbytes), ctypes.byref(p))
        if st != 0:
            raise RuntimeError(f"pp_host_alloc({nbytes}) failed ({_STATUS.get(st, st)})")
        self._p = p
        self.array = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_float)), shape=(max(nbytes // 4, 1),))
        self.points = None
        self.offsets = None
        self._users = weakref.WeakSet()     # engines that were handed this buffer (zero-copy passes read it late)

    def close(self):
        """Frees the buffer -- after every engine that was fed from it has finished the pass that reads it (small
        batches are not copied: the pass's first kernel reads this memory over the host link)."""
        if self._p:
            for eng in list(self._users):
                if getattr(eng, "_h", None):
                    eng.sync()
            self._users.clear()
            self.array = self.points = None
            self._lib.pp_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PinnedArray:
    """A page-locked host buffer (pp_host_alloc) viewed as a numpy array of the given shape / dtype: what a data
    loader fills in place so that the host-to-device copy of a training batch's targets is one DMA, not a staged
    pageable copy."""

    def __init__(self, lib, shape, dtype):
        self._lib = lib
        dt = np.dtype(dtype)
        n = int(np.prod(shape))
        p = ctypes.c_void_p()
        st = lib.pp_host_alloc(ctypes.c_int64(max(n * dt.itemsize, 4)), ctypes.byref(p))
        if st != 0:
            raise RuntimeError(f"pp_host_alloc({n * dt.itemsize}) failed ({_STATUS.get(st, st)})")
        self._p = p
        raw = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(max(n * dt.itemsize, 4),))
        self.array = raw[:n * dt.itemsize].view(dt).reshape(shape)

    def close(self):
        if self._p:
            self.array = None
            self._lib.pp_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MessageStaging:
    """The bytes of a batch of sensor_msgs/PointCloud2 messages in one page-locked buffer, with their layouts: what
    `Engine.ingest_pointcloud2_async` takes.  `.bytes` (uint8) may be refilled in place between uses by messages of the
    same layouts; `.byte_offsets` [batch + 1]; `.layouts`: the ctypes array of pp_pc2_layout.  features (a list of
    `ingest.FeatureField`s, or None): resolved against every message's fields here and kept -- `.features`, the ctypes array
    of pp_pc2_feature [batch][nfeat], and `.nfeat`; the ingest then writes rows of 3 + nfeat floats."""

    _records = "fields"             # the public attribute that holds the staged tuples without their data (tuples())

    def __init__(self, lib, msgs, features=None):
        from . import ingest
        tuples = [ingest.as_tuple(m) for m in msgs]
        self.byte_offsets, self.layouts, bufs = _pack_messages(tuples)
        self.fields = [t[1:] for t in tuples]       # what a later features= is resolved against (the bytes stay in .bytes)
        self.features, self.nfeat = _feature_table(tuples, None if features is None else ingest.rig_features(features, len(tuples)))
        self._fill(lib, bufs)

    def _fill(self, lib, bufs):
        self._pinned = PinnedArray(lib, (max(int(self.byte_offsets[-1]), 4),), np.uint8)
        self.bytes = self._pinned.array
        for b, buf in enumerate(bufs):
            self.bytes[self.byte_offsets[b]:self.byte_offsets[b] + buf.size] = buf
        self._users = weakref.WeakSet()

    def tuples(self):
        """The staged records as the tuples they were packed from (`ingest.as_tuple` / `ingest.image_as_tuple`), their
        data the pinned bytes as they are now."""
        return [(self.bytes[self.byte_offsets[b]:self.byte_offsets[b + 1]],) + tuple(g) for b, g in enumerate(getattr(self, self._records))]

    def close(self):
        """Frees the buffer after every engine that was fed from it has finished the pass that reads it.  As with
        Staging.close, that wait covers the engine's main stream: an ingest_pointcloud2_async with no detect_async behind
        it is not waited for -- consume (or ingest_info()) what was fed before closing."""
        if self._pinned is not None:
            for eng in list(self._users):
                if getattr(eng, "_h", None):
                    eng.sync()
            self._users.clear()
            self.bytes = None
            self._pinned.close()
            self._pinned = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DepthStaging(MessageStaging):
    """The bytes of a batch of depth images (sensor_msgs/Image, 16UC1 / mono16 / 32FC1) in one page-locked buffer: what
    `Engine.ingest_depth_async` takes.  `.bytes` may be refilled in place between uses by images of the same geometry;
    `.images`: their (width, height, step, encoding, is_bigendian).  The intrinsics are given with each ingest, so
    there is no `.layouts`."""

    _records = "images"

    def __init__(self, lib, images):
        from . import ingest
        tuples = [ingest.image_as_tuple(m) for m in images]
        self.byte_offsets, bufs = _pack_images(tuples)
        self.images = [t[1:] for t in tuples]
        self.layouts = None
        self._fill(lib, bufs)


def _pack(tuples, nbytes):
    """Records (data first) -> (byte_offsets [B + 1] int64, their byte views cut to nbytes[b])."""
    offs = np.zeros((len(tuples) + 1,), np.int64)
    bufs = []
    for b, t in enumerate(tuples):
        bufs.append(np.frombuffer(t[0], dtype=np.uint8)[:nbytes[b]])
        offs[b + 1] = offs[b] + bufs[b].size
    return offs, bufs


def _concat(bufs, offs):
    """The records' bytes as one array for a synchronous call (a single record: its own view; nothing: one zero byte)."""
    return (bufs[0] if len(bufs) == 1 else np.concatenate(bufs)) if bufs and offs[-1] else np.zeros((1,), np.uint8)


def _fill_layouts(ctype, keys, lays):
    """The ctypes array of `ctype` (pp_pc2_layout / pp_depth_layout) of a call's records from their layout dicts."""
    arr = (ctype * max(len(lays), 1))()
    for b, lay in enumerate(lays):
        for k in keys:
            setattr(arr[b], k, lay[k])
    return arr


def _pack_images(tuples):
    """[(data, width, height, step, encoding, is_bigendian)] -> (byte_offsets [B + 1] int64, the images' byte views cut to
    height * step)."""
    return _pack(tuples, [t[2] * t[3] for t in tuples])


def _pack_messages(tuples):
    """[(data, width, height, point_step, row_step, fields, is_bigendian)] -> (byte_offsets [B + 1] int64, ctypes array
    of pp_pc2_layout, the messages' byte views cut to height * row_step)."""
    from . import ingest
    lays = [ingest.layout_of(t) for t in tuples]
    offs, bufs = _pack(tuples, [lay["height"] * lay["row_step"] for lay in lays])
    return offs, _fill_layouts(_lib.PPPc2Layout, ingest.LAYOUT_KEYS, lays), bufs


def _depth_layouts(tuples, intrinsics, depth_scale, z_min, z_max):
    """The ctypes array of pp_depth_layout of a batch of images.  intrinsics: one set for the batch (anything
    `ingest.intrinsics_of` takes), or a list with one set per frame."""
    from . import ingest
    per_frame = isinstance(intrinsics, list) and not (len(intrinsics) in (4, 9) and all(np.ndim(v) == 0 for v in intrinsics))
    if per_frame and len(intrinsics) != len(tuples):
        raise ValueError(f"{len(intrinsics)} sets of intrinsics for {len(tuples)} images")
    return _fill_layouts(_lib.PPDepthLayout, ingest.DEPTH_LAYOUT_KEYS,
                         [ingest.depth_layout_of(t, intrinsics[b] if per_frame else intrinsics, depth_scale, z_min, z_max)
                          for b, t in enumerate(tuples)])


def _rig_depth_layouts(tuples, rig):
    """The ctypes array of pp_depth_layout of a rig call's images (frames back to back, a frame's cameras in rig order)."""
    from . import ingest
    n = len(rig)
    if any(k is None for k in rig.intrinsics):
        raise ValueError("a rig of depth cameras needs intrinsics (CameraRig(mounts, intrinsics=...))")
    return _fill_layouts(_lib.PPDepthLayout, ingest.DEPTH_LAYOUT_KEYS,
                         [ingest.depth_layout_of(t, rig.intrinsics[s % n], rig.depth_scale[s % n], rig.z_min[s % n], rig.z_max[s % n])
                          for s, t in enumerate(tuples)])


def _fill_config(c, first, decimate, r, r2, lift):
    """One pp_ingest_config: the selection, the two 3 x 3 matrices and the three lift terms."""
    c.first, c.decimate = int(first), int(decimate)
    c.r[:] = np.asarray(r, np.float64).reshape(-1).tolist()
    c.r2[:] = np.asarray(r2, np.float64).reshape(-1).tolist()
    c.lift[:] = [float(v) for v in lift]
    return c


def _ingest_config(first, decimate, lift, mount=None):
    """pp_ingest_config of a plain call.  mount None: the reference's RealSense matrices and [0, 0, lift] (lift None: the
    sensor height); else the `ingest.Mount`'s own r, r2 and lift (a lidar: Mount(np.eye(3), np.eye(3), 0.0))."""
    from . import ingest
    if mount is None:
        return _fill_config(_lib.PPIngestConfig(), first, decimate, *ingest._matrices(),
                            [0.0, 0.0, ingest.SENSOR_HEIGHT if lift is None else lift])
    if not isinstance(mount, ingest.Mount):
        raise ValueError("mount must be an ingest.Mount (Mount.realsense(), Mount.from_matrix(T), Mount(r, r2, lift))")
    if lift is not None:
        raise ValueError("lift and mount are both given: the mount carries its own lift")
    return _fill_config(_lib.PPIngestConfig(), first, decimate, mount.r, mount.r2, mount.lift)


def _rig_configs(rig, batch):
    """The ctypes array of pp_ingest_config of a rig call: one per source, the rig's cameras repeated for every frame."""
    n = len(rig)
    cfgs = (_lib.PPIngestConfig * (n * batch))()
    for s in range(n * batch):
        m = rig.mounts[s % n]
        _fill_config(cfgs[s], rig.first[s % n], rig.decimate[s % n], m.r, m.r2, m.lift)
    return cfgs


def _feature_table(tuples, per_message):
    """The ctypes array of pp_pc2_feature [len(tuples)][nfeat] of a _fields call and nfeat.  per_message: one list of
    `ingest.FeatureField`s per message (each resolved against its own message: `ingest.feature_layout_of`), or None ->
    (None, None): the call that delivers x y z only."""
    from . import ingest
    if per_message is None:
        return None, None
    rows = [ingest.feature_layout_of(t, f) for t, f in zip(tuples, per_message)]
    nf = len(rows[0]) if rows else 0
    if any(len(r) != nf for r in rows):
        raise ValueError(f"the messages' feature lists differ in length: {sorted({len(r) for r in rows})}")
    arr = (_lib.PPPc2Feature * max(len(rows) * nf, 1))()
    for b, row in enumerate(rows):
        for j, (off, typ, scale, bias) in enumerate(row):
            e = arr[b * nf + j]
            e.offset, e.datatype, e.scale, e.bias = int(off), int(typ), float(scale), float(bias)
    return arr, nf


def _rig_feature_table(tuples, rig, features):
    """`_feature_table` of a rig call's messages (frames back to back, a frame's cameras in rig order)."""
    from . import ingest
    if features is None:
        return None, None
    per = ingest.rig_features(features, len(rig))
    return _feature_table(tuples, [per[s % len(rig)] for s in range(len(tuples))])


def _tap_rows(tuples, first, decimate):
    """The points the parity tap of a plain call must hold: the sum of its records' `ingest.kept_bound`s (first / decimate
    held to what kept_bound takes: the library refuses such a call)."""
    from . import ingest
    first, decimate = max(int(first), 0), max(int(decimate), 1)
    return sum(ingest.kept_bound(t[1], t[2], first, decimate) for t in tuples)


def _rig_tap_rows(tuples, rig):
    """The same for a rig call's records (frames back to back, a frame's cameras in rig order)."""
    from . import ingest
    n = len(rig)
    return int(sum(ingest.kept_bound(t[1], t[2], rig.first[s % n], rig.decimate[s % n]) for s, t in enumerate(tuples)))


class RigDepthStaging(DepthStaging):
    """DepthStaging for `Engine.ingest_rig_depth_async`: the images of B frames, one per camera of a rig, frames back to
    back.  `.source_frame`: the frame of every image."""

    def __init__(self, lib, frames, rig):
        from . import ingest
        flat, self.source_frame = ingest.rig_frame_map(frames, rig, "staging_rig_depth")
        self.batch = len(frames)
        super().__init__(lib, flat)


class RigMessageStaging(MessageStaging):
    """MessageStaging for `Engine.ingest_rig_pointcloud2_async`, as RigDepthStaging.  features: `ingest.rig_features`."""

    def __init__(self, lib, frames, rig, features=None):
        from . import ingest
        flat, self.source_frame = ingest.rig_frame_map(frames, rig, "staging_rig_pointcloud2")
        self.batch = len(frames)
        super().__init__(lib, flat)
        if features is not None:
            self.features, self.nfeat = _rig_feature_table([ingest.as_tuple(m) for m in flat], rig, features)


class Engine:
    """config: reference-schema dict (or a config.Derived).  max_batch /
    max_points_per_frame size the device workspaces."""

    def __init__(self, config, max_batch=None, max_points_per_frame=32768, device=0, weights=None):
        self.d = config if isinstance(config, Derived) else Derived(config)
        d = self.d
        self.max_batch = int(max_batch if max_batch is not None else d.batch_size)
        self.max_points_per_frame = int(max_points_per_frame)
        self._lib = _lib.lib()
        c = _lib.PPConfig()
        c.pc_range[:] = [float(v) for v in d.pc_range]
        c.voxel_size[:] = [float(v) for v in d.voxel_size]
        c.max_points, c.max_voxels = d.max_points, d.max_voxels
        c.num_point_features, c.pfn_filters = d.num_point_features, d.pfn_filters
        c.layer_nums[:] = d.layer_nums
        c.layer_strides[:] = d.layer_strides
        c.num_filters[:] = d.num_filters
        c.upsample_strides[:] = d.upsample_strides
        c.num_upsample_filters[:] = d.num_upsample_filters
        c.num_anchor_per_loc, c.num_class = d.num_anchor_per_loc, d.num_class
        c.nms_pre_max_size, c.nms_post_max_size = d.nms_pre_max_size, d.nms_post_max_size
        c.nms_score_threshold, c.nms_iou_threshold = d.nms_score_threshold, d.nms_iou_threshold
        thr = d.anchor_area_threshold
        c.anchor_area_threshold = float(thr) if thr is not None else -1.0
        c.max_batch, c.max_points_per_frame = self.max_batch, self.max_points_per_frame
        c.use_direction_classifier = 1 if d.use_direction_classifier else 0
        c.with_distance = 1 if d.with_distance else 0
        h = ctypes.c_void_p()
        st = self._lib.pp_create(ctypes.byref(c), int(device), ctypes.byref(h))
        if st != 0:
            msg = self._lib.pp_last_error(None)
            raise RuntimeError(f"pp_create failed ({_STATUS.get(st, st)}): {msg.decode() if msg else ''}")
        self._h = h
        self._train_targets = None      # labels / regression targets of a step in flight (train_step_async)
        self._staged = collections.deque(maxlen=2)   # Stagings of the last two upload_async calls (see there)
        self.anchors = build_anchors(d)
        self.anchor_cells = build_anchor_cells(self.anchors, d)
        self._check(self._lib.pp_set_anchors(self._h, _ptr(self.anchors), _ptr(self.anchor_cells),
                                             ctypes.c_int64(self.anchors.shape[0])), "pp_set_anchors")
        self.weights_loaded = False
        if d.use_rotate_nms:
            self.set_nms_mode("rotated")
        if d.soft_nms is not None:
            self.set_soft_nms(**d.soft_nms)
        if d.use_soft_nms:
            self.set_nms_mode("soft")
        if d.use_multi_class_nms:
            self.set_class_nms("per_class")
        self._last_stamp = np.full(self.max_batch, np.nan)      # per stream: the last time stamp a detect* was given
        self._track_ego = False                                 # set_track_ego: poses= of a detect* also go to the tracker
        if d.tracking is not None:
            self.set_tracking(d.tracking)
        self._sweep_last = np.full(self.max_batch, np.nan)      # per stream: the last stamp an accumulate_sweeps* was given
        if d.sweeps is not None:
            self.set_sweeps(d.sweeps)
        self._costmap_queued = False                            # a costmap_async whose grids costmaps() has not fetched
        self._infl_run = {}                                     # source index -> (batch, (H, W), origins [B, 2], poses [B, 3, 4] or None, resolution) of the run its last inflate_async read
        self._frontier_run = {}                                 # source index -> (batch, (H, W), origins [B, 2], resolution) of its last frontier_async
        self._navfn_run = {}                                    # source index -> (batch, (H, W), max_path, origins, resolution, poses) of its last navfn_async
        self._local_run = {}                                    # source index -> (batch, LocalPlanConfig, resolution or None, step dt or None) of its last local_plan_async
        self._local_movers_run = {}                             # source index -> the MoverConfig that run used, or None
        self._local_foot_run = {}                               # source index -> (Footprint, FootprintConfig) that run used, or None
        if d.costmap is not None:
            self.set_costmap(d.costmap)
        if weights is not None:
            self.load_weights(weights)

    @staticmethod
    def det_dtype():
        return DET_DTYPE

    # ---- plumbing ----
    def _check(self, st, what):
        if st != 0:
            msg = self._lib.pp_last_error(self._h)
            cls = NumericError if st == PP_ERR_NUMERIC else RuntimeError
            raise cls(f"{what} failed ({_STATUS.get(st, st)}): {msg.decode() if msg else ''}")

    # ---- GEMM arithmetic (pp_set_gemm_precision) ----
    def set_gemm_precision(self, precision):
        """'split_f16' (default: fp32 results from two float16 pieces per operand on the 16-bit matrix pipe) or 'f32'
        (the float32 matrix instruction everywhere: float32's range, about a sixth of the matrix rate)."""
        if precision not in _PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}")
        self._check(self._lib.pp_set_gemm_precision(self._h, _PRECISIONS[precision]), "pp_set_gemm_precision")

    # ---- suppression rule of the post-process (pp_set_nms_mode) ----
    def set_nms_mode(self, mode):
        """'standup' (default: the reference's predict() rule, stand-up boxes with `+1` on metre widths), 'rotated'
        (rotate_nms_gpu's rule: rotated IoU of the decoded boxes) or 'soft' (soft_nms_jit's rule on the stand-up boxes: a
        neighbour of a selected box keeps its place with a decayed score, see set_soft_nms).  Takes effect from the next
        predict / detect; the config keys model.second.use_rotate_nms / use_soft_nms select 'rotated' / 'soft' at
        construction.  'rotated' <-> 'soft' goes through 'standup': soft re-scoring on the rotated overlap is not built."""
        if mode not in _NMS_MODES:
            raise ValueError(f"mode must be one of {sorted(_NMS_MODES)}")
        self._check(self._lib.pp_set_nms_mode(self._h, _NMS_MODES[mode]), "pp_set_nms_mode")

    # ---- parameters of the 'soft' rule (pp_set_soft_nms) ----
    def set_soft_nms(self, method=None, sigma=None, score_floor=None):
        """method 'hard' / 'linear' / 'gaussian' (default 'gaussian'), sigma of the Gaussian weight (0.5), score_floor under
        which a re-scored box is dropped (0.001): soft_nms_jit's defaults.  None leaves a value as it is.  Read by the
        'soft' mode only, from the next predict / detect; Nt is model.second.nms_iou_threshold."""
        cur = self.soft_nms
        m = _soft.method_id(cur["method"] if method is None else method)
        try:
            sg = float(cur["sigma"] if sigma is None else sigma)
            fl = float(cur["score_floor"] if score_floor is None else score_floor)
        except (TypeError, ValueError):
            raise ValueError(f"sigma and score_floor must be numbers, got {sigma!r}, {score_floor!r}")
        _soft.check_params(sg, fl)
        self._check(self._lib.pp_set_soft_nms(self._h, m, ctypes.c_float(sg), ctypes.c_float(fl)), "pp_set_soft_nms")

    @property
    def soft_nms(self):
        """{'method', 'sigma', 'score_floor'} of the 'soft' rule, as set (float32 values)."""
        m, sg, fl = ctypes.c_int32(0), ctypes.c_float(0), ctypes.c_float(0)
        self._check(self._lib.pp_get_soft_nms(self._h, ctypes.byref(m), ctypes.byref(sg), ctypes.byref(fl)), "pp_get_soft_nms")
        return {"method": {v: k for k, v in _soft.METHODS.items()}[m.value], "sigma": sg.value, "score_floor": fl.value}

    @property
    def nms_mode(self):
        v = ctypes.c_int32(0)
        self._check(self._lib.pp_get_nms_mode(self._h, ctypes.byref(v)), "pp_get_nms_mode")
        return {v_: k for k, v_ in _NMS_MODES.items()}[v.value]

    # ---- one suppression pass for all classes, or one per class (pp_set_class_nms) ----
    def set_class_nms(self, mode):
        """'joint' (default: the reference's predict() -- an anchor's score is its largest class score, one top-100 and
        one NMS serve all classes) or 'per_class' (model.second.use_multi_class_nms, which selects it at construction:
        threshold, top-100, NMS and both caps run per class on that class's score alone; a frame's detections are class
        0's kept boxes in descending score, then class 1's, ..., up to num_class * nms_post_max_size rows, and an anchor
        may appear under several labels).  Takes effect from the next predict / detect; `detection_rows` follows it, and
        the results of a pass run in the other mode can no longer be fetched."""
        if mode not in _CLASS_NMS:
            raise ValueError(f"mode must be one of {sorted(_CLASS_NMS)}")
        self._check(self._lib.pp_set_class_nms(self._h, _CLASS_NMS[mode]), "pp_set_class_nms")

    @property
    def class_nms(self):
        v = ctypes.c_int32(0)
        self._check(self._lib.pp_get_class_nms(self._h, ctypes.byref(v)), "pp_get_class_nms")
        return {v_: k for k, v_ in _CLASS_NMS.items()}[v.value]

    @property
    def detection_rows(self):
        """Rows per frame of the arrays predict / detections / detect / bboxes return in the current class mode:
        nms_post_max_size ('joint') or num_class * nms_post_max_size ('per_class')."""
        v = ctypes.c_int32(0)
        self._check(self._lib.pp_get_detection_rows(self._h, ctypes.byref(v)), "pp_get_detection_rows")
        return v.value

    # ---- image boxes of the kept detections (pp_set_projection) ----
    def set_projection(self, p2):
        """p2 [4,4] (every frame) or [B,4,4] (frame b of a pass uses matrix b), or None: off (the default).  With it on,
        the post-process also projects every kept detection's camera box into the image (projection.py states the
        rule) and `bboxes()` returns the result.  Takes effect from the next predict / detect."""
        if p2 is None:
            self._check(self._lib.pp_set_projection(self._h, None, 0), "pp_set_projection")
            return
        p = np.asarray(p2, np.float64)
        if p.ndim == 2:
            p = np.broadcast_to(p, (self.max_batch,) + p.shape)
        if p.ndim != 3 or p.shape[1:] != (4, 4):
            raise ValueError(f"p2 must be [4,4] or [B,4,4], got {np.asarray(p2).shape}")
        p = np.ascontiguousarray(p).reshape(p.shape[0], 16)
        self._check(self._lib.pp_set_projection(self._h, _ptr(p), int(p.shape[0])), "pp_set_projection")

    @property
    def projection(self):
        v = ctypes.c_int32(0)
        self._check(self._lib.pp_get_projection(self._h, ctypes.byref(v)), "pp_get_projection")
        return bool(v.value)

    def bboxes(self, batch=None):
        """[B, detection_rows, 4] float64 image boxes (min u, min v, max u, max v) of the last pass, row i of frame b
        beside detection i; rows at or beyond the frame's count are zero.  Raises when that pass ran with projection off."""
        post = self.detection_rows
        out = np.zeros((self.max_batch, post, 4), dtype=np.float64)
        self._check(self._lib.pp_get_bboxes(self._h, _ptr(out)), "pp_get_bboxes")
        return out if batch is None else out[:batch]

    # ---- tracking across frames (pp_set_tracking; tracking.py states the rule) ----
    def set_tracking(self, cfg):
        """A tracking.TrackConfig, a dict of its fields or True (the defaults): from the next detect_async every pass
        advances one track table per stream (frame b is stream b) behind its post-process, on the GPU -- `tracks()` then
        returns ids and velocities.  None: off (the default); the tables and the configuration are kept.  The config key
        model.second.tracking selects it at construction."""
        pc = None if cfg is None or cfg is False else ctypes.byref(_to_struct(_lib.PPTrackConfig, _trk.TrackConfig.from_any(cfg)))
        self._check(self._lib.pp_set_tracking(self._h, pc), "pp_set_tracking")

    def _stage_config(self, getter, ctype):
        """(on, the ctypes struct) of a stage's pp_get_* call."""
        on, pc = ctypes.c_int32(0), ctype()
        self._check(getattr(self._lib, getter)(self._h, ctypes.byref(on), ctypes.byref(pc)), getter)
        return bool(on.value), pc

    def _stage_info(self, call, keys, n):
        """A stage's int32 counts of its last run, `n` per key (waits for the run): {key: [n]}."""
        out = {k: np.zeros(max(n, 1), np.int32) for k in keys}
        self._check(getattr(self._lib, call)(self._h, *(_ptr(v) for v in out.values()), n), call)
        return {k: v[:n] for k, v in out.items()}

    def _get_tracking(self):
        return self._stage_config("pp_get_tracking", _lib.PPTrackConfig)

    @property
    def tracking_on(self):
        return self._get_tracking()[0]

    @property
    def tracking(self):
        """The TrackConfig the passes track with, or None while tracking is off."""
        on, pc = self._get_tracking()
        return _from_struct(_trk.TrackConfig, pc) if on else None

    def set_track_dt(self, dt):
        """Seconds by which the next tracked pass advances streams 0 .. len(dt) - 1 (pp_set_track_dt; queued on the
        engine's stream, consumed by that pass; a stream without a value advances by the configuration's period)."""
        d = np.ascontiguousarray(dt, np.float64).reshape(-1)
        self._check(self._lib.pp_set_track_dt(self._h, _ptr(d), int(d.shape[0])), "pp_set_track_dt")

    def _track_out(self, B):
        tr = np.zeros((max(B, 1), _lib.PP_TRACK_MAX), _trk.TRACK_DTYPE)
        return tr, np.zeros(max(B, 1), np.int32), np.zeros(max(B, 1), np.int32)

    def tracks(self, batch=None):
        """(tracks [B, 64] tracking.TRACK_DTYPE, n_tracks [B], overflow [B]) of the last tracked pass or track_update (waits
        for it): the live tracks of stream b in ascending slot order, zeros behind them.  Raises when the last pass ran
        untracked, and NumericError where `detections()` would."""
        tr, n, ov = self._track_out(self.max_batch)
        n[:] = -1                       # the call fills the streams of that pass (or track_update) only
        self._check(self._lib.pp_get_tracks(self._h, _ptr(tr), _ptr(n), _ptr(ov)), "pp_get_tracks")
        B = int(batch) if batch is not None else int(np.count_nonzero(n >= 0))
        return tr[:B], n[:B], ov[:B]

    def set_track_pose(self, poses):
        """The ego poses of the next tracked step (pp_set_track_pose): [k, 3, 4] float64 sensor-to-fixed transforms
        (sweeps.pose_from_xyyaw / pose_from_matrix) for streams 0 .. k - 1.  That step -- the next tracked pass's or
        track_update's -- first carries each posed stream's tracks from the sensor frame of its previous posed step into
        the current one, so ids survive the sensor's own motion and velocities are over ground (tracking.py states the
        rule); `tracks_fixed()` then gives its rows in the fixed frame.  Queued on the engine's stream and spent by that
        step, as set_track_dt's values are."""
        P = np.ascontiguousarray(poses, np.float64)
        if P.ndim != 3 or P.shape[1:] != (3, 4):
            raise ValueError(f"set_track_pose: poses must be [streams, 3, 4] (sensor to fixed frame, [R | t]), got {P.shape}")
        self._check(self._lib.pp_set_track_pose(self._h, _ptr(P), int(P.shape[0])), "pp_set_track_pose")

    def tracks_fixed(self, batch=None):
        """(tracks [B, 64] tracking.TRACK_DTYPE, n_tracks [B]) of the last tracked pass or track_update in the FIXED frame
        of the poses that step was given (pp_get_tracks_fixed): `tracks()`'s rows with position, velocity and yaw mapped by
        the stream's pose; n_tracks is -1 (rows zero) for a stream whose step had no pose.  Raises where `tracks()` does."""
        tr, n, _ = self._track_out(self.max_batch)
        n[:] = -2                       # the call fills the streams of that pass (or track_update) only
        self._check(self._lib.pp_get_tracks_fixed(self._h, _ptr(tr), _ptr(n)), "pp_get_tracks_fixed")
        B = int(batch) if batch is not None else int(np.count_nonzero(n >= -1))
        return tr[:B], n[:B]

    def set_track_ego(self, on):
        """on: the poses= (and stamps=) of detect, detect_pointcloud2, detect_depth, detect_rig_depth and
        detect_rig_pointcloud2 also go to the tracker (set_track_pose beside set_track_dt), and are accepted without
        set_sweeps -- they then serve the tracker alone; with sweeps configured both consume the same poses.  Off (the
        default): poses= means sweeps only, as before.  A policy of this class: the library knows nothing of it.  Needs
        tracking on."""
        if on and not self.tracking_on:
            raise ValueError("set_track_ego: tracking is off (set_tracking first)")
        self._track_ego = bool(on)

    @property
    def track_ego(self):
        return self._track_ego

    def track_update(self, dets, n_dets, dt=None, poses=None):
        """One tracking step on host-given rows (pp_track_update; the same kernel, on this engine's same tables): dets
        [batch, rows] DET_DTYPE, n_dets [batch], dt [batch] seconds or None (the period), poses as `set_track_pose` takes
        them or None.  Returns `tracks(batch)`."""
        n = _i32(np.asarray(n_dets).reshape(-1))
        d = np.ascontiguousarray(dets, DET_DTYPE)
        if d.ndim != 2 or d.shape[0] != n.shape[0]:
            raise ValueError(f"track_update: dets must be [batch, rows] with one count per frame, got {d.shape} and {n.shape}")
        t = None if dt is None else np.ascontiguousarray(dt, np.float64).reshape(-1)
        if t is not None and t.shape[0] != n.shape[0]:
            raise ValueError(f"track_update: {t.shape[0]} dt values for {n.shape[0]} streams")
        if poses is not None:
            if np.asarray(poses).ndim != 3 or not 1 <= np.asarray(poses).shape[0] <= n.shape[0]:
                raise ValueError(f"track_update: poses {np.asarray(poses).shape} for {n.shape[0]} streams")
            self.set_track_pose(poses)
        self._check(self._lib.pp_track_update(self._h, _ptr(d), _ptr(n), int(d.shape[1]), int(d.shape[0]), _ptr(t)),
                    "pp_track_update")
        return self.tracks(int(d.shape[0]))

    def track_reset(self, stream=None):
        """Frees every track of `stream` (None: of all streams); its ids start at 1 again, its overflow count, its last
        time stamp and its previous ego pose are forgotten."""
        s = -1 if stream is None else int(stream)
        self._check(self._lib.pp_track_reset(self._h, s), "pp_track_reset")
        if s < 0:
            self._last_stamp[:] = np.nan
        else:
            self._last_stamp[s] = np.nan

    def track_info(self):
        """Per stream, [max_batch] int32 each: `live` tracks, `next_id`, `overflow`."""
        live, nid, ov = (np.zeros(self.max_batch, np.int32) for _ in range(3))
        self._check(self._lib.pp_track_info(self._h, _ptr(live), _ptr(nid), _ptr(ov)), "pp_track_info")
        return {"live": live, "next_id": nid, "overflow": ov}

    def _stamps_dt(self, stamps, batch):
        """stamps of a detect*: (dt, the streams' new last stamps), or None without stamps.  Raises before anything is
        queued; `_detect_resident` commits."""
        if stamps is None:
            return None
        on, pc = self._get_tracking()
        if not on:
            raise ValueError("stamps: tracking is off (set_tracking first)")
        return _trk.stamps_to_dt(self._last_stamp, stamps, batch, pc.period)

    def set_cache_budget(self, megabytes):
        """Last-level-cache budget of a pass in MiB (pp_set_cache_budget; default 256, 0 = off): layers whose maps exceed
        it run over sub-ranges of the batch's frames.  Right for one engine in flight per GPU; set 0 when several
        engines share the GPU (their working sets evict each other)."""
        self._check(self._lib.pp_set_cache_budget(self._h, int(megabytes)), "pp_set_cache_budget")

    def gemm_precision(self):
        v = ctypes.c_int32(0)
        self._check(self._lib.pp_get_gemm_precision(self._h, ctypes.byref(v)), "pp_get_gemm_precision")
        return {v_: k for k, v_ in _PRECISIONS.items()}[v.value]

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pp_destroy(self._h)      # waits for the handle's streams
            self._h = None
        if getattr(self, "_staged", None) is not None:
            self._staged.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights (net.load_weights, train.py:731-734) ----
    def load_weights(self, w):
        check_weights(self.d, w)
        for name, arr in w.items():
            a = _f32(arr)
            shape = (ctypes.c_int64 * a.ndim)(*a.shape)
            self._check(self._lib.pp_set_weight(self._h, name.encode(), _ptr(a), shape, a.ndim), f"pp_set_weight({name})")
        self._check(self._lib.pp_finalize_weights(self._h), "pp_finalize_weights")
        self.weights_loaded = True

    def publish_weights(self, params_ptr, state_ptr):
        """The detector's weights from a trainer's flat device buffers (train_layout; Trainer.params / .state), folded
        on the GPU (pp_publish_train_weights, csrc/weight_publish.hip): the bytes load_weights(trainer.weights()) would
        leave, without the trip through the host.  Runs on the engine's stream, behind a step or update enqueued there;
        returns with the weights usable.  After the first call the arrays are rewritten in place and the captured
        inference graphs survive (publish_info)."""
        self._check(self._lib.pp_publish_train_weights(self._h, ctypes.c_void_p(int(params_ptr)),
                                                       ctypes.c_void_p(int(state_ptr))), "pp_publish_train_weights")
        self.weights_loaded = True

    def publish_info(self):
        """{"publishes", "reallocations", "graph_invalidations"} of publish_weights on this engine, and
        "f32_fallback_layers": the layers of the CURRENT weights (published or loaded) on the float32 fallback."""
        s = _lib.PPPublishStats()
        self._check(self._lib.pp_publish_info(self._h, ctypes.byref(s)), "pp_publish_info")
        return {k: int(getattr(s, k)) for k, _ in _lib.PPPublishStats._fields_}

    # ---- a1 ----
    def points_to_voxel(self, points):
        d = self.d
        points = _f32(points)
        if points.ndim != 2 or points.shape[1] != d.num_point_features:
            raise ValueError(f"points must be [N,{d.num_point_features}], got {points.shape}")
        voxels = np.empty((d.max_voxels, d.max_points, d.num_point_features), dtype=np.float32)
        coors = np.empty((d.max_voxels, 3), dtype=np.int32)
        num = np.empty((d.max_voxels,), dtype=np.int32)
        P = ctypes.c_int32(0)
        self._check(self._lib.pp_points_to_voxel(self._h, _ptr(points), ctypes.c_int64(points.shape[0]),
                                                 _ptr(voxels), _ptr(coors), _ptr(num), ctypes.byref(P)),
                    "pp_points_to_voxel")
        n = P.value
        return voxels[:n].copy(), coors[:n].copy(), num[:n].copy()

    # ---- a4 ----
    def anchor_mask(self, coors4, batch):
        coors4 = _i32(coors4).reshape(-1, 4)
        mask = np.empty((batch, self.anchors.shape[0]), dtype=np.uint8)
        self._check(self._lib.pp_anchor_mask(self._h, _ptr(coors4), ctypes.c_int64(coors4.shape[0]), int(batch),
                                             _ptr(mask)), "pp_anchor_mask")
        return mask

    # ---- a5-a7, a13 ----
    def forward_voxels(self, voxels, num_points, coors4, batch, want_features=False, want_canvas=False):
        d = self.d
        voxels, num_points, coors4 = _f32(voxels), _i32(num_points), _i32(coors4)
        P = voxels.shape[0]
        if voxels.shape[1:] != (d.max_points, d.num_point_features):
            raise ValueError(f"voxels must be [P,{d.max_points},{d.num_point_features}], got {voxels.shape}")
        if num_points.shape != (P,) or coors4.shape != (P, 4):
            raise ValueError("num_points must be [P] and coors [P,4] (b,z,y,x)")
        H, W, k = d.head_h, d.head_w, d.num_anchor_per_loc
        box = np.empty((batch, H, W, k * 7), dtype=np.float32)
        cls = np.empty((batch, H, W, k * d.num_class), dtype=np.float32)
        dr = np.empty((batch, H, W, k * 2), dtype=np.float32) if d.use_direction_classifier else None
        feat = np.empty((P, d.pfn_filters), dtype=np.float32) if want_features else None
        canvas = np.empty((batch, d.ny, d.nx, d.pfn_filters), dtype=np.float32) if want_canvas else None
        self._check(self._lib.pp_forward_voxels(self._h, _ptr(voxels), _ptr(num_points), _ptr(coors4),
                                                ctypes.c_int64(P), int(batch), _ptr(box), _ptr(cls), _ptr(dr),
                                                _ptr(feat), _ptr(canvas)), "pp_forward_voxels")
        out = {"box_preds": box, "cls_preds": cls}
        if dr is not None:             # model/voxelnet.py:714: the key exists only with the direction head
            out["dir_cls_preds"] = dr
        if want_features:
            out["pillar_features"] = feat
        if want_canvas:
            out["canvas"] = canvas
        return out

    # ---- a8-a12 ----
    def predict(self, box_preds, cls_preds, dir_cls_preds, anchors_mask, rect, trv2c, p2=None):
        """p2 ([4,4] or [batch,4,4]): set_projection(p2) first -- `bboxes(batch)` then holds the image boxes."""
        batch = box_preds.shape[0]
        if p2 is not None:
            self.set_projection(np.broadcast_to(np.asarray(p2, np.float64), (batch, 4, 4)))
        post = self.detection_rows
        dets = np.zeros((batch, post), dtype=DET_DTYPE)
        n = np.zeros((batch,), dtype=np.int32)
        m = np.ascontiguousarray(anchors_mask, dtype=np.uint8).reshape(batch, -1)
        if m.shape[1] != self.anchors.shape[0]:
            raise ValueError(f"anchors_mask must be [batch,{self.anchors.shape[0]}]")
        dirp = _f32(dir_cls_preds) if self.d.use_direction_classifier else None
        self._check(self._lib.pp_predict(self._h, _ptr(_f32(box_preds)), _ptr(_f32(cls_preds)), _ptr(dirp),
                                         _ptr(m), _ptr(_f32(rect).reshape(batch, 16)), _ptr(_f32(trv2c).reshape(batch, 16)),
                                         int(batch), _ptr(dets), _ptr(n)), "pp_predict")
        return dets, n

    # ---- fused path ----
    @staticmethod
    def _pack(frames, F):
        offs = np.zeros((len(frames) + 1,), dtype=np.int32)
        for i, f in enumerate(frames):
            if f.ndim != 2 or f.shape[1] != F:
                raise ValueError(f"frame {i} must be [N,{F}], got {f.shape}")
            offs[i + 1] = offs[i] + f.shape[0]
        pts = np.concatenate([_f32(f) for f in frames], axis=0) if frames else np.zeros((0, F), np.float32)
        return np.ascontiguousarray(pts), offs

    def upload(self, frames, rect=None, trv2c=None):
        """frames: list of [N_b,F] float32 clouds -> engine's resident input buffer."""
        pts, offs = self._pack(frames, self.d.num_point_features)
        self._check(self._lib.pp_upload_points(self._h, _ptr(pts), _ptr(offs), len(frames)), "pp_upload_points")
        self._offsets = offs          # the resident frames' offsets (augment splits its output by them)
        if rect is not None:
            self.set_calib(rect, trv2c, len(frames))

    def set_calib(self, rect, trv2c, batch):
        self._check(self._lib.pp_set_calib(self._h, _ptr(_f32(rect).reshape(batch, 16)),
                                           _ptr(_f32(trv2c).reshape(batch, 16)), batch), "pp_set_calib")

    def staging(self, frames):
        """Packs frames into a page-locked staging buffer (pp_host_alloc) for upload_async.  Returns a
        Staging whose `.points` / `.offsets` may be refilled in place between uses."""
        pts, offs = self._pack(frames, self.d.num_point_features)
        st = Staging(self._lib, max(pts.nbytes, 4))
        st.points = st.array[:pts.size].reshape(pts.shape)
        st.points[...] = pts
        st.offsets = offs
        return st

    def upload_async(self, staging):
        """Queues the host-to-device copy of a Staging on the engine's stream and returns at once; the staging
        buffer must not be rewritten before the sync() that follows the detect_async() consuming it."""
        self._check(self._lib.pp_upload_points_async(self._h, _ptr(staging.points), _ptr(staging.offsets),
                                                     staging.offsets.shape[0] - 1), "pp_upload_points_async")
        self._offsets = np.array(staging.offsets, np.int64)
        # The handle's two input buffers alternate and the library waits for the pass that read a buffer before it
        # re-stages it, so the buffers of the last two uploads are the ones a pass may still read: the engine keeps
        # them alive (a temporary Staging would otherwise be freed under the zero-copy kernel).
        users = getattr(staging, "_users", None)     # (anything with .points / .offsets may be passed)
        if users is not None:
            users.add(self)
        self._staged.append(staging)

    def upload_device(self, dev_ptr, offsets, producer_stream=None):
        """dev_ptr: integer device address of concatenated [sum N, F] float32 points.  producer_stream: integer
        hipStream_t handle the points were written on (e.g. torch.cuda.current_stream().cuda_stream), or None
        if that work has already completed."""
        offs = _i32(offsets)
        ps = ctypes.c_void_p(int(producer_stream)) if producer_stream else None
        self._check(self._lib.pp_upload_points_device(self._h, ctypes.c_void_p(int(dev_ptr)), _ptr(offs),
                                                      offs.shape[0] - 1, ps), "pp_upload_points_device")
        self._offsets = offs

    def _need_host_offsets(self, what):
        """augment / gt_sample split their outputs by the resident frames' offsets, which the host knows after an upload
        only: an ingest (and a sampled training step) leaves the sizes on the device."""
        if getattr(self, "_offsets", None) is None:
            raise RuntimeError(f"{what}: the resident frames' sizes are known on the device only (they were ingested from "
                               "camera messages, or nothing was uploaded): upload frames first")

    def _batches(self):
        up, res = ctypes.c_int32(0), ctypes.c_int32(0)
        self._check(self._lib.pp_current_batch(self._h, ctypes.byref(up), ctypes.byref(res)), "pp_current_batch")
        return up.value, res.value

    def detect_async(self):
        self._check(self._lib.pp_detect_async(self._h), "pp_detect_async")

    def sync(self):
        self._check(self._lib.pp_sync(self._h), "pp_sync")

    def detections(self, out=None):
        """Results of the last detect_async (waits for it).  out: optional (dets, n) arrays to fill."""
        B, post = self._batches()[1], self.detection_rows
        if out is None:
            out = (np.zeros((max(B, 1), post), dtype=DET_DTYPE), np.zeros((max(B, 1),), dtype=np.int32))
        dets, n = out
        if dets.shape[0] < B or n.shape[0] < B:
            raise ValueError("detections(out=...): arrays smaller than the batch")
        if dets.ndim != 2 or dets.shape[1] != post:
            raise ValueError(f"detections(out=...): dets must have detection_rows = {post} rows per frame, got {dets.shape}")
        self._check(self._lib.pp_get_detections(self._h, _ptr(dets), _ptr(n)), "pp_get_detections")
        return dets, n

    def detect(self, frames, rect=None, trv2c=None, on_numeric="f32", p2=None, image_shape=None, bbox=False, stamps=None,
               poses=None):
        """upload + detect_async + sync + detections.  on_numeric: what to do when the default arithmetic reports
        activations outside the float16 pieces' range (NumericError) -- "f32": switch this engine to the float32
        matrix instruction (it stays there: `gemm_precision()`), run the still-resident frames again and return those
        results; "raise": propagate.  A network that overflows float32 itself always raises.
        p2 ([4, 4] or [B, 4, 4]) and image_shape ((height, width) or [B, 2]), both or neither: the uploaded frames are
        cropped to the camera frustum on the GPU (crop_to_image) before the pass -- once: the float32 re-run reads the
        cropped frames; rect and trv2c are then required.
        bbox=True (needs p2; image_shape only when the frames are to be cropped as well): set_projection(p2) for this
        pass -- `bboxes(len(frames))` then holds the detections' image boxes.
        stamps (tracking on): one time stamp in seconds per frame; stream b advances by the difference to its previous
        stamp (the configuration's period the first time).  A stamp that does not increase raises ValueError before
        anything is queued.  Without stamps every stream advances by the period.
        With tracking on, on_numeric="f32" does NOT run a flagged pass again: the pass has advanced the streams of its
        unflagged frames, a second run would advance them twice.  The engine switches to "f32" and the NumericError is
        raised; the flagged frames' streams did not move (their dt and their stamps are spent), the next pass runs in
        float32.
        poses ([B, 3, 4] sensor-to-fixed transforms; needs set_sweeps and stamps): accumulate_sweeps(poses, stamps) runs
        between the upload (and the crop) and the pass -- once: the float32 re-run reads the accumulated frames.  Under
        set_track_ego(True) the poses also go to the pass's tracking step (set_track_pose) and need no set_sweeps."""
        sweep, dts, ego = self._pose_args(poses, stamps, len(frames), "detect")
        if bbox and p2 is None:
            raise ValueError("detect: bbox=True needs p2 (the camera matrix the boxes are projected by)")
        if (image_shape is not None and p2 is None) or (p2 is not None and image_shape is None and not bbox):
            raise ValueError("detect: p2 and image_shape go together (both crop the frames to the image, neither does not); "
                             "p2 alone projects, with bbox=True")
        if image_shape is not None and (rect is None or trv2c is None):
            raise ValueError("detect: the frustum crop needs rect and trv2c")
        if bbox:
            self.set_projection(np.broadcast_to(np.asarray(p2, np.float64), (len(frames), 4, 4)))
        self.upload(frames, rect, trv2c)
        if image_shape is not None:
            from . import frustum
            B = len(frames)
            r4, t4, p4 = (np.broadcast_to(np.asarray(m, np.float64), (B, 4, 4)) for m in (rect, trv2c, p2))
            shp = np.broadcast_to(np.asarray(image_shape), (B, 2))
            self.crop_to_image(np.stack([frustum.frustum_planes(r4[b], t4[b], p4[b], shp[b]) for b in range(B)]))
        return self._detect_resident(on_numeric, dts, sweep, ego)

    def _detect_resident(self, on_numeric, dts=None, sweep=None, ego=None):
        if sweep is not None:         # (before the pass, and not again before the float32 re-run below)
            self.accumulate_sweeps(*sweep)
        if dts is not None:
            self.set_track_dt(dts[0])
            self._last_stamp = dts[1]
        if ego is not None:           # (set_track_ego: the pass's tracking step carries its streams under these poses)
            self.set_track_pose(ego)
        self.detect_async()
        self.sync()
        try:
            return self.detections()
        except NumericError:
            if on_numeric != "f32" or self.gemm_precision() == "f32":
                raise
            if self.tracking_on:      # the pass has stepped its unflagged streams: running it again would step them twice
                self.set_gemm_precision("f32")
                raise
        self.set_gemm_precision("f32")
        self.detect_async()
        self.sync()
        return self.detections()

    # ---- frustum crop of the resident frames (pp_frustum_crop*; frustum.py states the rule) ----
    @staticmethod
    def _crop_planes(planes):
        pl = np.ascontiguousarray(planes, np.float64)
        if pl.ndim != 3 or pl.shape[1:] != (6, 4):
            raise ValueError(f"planes must be [batch, 6, 4] (frustum.frustum_planes per frame), got {pl.shape}")
        return pl

    def crop_to_image(self, planes, back=False, return_points=False):
        """Crops the frames uploaded to this engine to their camera frustums, on the GPU (pp_frustum_crop): what the
        reference's remove_outside_points does to a KITTI cloud.  planes: [B, 6, 4] float64, frustum.frustum_planes of
        each frame's calibration; back: negate x first (the `_back` files).  The cropped frames replace the resident
        ones, as after an upload: detect_async, count_points_in_gt, build_gt_objects, augment ... see them.  Returns the
        kept counts, int32 [B]; return_points: (counts, [B float32 arrays [kept_b, F]])."""
        pl = self._crop_planes(planes)
        B, F = len(pl), self.d.num_point_features
        kept = np.zeros(max(B, 1), np.int32)
        resident = getattr(self, "_offsets", None)
        cap = int(resident[-1]) if return_points and resident is not None else 0
        pts = np.empty((max(cap, 1), F), np.float32) if return_points else None
        self._check(self._lib.pp_frustum_crop(self._h, _ptr(pl), B, _lib.PP_CROP_BACK if back else 0, _ptr(kept), _ptr(pts),
                                              ctypes.c_int64(cap)), "pp_frustum_crop")
        kept = kept[:B]
        off = np.zeros(B + 1, np.int32)
        off[1:] = np.cumsum(kept)
        self._offsets = off
        self._crop_batch = B
        if not return_points:
            return kept
        return kept, [pts[off[b]:off[b + 1]].copy() for b in range(B)]

    def crop_to_image_async(self, planes, back=False):
        """crop_to_image without waiting (pp_frustum_crop_async): on the copy stream behind an upload_async, the voxeliser
        behind it; the kept counts stay on the device (crop_info reads them back) and the engine is left as after an
        ingest: detect_async works, the calls that need the frames' sizes on the host are refused until the next upload."""
        pl = self._crop_planes(planes)
        self._check(self._lib.pp_frustum_crop_async(self._h, _ptr(pl), len(pl), _lib.PP_CROP_BACK if back else 0),
                    "pp_frustum_crop_async")
        self._offsets = None
        self._crop_batch = len(pl)

    def crop_info(self):
        """The kept counts of the last crop, int32 [B] (pp_frustum_crop_info; waits for it)."""
        return self._stage_info("pp_frustum_crop_info", ("kept",), getattr(self, "_crop_batch", 0))["kept"]

    # ---- multi-sweep accumulation (pp_set_sweeps, pp_sweeps_accumulate*; sweeps.py states the rule) ----
    def set_sweeps(self, cfg):
        """A sweeps.SweepConfig, a dict of its fields or True (the defaults): the engine keeps the last `history` sweeps of
        every stream (frame b is stream b) on the GPU and `accumulate_sweeps` carries them into the current frame.  The ring
        is allocated here; a configuration with another history or capacity forgets the streams' history.  None: off (the
        default); the ring is kept.  The config key model.second.sweeps selects it at construction."""
        if cfg is None or cfg is False:
            self._check(self._lib.pp_set_sweeps(self._h, None), "pp_set_sweeps")
            return
        c = _swp.SweepConfig.from_any(cfg).resolved(self.d.num_point_features, self.max_points_per_frame)
        pc = _to_struct(_lib.PPSweepConfig, c)
        on, old = self._get_sweeps()
        self._check(self._lib.pp_set_sweeps(self._h, ctypes.byref(pc)), "pp_set_sweeps")
        if (old.history, old.capacity) != (c.history, c.capacity):      # the ring was re-made: the stamps went with it
            self._sweep_last[:] = np.nan

    def _get_sweeps(self):
        return self._stage_config("pp_get_sweeps", _lib.PPSweepConfig)

    def sweeps(self):
        """The SweepConfig in force (capacity filled in), or None while the stage is off."""
        on, pc = self._get_sweeps()
        return _from_struct(_swp.SweepConfig, pc) if on else None

    def _sweep_call(self, poses, stamps, who):
        """What accumulate_sweeps* refuse before anything is queued; returns (poses, stamps, the streams' new stamps)."""
        if not self._get_sweeps()[0]:
            raise RuntimeError(f"{who}: sweeps are not configured (set_sweeps first)")
        B = np.asarray(poses).shape[0] if np.asarray(poses).ndim == 3 else -1
        if B > self.max_batch:
            raise ValueError(f"{who}: {B} poses, the engine has {self.max_batch} streams")
        return _swp.check_call(poses, stamps, B, self._sweep_last[:max(B, 0)])

    def accumulate_sweeps(self, poses, stamps, return_points=False):
        """Carries every stream's stored sweeps into the resident frames, on the GPU (pp_sweeps_accumulate), exactly as
        sweeps.SweepAccumulator.accumulate does on the host; then stores the original frames in the streams' rings.  poses:
        [B, 3, 4] float64 sensor-to-fixed transforms (sweeps.pose_from_xyyaw / pose_from_matrix), stamps: [B] seconds.
        Works on any resident frames, also ingested ones whose sizes only the device knows.  The accumulated frames replace
        the resident ones, as after an upload.  Returns the output frames' rows, int32 [B]; return_points: (counts, [B
        float32 arrays [count_b, F]])."""
        P, S, new_last = self._sweep_call(poses, stamps, "accumulate_sweeps")
        B, F = len(P), self.d.num_point_features
        counts = np.zeros(max(B, 1), np.int32)
        cap = B * self.max_points_per_frame if return_points else 0
        pts = np.empty((max(cap, 1), F), np.float32) if return_points else None
        self._check(self._lib.pp_sweeps_accumulate(self._h, _ptr(P), _ptr(S), B, _ptr(counts), _ptr(pts), ctypes.c_int64(cap)),
                    "pp_sweeps_accumulate")
        self._sweep_last[:B] = new_last
        counts = counts[:B]
        off = np.zeros(B + 1, np.int32)
        off[1:] = np.cumsum(counts)
        self._offsets = off
        self._sweep_batch = B
        if not return_points:
            return counts
        return counts, [pts[off[b]:off[b + 1]].copy() for b in range(B)]

    def accumulate_sweeps_async(self, poses, stamps):
        """accumulate_sweeps without waiting (pp_sweeps_accumulate_async): on the copy stream behind an upload_async, an
        asynchronous ingest or crop, the voxeliser behind it; the counts stay on the device (sweeps_info reads them back)
        and the engine is left as after an ingest."""
        P, S, new_last = self._sweep_call(poses, stamps, "accumulate_sweeps_async")
        self._check(self._lib.pp_sweeps_accumulate_async(self._h, _ptr(P), _ptr(S), len(P)), "pp_sweeps_accumulate_async")
        self._sweep_last[:len(P)] = new_last
        self._offsets = None
        self._sweep_batch = len(P)

    def sweeps_info(self):
        """Per frame of the last accumulate (waits for it), int32 [B] each: `count` output rows, `used` sweeps, rows
        `truncated` at max_points_per_frame, rows `push_truncated` at the capacity when the frame was stored."""
        return self._stage_info("pp_sweeps_info", ("count", "used", "truncated", "push_truncated"), getattr(self, "_sweep_batch", 0))

    def sweeps_reset(self, stream=None):
        """Forgets the stored sweeps and the last stamp of `stream` (None: of all streams)."""
        s = -1 if stream is None else int(stream)
        self._check(self._lib.pp_sweeps_reset(self._h, s), "pp_sweeps_reset")
        if s < 0:
            self._sweep_last[:] = np.nan
        else:
            self._sweep_last[s] = np.nan

    # ---- obstacle costmap per frame (pp_set_costmap, pp_costmap_async, pp_get_costmaps; costmap.py states the rule) ----
    def set_costmap(self, cfg):
        """A costmap.CostmapConfig, a dict of its fields or True (the defaults): `costmaps()` then turns the resident
        points and -- `objects` -- the pass's detections or the streams' tracks into one int8 grid per frame on the GPU, in
        the layout of nav_msgs/OccupancyGrid (costmap.to_occupancy_grid makes the message's dict).  None: the stage off (the
        default); its buffers are kept.  The config key model.second.costmap selects it at construction."""
        pc = None if cfg is None or cfg is False else ctypes.byref(_to_struct(_lib.PPCostmapConfig, _cm.CostmapConfig.from_any(cfg)))
        self._check(self._lib.pp_set_costmap(self._h, pc), "pp_set_costmap")

    @property
    def costmap(self):
        """The CostmapConfig in force, or None while the stage is off."""
        on, pc = self._stage_config("pp_get_costmap_config", _lib.PPCostmapConfig)
        return _from_struct(_cm.CostmapConfig, pc) if on else None

    def costmap_async(self):
        """Queues the stage on the resident frames behind whatever the engine's stream holds (pp_costmap_async) and returns
        at once: behind a detect_async it reads that pass's detections or the tables its tracking step leaves."""
        self._check(self._lib.pp_costmap_async(self._h), "pp_costmap_async")
        self._costmap_queued = True
        self._costmap_batch = self._batches()[0]
        c = self.costmap
        self._costmap_shape = (c.height, c.width)
        self._costmap_frame = (c.x_min, c.y_min, c.resolution)  # (of this run: set_costmap may give another before inflate_async)

    def costmaps(self, batch=None, counts=False):
        """The grids int8 [B, H, W] of the resident frames (waits for them): of the costmap_async still unfetched, else the
        stage is queued here first.  counts=True: (grids, counts int32 [B, H, W]), the points counted per cell.  Raises
        NumericError where `detections()` would (objects = detections; the grids are written all the same)."""
        if not self._costmap_queued:
            self.costmap_async()
        self._costmap_queued = False
        B = int(batch) if batch is not None else self._costmap_batch
        H, W = self._costmap_shape
        grid = np.zeros((max(B, 1), H, W), np.int8)
        cnt = np.zeros((max(B, 1), H, W), np.int32) if counts else None
        self._check(self._lib.pp_get_costmaps(self._h, _ptr(grid), _ptr(cnt), B), "pp_get_costmaps")
        return (grid[:B], cnt[:B]) if counts else grid[:B]

    def costmap_info(self, classes=False):
        """Per frame of the last costmap run (waits for it), int32 [B] each: `points_in_grid`, `footprints`.  classes=True:
        a third key, `classes`, True when the ground stage's classes stood in the place of the z band in that run."""
        info = self._stage_info("pp_costmap_info", ("points_in_grid", "footprints"), getattr(self, "_costmap_batch", 0))
        if classes:
            info["classes"] = self._ground_used("costmap")
        return info

    # ---- rolling occupancy map per stream (pp_set_occupancy, pp_occupancy_update_async, pp_get_occupancy; occupancy.py states the rule) ----
    def set_occupancy(self, cfg):
        """An occupancy.OccupancyConfig, a dict of its fields or True (the defaults): the engine keeps one rolling
        log-odds map per stream (frame b is stream b) in the fixed frame on the GPU; `occupancy_update_async(poses)`
        updates the maps from the resident frames -- hits where returns end, free space along the rays -- and
        `occupancy_maps()` fetches them as int8 grids in the layout of nav_msgs/OccupancyGrid with their origins
        (occupancy.to_occupancy_grid makes the message's dict).  A configuration with another width, height, resolution
        or log-odds field forgets every stream's map.  None: the stage off (the default); buffers and maps are kept."""
        if cfg is None or cfg is False:
            self._check(self._lib.pp_set_occupancy(self._h, None, None, 0), "pp_set_occupancy")
            return
        c = _occ.OccupancyConfig.from_any(cfg)
        pc = _to_struct(_lib.PPOccupancyConfig, c)
        table = np.ascontiguousarray(_occ.cost_table(c), np.int8)
        self._check(self._lib.pp_set_occupancy(self._h, ctypes.byref(pc), _ptr(table), len(table)), "pp_set_occupancy")

    def _get_occupancy(self):
        return self._stage_config("pp_get_occupancy_config", _lib.PPOccupancyConfig)

    @property
    def occupancy(self):
        """The OccupancyConfig in force, or None while the stage is off."""
        on, pc = self._get_occupancy()
        return _from_struct(_occ.OccupancyConfig, pc) if on else None

    def occupancy_update_async(self, poses):
        """Updates the maps of streams 0 .. B - 1 from the resident frames under poses [B, 3, 4] float64, the
        sensor-to-fixed transforms (sweeps.pose_from_xyyaw / pose_from_matrix), exactly as occupancy.OccupancyMap.update
        does on the host (pp_occupancy_update_async): queued behind whatever the engine's stream holds, returns at once.
        B must be the resident batch; the other streams' maps stay as they are.  The update reads whatever is resident:
        call it between the upload or ingest and accumulate_sweeps, whose carried rows would cast rays from the current
        sensor position."""
        if not self._get_occupancy()[0]:
            raise RuntimeError("occupancy_update_async: the occupancy stage is not configured (set_occupancy first)")
        P = np.asarray(poses)
        B = P.shape[0] if P.ndim == 3 else -1
        if B > self.max_batch:
            raise ValueError(f"occupancy_update_async: {B} poses, the engine has {self.max_batch} streams")
        P = _swp.check_poses(poses, B)
        c = self.occupancy
        cells = [_occ.window_origin(c, P[b]) for b in range(B)]
        self._check(self._lib.pp_occupancy_update_async(self._h, _ptr(P), B), "pp_occupancy_update_async")
        self._occ_batch = B
        self._occ_origins = np.array(cells, np.float64).reshape(B, 2) * c.resolution      # (pp_get_occupancy's arithmetic)
        self._occ_shape = (c.height, c.width)
        self._occ_res = c.resolution
        self._occ_poses = P.copy()                              # (local_plan_async's default poses)

    def occupancy_maps(self, batch=None, logodds=False):
        """(grids int8 [B, H, W], origins float64 [B, 2]) of the streams of the last occupancy_update_async (waits for
        it; queues nothing): origins[b] is the fixed-frame (x, y) of grid b's cell [0, 0].  logodds=True: a third value,
        the log-odds int16 [B, H, W] (0 where unknown).  A stream reset since the update reads all unknown with a NaN
        origin.  Raises when no update has run, or when `batch` is not that update's."""
        B = int(batch) if batch is not None else getattr(self, "_occ_batch", 0)
        H, W = getattr(self, "_occ_shape", (1, 1))
        grid = np.zeros((max(B, 1), H, W), np.int8)
        lo = np.zeros((max(B, 1), H, W), np.int16) if logodds else None
        org = np.zeros((max(B, 1), 2), np.float64)
        self._check(self._lib.pp_get_occupancy(self._h, _ptr(grid), _ptr(lo), _ptr(org), B), "pp_get_occupancy")
        return (grid[:B], org[:B], lo[:B]) if logodds else (grid[:B], org[:B])

    def occupancy_info(self, masked=False, classes=False):
        """Per frame of the last occupancy update (waits for it), int32 [B] each: rows `hits`, `ground`, `ignored`;
        `cells_hit`, `cells_free` (passed and not hit); `cleared`, the cells of the new window the old one did not hold.
        masked=True: a seventh key, `masked`, the rows the object mask turned from hits into masked ends.  classes=True:
        the key `classes`, True when the ground stage's classes stood in the place of the z band in that update."""
        keys = ("hits", "ground", "ignored", "cells_hit", "cells_free", "cleared")
        info = self._stage_info("pp_occupancy_info", keys, getattr(self, "_occ_batch", 0))
        if masked:
            info.update(self._stage_info("pp_occupancy_masked", ("masked",), getattr(self, "_occ_batch", 0)))
        if classes:
            info["classes"] = self._ground_used("occupancy")
        return info

    def occupancy_reset(self, stream=None):
        """Forgets the map of `stream` (None: of all streams): its next update starts from an unknown window."""
        self._check(self._lib.pp_occupancy_reset(self._h, -1 if stream is None else int(stream)), "pp_occupancy_reset")
        org = getattr(self, "_occ_origins", None)
        if org is not None:
            org[slice(None) if stream is None else slice(int(stream), int(stream) + 1)] = np.nan

    # ---- scan match in front of the occupancy update (pp_set_scan_match, pp_scan_match_async, pp_get_scan_match; scan_match.py states the rule) ----
    def set_scan_match(self, cfg):
        """A scan_match.ScanMatchConfig, a dict of its fields or True (the defaults): `scan_match_async(poses)` then matches
        the resident frames under PRIOR poses against the streams' occupancy maps as they stand (set_occupancy first), a
        brute-force search over a window of translations and headings scored on the maps' log-odds, and `localize(poses)`
        corrects the priors by it before it fuses the frames.  None: off (the default), and every launch, buffer and
        result of the other stages is what it was."""
        if cfg is None or cfg is False:
            self._check(self._lib.pp_set_scan_match(self._h, None, None, 0), "pp_set_scan_match")
            return
        c = _scan.ScanMatchConfig.from_any(cfg)
        pc = _to_struct(_lib.PPScanMatchConfig, c)
        trig = np.ascontiguousarray(_loc.trig_table(), np.int32)
        self._check(self._lib.pp_set_scan_match(self._h, ctypes.byref(pc), _ptr(trig), len(trig)), "pp_set_scan_match")

    @property
    def scan_match(self):
        """The ScanMatchConfig in force, or None while the stage is off."""
        on, pc = self._stage_config("pp_get_scan_match_config", _lib.PPScanMatchConfig)
        return _from_struct(_scan.ScanMatchConfig, pc) if on else None

    def scan_match_async(self, poses):
        """Matches the resident frames of streams 0 .. B - 1 under the priors poses [B, 3, 4] float64 against the streams'
        maps, exactly as scan_match.match_np does on the host (pp_scan_match_async): queued behind whatever the engine's
        stream holds, returns at once.  B must be the resident batch.  Neither the maps nor their windows change; a stream
        without a map gives NO_MAP."""
        c = self.scan_match
        if c is None:
            raise RuntimeError("scan_match_async: the scan match is not configured (set_scan_match first)")
        oc = self.occupancy
        if oc is None:
            raise RuntimeError("scan_match_async: the occupancy stage is not configured (set_occupancy first)")
        P = np.asarray(poses)
        B = P.shape[0] if P.ndim == 3 else -1
        if B > self.max_batch:
            raise ValueError(f"scan_match_async: {B} poses, the engine has {self.max_batch} streams")
        P = _swp.check_poses(poses, B)
        self._check(self._lib.pp_scan_match_async(self._h, _ptr(P), B), "pp_scan_match_async")
        self._scan_run = (B, c, oc, P.copy())                   # (what scan_match_poses corrects, and by what)

    def scan_match_results(self, scores=False, classes=False):
        """words int32 [B, 8] (scan_match.WORDS: status, dx, dy, dt in steps, best, prior, n_scan, ignored) of the last
        scan_match_async (waits for it); scores=True: (words, scores int32 [B, candidates]); classes=True: one more value
        at the end, True when the ground stage's classes stood in the place of the z band in that match."""
        B, c = (self._scan_run[0], self._scan_run[1]) if getattr(self, "_scan_run", None) else (0, None)
        words = np.zeros((max(B, 1), _lib.PP_SCAN_RESULT), np.int32)
        sc = np.zeros((max(B, 1), c.candidates if c else 1), np.int32) if scores else None
        self._check(self._lib.pp_get_scan_match(self._h, _ptr(words), _ptr(sc), B), "pp_get_scan_match")
        out = (words[:B], sc[:B]) if scores else (words[:B],)
        if classes:
            out = out + (self._ground_used("scan_match"),)
        return out if len(out) > 1 else out[0]

    def scan_match_poses(self):
        """The corrected poses float64 [B, 3, 4] of the last scan_match_async (waits for it): scan_match.corrected_pose of
        its words and its priors, by the configurations that call ran with."""
        return self._scan_correct(self.scan_match_results())

    def _scan_correct(self, words):
        B, c, oc, P = self._scan_run
        return np.stack([_scan.corrected_pose(P[b], words[b], oc, c) for b in range(B)])

    def localize(self, poses):
        """One frame of scan-matched mapping: scan_match_async(poses), the wait, the correction, then
        occupancy_update_async(corrected).  Returns (corrected float64 [B, 3, 4], words int32 [B, 8]).  On a stream's first
        frame there is no map yet: the prior comes back with NO_MAP and starts the map."""
        self.scan_match_async(poses)
        words = self.scan_match_results()
        corrected = self._scan_correct(words)
        self.occupancy_update_async(corrected)
        return corrected, words

    # ---- per-point object mask in front of the three readers of the rows (pp_set_object_mask, pp_object_mask_async, pp_get_object_mask; object_mask.py states the rule) ----
    def set_object_mask(self, cfg):
        """An object_mask.ObjectMaskConfig, a dict of its fields or True (the defaults): `object_mask_async()` then marks
        every resident row that lies in the BEV rectangle of a detection of the last pass or of a live track, on the GPU,
        and the stages named in `consumers` -- occupancy_update_async, scan_match_async (so localize), costmap_async --
        leave those rows out as object_mask.py states.  A named stage refuses to run without a mask of the resident
        frames.  None: off (the default), and every launch, buffer and result of the other stages is what it was."""
        pc = None if cfg is None or cfg is False else ctypes.byref(_to_struct(_lib.PPObjectMaskConfig, _om.ObjectMaskConfig.from_any(cfg)))
        self._check(self._lib.pp_set_object_mask(self._h, pc), "pp_set_object_mask")

    @property
    def object_mask_config(self):
        """The ObjectMaskConfig in force, or None while the stage is off."""
        on, pc = self._stage_config("pp_get_object_mask_config", _lib.PPObjectMaskConfig)
        return _from_struct(_om.ObjectMaskConfig, pc) if on else None

    def object_mask_async(self, poses=None, dt=None):
        """Queues the mask of the resident frames behind whatever the engine's stream holds (pp_object_mask_async) and
        returns at once.  objects = "tracks" reads the streams' tracks as the last step left them; poses [B, 3, 4] float64
        (the sensor-to-fixed transforms of the resident frames) and dt [B] seconds bring a copy of them to now -- carried
        as the tracker's next posed step would carry them, then predicted -- which is what lets the mask run in front of
        localize, before the pass of the current frame.  The tracker itself is not touched."""
        B = self._batches()[0]
        P = None
        if poses is not None:
            P = np.ascontiguousarray(poses, np.float64)
            if P.ndim != 3 or P.shape != (B, 3, 4):
                raise ValueError(f"object_mask_async: poses must be [{B}, 3, 4] (one per resident frame), got {P.shape}")
        t = None
        if dt is not None:
            t = np.ascontiguousarray(dt, np.float64).reshape(-1)
            if t.shape[0] != B:
                raise ValueError(f"object_mask_async: {t.shape[0]} dt values for {B} resident frames")
        self._check(self._lib.pp_object_mask_async(self._h, _ptr(P), _ptr(t), B), "pp_object_mask_async")

    def object_mask(self, batch=None):
        """(masks, info) of the last object_mask_async (waits for it): masks a list of B bool arrays, one flag per row of
        the frame; info a dict of int32 [B] each: `footprints`, `masked` rows, `rows`, `flagged`.  Raises when none has
        run, or when the frames it belongs to have been replaced since."""
        nb, wpf = ctypes.c_int32(0), ctypes.c_int32(0)
        self._check(self._lib.pp_object_mask_shape(self._h, ctypes.byref(nb), ctypes.byref(wpf)), "pp_object_mask_shape")
        B = int(batch) if batch is not None else int(nb.value)
        words = np.zeros((max(B, 1), max(int(wpf.value), 1)), np.uint64)
        info = np.zeros((max(B, 1), _lib.PP_OBJMASK_INFO), np.int32)
        self._check(self._lib.pp_get_object_mask(self._h, _ptr(words), _ptr(info), B), "pp_get_object_mask")
        masks = [_om.unpack_words(words[b], info[b, 2]) for b in range(B)]
        return masks, {k: info[:B, i].copy() for i, k in enumerate(_om.INFO)}

    # ---- ground plane per frame and the rows' classes in front of the same three readers (pp_set_ground, pp_ground_async, pp_get_ground; ground.py states the rule) ----
    def set_ground(self, cfg):
        """A ground.GroundConfig, a dict of its fields or True (the defaults): `ground_async()` then fits one plane
        z = a x + b y + c per resident frame by RANSAC on the GPU and classifies every row by its vertical residual, and
        the stages named in `consumers` -- occupancy_update_async, scan_match_async (so localize), costmap_async -- use
        the classes in the place of their fixed z band, as ground.py states.  A named stage refuses to run without
        classes of the resident frames.  None: off (the default), and every launch, buffer and result of the other stages
        is what it was."""
        if cfg is None or cfg is False:
            self._check(self._lib.pp_set_ground(self._h, None), "pp_set_ground")
            return
        c = _gr.GroundConfig.from_any(cfg)
        _gr.check_refine(c, self.max_points_per_frame)
        if getattr(self, "_ground_drawn", None) != (c.seed, c.hypotheses):
            self._ground_drawn, self._ground_call = (c.seed, c.hypotheses), 0      # another stream of triples: its call index starts at 0
        self._check(self._lib.pp_set_ground(self._h, ctypes.byref(_to_struct(_lib.PPGroundConfig, c))), "pp_set_ground")

    @property
    def ground_config(self):
        """The GroundConfig in force, or None while the stage is off."""
        on, pc = self._stage_config("pp_get_ground_config", _lib.PPGroundConfig)
        return _from_struct(_gr.GroundConfig, pc) if on else None

    def _ground_used(self, reader):
        """Whether the reader's last queued run took the classes in the place of its z band (pp_ground_used)."""
        bits = ctypes.c_int32(0)
        self._check(self._lib.pp_ground_used(self._h, ctypes.byref(bits)), "pp_ground_used")
        return bool(bits.value & _gr.CONSUMERS[reader])

    def ground_async(self, triples=None):
        """Queues the fit and the classes of the resident frames behind whatever the engine's stream holds
        (pp_ground_async) and returns at once.  triples: uint32 [B, K, 3], or None: ground.draw_triples(seed, call_index,
        B, K), call_index counting this engine's drawn calls under this seed and K (a set_ground that gives the same seed and K
        again does not start it over, so a caller that re-sends its configuration every cycle still draws new triples)."""
        c = self.ground_config
        if c is None:
            raise RuntimeError("ground_async: the ground stage is not configured (set_ground first)")
        B = self._batches()[0]
        if triples is None:
            t = _gr.draw_triples(c.seed, getattr(self, "_ground_call", 0), max(B, 1), c.hypotheses)
        else:
            t = np.ascontiguousarray(triples)
            if t.dtype != np.uint32 or t.shape != (B, c.hypotheses, 3):
                raise ValueError(f"ground_async: triples must be uint32 [{B}, {c.hypotheses}, 3], got {t.dtype} {t.shape}")
        self._check(self._lib.pp_ground_async(self._h, _ptr(t), B), "pp_ground_async")
        if triples is None:
            self._ground_call = getattr(self, "_ground_call", 0) + 1
        self._ground_k = c.hypotheses

    def ground(self, batch=None, bits=False, debug=False):
        """(planes float64 [B, 3] = a b c, info) of the last ground_async (waits for it); info a dict of int32 [B] each
        (ground.INFO).  bits=True: two more values, the GROUND and the OBSTACLE flags, each a list of B bool arrays, one
        flag per row.  debug=True: two more at the end, the refit's sums int64 [B, 9] (ground.SUMS) and the hypotheses'
        counts int32 [B, K].  Raises when none has run, or when the frames it belongs to have been replaced since."""
        nb, wpf = ctypes.c_int32(0), ctypes.c_int32(0)
        self._check(self._lib.pp_ground_shape(self._h, ctypes.byref(nb), ctypes.byref(wpf)), "pp_ground_shape")
        B = int(batch) if batch is not None else int(nb.value)
        n1, w1 = max(B, 1), max(int(wpf.value), 1)
        planes, info = np.zeros((n1, 3), np.float64), np.zeros((n1, _lib.PP_GROUND_INFO), np.int32)
        gw, ow = (np.zeros((n1, w1), np.uint64), np.zeros((n1, w1), np.uint64)) if bits else (None, None)
        sums = np.zeros((n1, _lib.PP_GROUND_SUMS), np.int64) if debug else None
        counts = np.zeros((n1, getattr(self, "_ground_k", 1)), np.int32) if debug else None
        self._check(self._lib.pp_get_ground(self._h, _ptr(planes), _ptr(info), _ptr(gw), _ptr(ow), _ptr(sums), _ptr(counts), B), "pp_get_ground")
        out = (planes[:B], {k: info[:B, i].copy() for i, k in enumerate(_gr.INFO)})
        if bits:
            out += ([_gr.unpack_words(gw[b], info[b, 11]) for b in range(B)], [_gr.unpack_words(ow[b], info[b, 11]) for b in range(B)])
        if debug:
            out += (sums[:B], counts[:B])
        return out

    # ---- obstacle inflation behind either grid (pp_set_inflation, pp_inflate_async, pp_get_inflated; inflation.py states the rule) ----
    @staticmethod
    def _infl_source(source):
        if source not in _infl.SOURCES:
            raise ValueError(f"inflation: source must be one of {_infl.SOURCES}, got {source!r}")
        return _infl.SOURCES.index(source)

    def set_inflation(self, cfg, source="costmap"):
        """An inflation.InflationConfig, a dict of its fields or True (the defaults) for the grids of `source`, "costmap"
        or "occupancy": `inflated_costmaps()` / `inflated_occupancy_maps()` then give that stage's grids with every
        obstacle grown by the inscribed radius and a falling cost up to the inflation radius, computed on the GPU from
        the grid where it lies; the source's own grids stay as they are.  resolution = 0.0 takes the resolution of the
        source's configuration in force (the source must be on); any other must equal it when the stage runs.  None: the
        source's inflation off (the default); its buffers are kept."""
        k = self._infl_source(source)
        if cfg is None or cfg is False:
            self._check(self._lib.pp_set_inflation(self._h, k, None, None, 0), "pp_set_inflation")
            return
        c = _infl.InflationConfig.from_any(cfg)
        if c.resolution == 0.0:
            src = self.costmap if k == 0 else self.occupancy
            if src is None:
                raise RuntimeError(f"set_inflation: resolution = 0.0 stands for the {source} stage's, and that stage is not "
                                   f"configured (set_{source} first)")
            c = dataclasses.replace(c, resolution=src.resolution)
        pc = _to_struct(_lib.PPInflationConfig, c)
        table = np.ascontiguousarray(_infl.cost_table(c), np.int8)
        self._check(self._lib.pp_set_inflation(self._h, k, ctypes.byref(pc), _ptr(table), len(table)), "pp_set_inflation")

    def inflation_config(self, source="costmap"):
        """The InflationConfig in force for `source`, or None while its inflation is off."""
        k = self._infl_source(source)
        on, pc = ctypes.c_int32(0), _lib.PPInflationConfig()
        self._check(self._lib.pp_get_inflation_config(self._h, k, ctypes.byref(on), ctypes.byref(pc)), "pp_get_inflation_config")
        return _from_struct(_infl.InflationConfig, pc) if on.value else None

    def inflate_async(self, source="costmap"):
        """Queues the inflation of the grids of the source's last run (costmap_async / occupancy_update_async) behind
        whatever the engine's stream holds (pp_inflate_async, one launch) and returns at once.  Raises when the source or
        its inflation is off, the source has not run, or its resolution is not the inflation's.  It reads the source's
        grids as they are when it runs: queue it before the next costmap_async / occupancy_update_async to inflate this
        cycle's grids; the inflated grids then stay while the source runs again, until the next inflate_async of that
        source -- and so does their frame: the call records the batch, the shape, the origins, the resolution and the
        poses of the run it inflates (for the costmap as costmap_async found them, whatever set_costmap has given
        since), and navfn_async, local_plan_async's default poses, the movers' frame and inflated_occupancy_maps read them
        from that record, not from whatever occupancy_update_async has run or set_costmap / set_occupancy has given since:
        the source may even be off by then.  The table's resolution is held to the run's as well.  A navfn_async has to follow before the next
        local_plan_async or drive: the local planner refuses a field made on the grids this call replaces
        (PP_ERR_STATE), and so does a getter that would have to roll the samples again."""
        k = self._infl_source(source)
        self._check(self._lib.pp_inflate_async(self._h, k), "pp_inflate_async")
        if k == 0:
            B = self._costmap_batch
            x_min, y_min, res = self._costmap_frame                # (of the costmap_async it read, not of the configuration in force)
            org = np.tile(np.array([[x_min, y_min]], np.float64), (B, 1))          # the sensor frame: the sensor at yaw 0
            self._infl_run[k] = (B, self._costmap_shape, org, None, res)
        else:
            B = self._occ_batch
            self._infl_run[k] = (B, self._occ_shape, self._occ_origins[:B].copy(), self._occ_poses[:B].copy(), self._occ_res)

    @staticmethod
    def _infl_batch(batch, run, who):
        if batch is not None and run > 0 and int(batch) != run:
            raise ValueError(f"{who}: the source's run has {run} grids, batch is {int(batch)}")

    def _inflated(self, k, batch, clearance):
        B0, (H, W) = self._infl_run.get(k, (0, (1, 1)))[:2]
        B = int(batch) if batch is not None else B0
        grid = np.zeros((max(B, 1), H, W), np.int8)
        d2 = np.zeros((max(B, 1), H, W), np.uint16) if clearance else None
        self._check(self._lib.pp_get_inflated(self._h, k, _ptr(grid), _ptr(d2), B), "pp_get_inflated")
        return grid[:B], (d2[:B] if clearance else None)

    def inflated_costmaps(self, batch=None, clearance=False):
        """The inflated grids int8 [B, H, W] of the resident frames (waits for them): the costmap stage is queued first if
        no costmap_async is pending, as `costmaps()` does, then the inflation; the pending run counts as fetched, so a
        `costmaps()` afterwards runs the stage again on the same frames.  clearance=True: (grids, dist2 uint16 [B, H, W]), the squared cell distance to the nearest
        obstacle (R * R + 1: none in reach).  A `batch` that is not the run's is refused before anything is queued."""
        self._infl_batch(batch, self._costmap_batch if self._costmap_queued else self._batches()[0], "inflated_costmaps")
        if not self._costmap_queued:
            self.costmap_async()
        self.inflate_async("costmap")
        self._costmap_queued = False
        grid, d2 = self._inflated(0, batch, clearance)
        return (grid, d2) if clearance else grid

    def inflated_occupancy_maps(self, batch=None, clearance=False):
        """(grids int8 [B, H, W], origins float64 [B, 2]) of the streams of the last occupancy_update_async, inflated
        (queues the inflation, waits for it); the origins are those of `occupancy_maps()`.  clearance=True: a third value,
        dist2 uint16 [B, H, W].  A stream reset since the update reads all unknown with a NaN origin.  A `batch` that is
        not the update's is refused before anything is queued."""
        self._infl_batch(batch, getattr(self, "_occ_batch", 0), "inflated_occupancy_maps")
        self.inflate_async("occupancy")
        grid, d2 = self._inflated(1, batch, clearance)
        org = self._infl_run[1][2][:len(grid)].copy()              # (of the update this inflation read)
        return (grid, org, d2) if clearance else (grid, org)

    def inflation_info(self, source="costmap"):
        """Per grid of the source's last inflation (waits for it), int32 [B] each: `lethal`, the obstacle cells, and
        `raised`, the cells the inflation changed."""
        k = self._infl_source(source)
        n = self._infl_run.get(k, (0, None))[0]
        out = {key: np.zeros(max(n, 1), np.int32) for key in ("lethal", "raised")}
        self._check(self._lib.pp_inflation_info(self._h, k, _ptr(out["lethal"]), _ptr(out["raised"]), n), "pp_inflation_info")
        return {key: v[:n] for key, v in out.items()}

    # ---- navigation function behind either inflation (pp_set_navfn, pp_navfn_async, pp_get_navfn; navfn.py states the rule) ----
    def set_navfn(self, cfg, source="costmap"):
        """A navfn.NavfnConfig, a dict of its fields or True (the defaults) for the inflated grids of `source`, "costmap" or
        "occupancy": `navfn_async(goals)` / `plan(goals)` then compute the cost-to-go field from a goal per grid and the
        path from the sensor's cell (or `starts`) on the GPU, from the inflated grid where it lies; the inflated grids
        stay as they are.  None: the source's stage off (the default); its buffers are kept."""
        k = self._infl_source(source)
        pc = None if cfg is None or cfg is False else ctypes.byref(_to_struct(_lib.PPNavfnConfig, _nav.NavfnConfig.from_any(cfg)))
        self._check(self._lib.pp_set_navfn(self._h, k, pc), "pp_set_navfn")

    def navfn_config(self, source="costmap"):
        """The NavfnConfig in force for `source`, or None while its stage is off."""
        k = self._infl_source(source)
        on, pc = ctypes.c_int32(0), _lib.PPNavfnConfig()
        self._check(self._lib.pp_get_navfn_config(self._h, k, ctypes.byref(on), ctypes.byref(pc)), "pp_get_navfn_config")
        return _from_struct(_nav.NavfnConfig, pc) if on.value else None

    def _navfn_frame(self, k, who):
        """(batch, (H, W), origins float64 [B, 2], resolution, poses [B, 3, 4] or None) of the source's last inflation:
        the grids' frame as inflate_async recorded it, whatever the source has run since."""
        if k not in self._infl_run:
            raise RuntimeError(f"{who}: no inflation has run on the {_infl.SOURCES[k]} source (inflate_async first)")
        B, shape, org, poses, res = self._infl_run[k]
        return B, shape, org.copy(), res, poses

    def _navfn_cells_async(self, k, goals, starts):
        """pp_navfn_async on cells: goals int32 [B, 2], starts int32 [B, 2] or None (no paths)."""
        g = np.ascontiguousarray(goals, np.int32)
        s = None if starts is None else np.ascontiguousarray(starts, np.int32)
        self._check(self._lib.pp_navfn_async(self._h, k, _ptr(g), _ptr(s), int(g.shape[0])), "pp_navfn_async")
        c = self.navfn_config(_infl.SOURCES[k])
        self._navfn_run[k] = (int(g.shape[0]), self._infl_run[k][1], c.max_path, None, None, None)     # (no frame in metres yet)

    def _sensor_cells(self, k, B, org, res, shape):
        """The sensor's own cell per grid, int32 [B, 2]: floor((0 - x_min) / resolution) and likewise in y for the costmap,
        (W // 2, H // 2) for the occupancy maps."""
        if k == 0:
            return _nav.goal_cells(np.zeros((B, 2)), org, res, shape)
        return np.tile(np.array([[shape[1] // 2, shape[0] // 2]], np.int32), (B, 1))

    def navfn_async(self, goals, source="costmap", starts=None):
        """Queues the field and the paths on the grids of the source's last inflation behind whatever the engine's stream
        holds (pp_navfn_async) and returns at once.  goals float64 [B, 2] (or one (x, y) for every grid), metres in the
        grids' frame: the sensor frame for the costmap, the fixed frame for the occupancy maps; they become cells through
        navfn.goal_cells with the origins and the resolution inflate_async recorded for those grids, so a goal outside a
        window is no error (goal_state 2) and a set_costmap / set_occupancy since, None included, changes nothing.  The
        run's own record holds (batch, shape, max_path, origins, resolution, poses): the getters and local_plan_async
        read it, not the configurations in force.  starts=None: the sensor's own cell -- floor((0 - x_min) / resolution) and likewise in y for the
        costmap, (W // 2, H // 2) for the occupancy maps; an array like `goals`: those points; False: no paths."""
        k = self._infl_source(source)
        B, shape, org, res, poses = self._navfn_frame(k, "navfn_async")
        G = np.asarray(goals, np.float64)
        if G.shape not in ((2,), (B, 2)):
            raise ValueError(f"navfn_async: goals must be metres [{B}, 2] (the inflation run's grids) or one (x, y), got {G.shape}")
        g = _nav.goal_cells(np.broadcast_to(G, (B, 2)), org, res, shape)
        if starts is False:
            s = None
        elif starts is None:
            s = self._sensor_cells(k, B, org, res, shape)
        else:
            S = np.asarray(starts, np.float64)
            if S.shape not in ((2,), (B, 2)):
                raise ValueError(f"navfn_async: starts must be metres [{B}, 2] or one (x, y), None or False, got {S.shape}")
            s = _nav.goal_cells(np.broadcast_to(S, (B, 2)), org, res, shape)
        self._navfn_cells_async(k, g, s)
        self._navfn_run[k] = self._navfn_run[k][:3] + (org, res, poses)

    def _navfn_last(self, k, who):
        if k not in self._navfn_run:
            raise RuntimeError(f"{who}: no navigation function has run on the {_infl.SOURCES[k]} source (navfn_async first)")
        return self._navfn_run[k]

    def navfn_fields(self, source="costmap"):
        """The fields uint32 [B, H, W] of the source's last navfn_async (waits for it, and lets the GPU finish the rounds
        still missing: always the exact field); navfn.UNREACHED where no chain of moves joins the cell to the goal."""
        k = self._infl_source(source)
        B, (H, W) = self._navfn_last(k, "navfn_fields")[:2]
        pot = np.zeros((B, H, W), np.uint32)
        self._check(self._lib.pp_get_navfn(self._h, k, _ptr(pot), None, None, B), "pp_get_navfn")
        return pot

    def navfn_paths(self, source="costmap", metres=False):
        """(paths, path_state int32 [B]) of the source's last navfn_async (waits as navfn_fields does): a list of B arrays
        int32 [n, 2] of cells (x, y), start and goal included; metres=True: float64 [n, 2], the cells' centres in the
        grids' frame (navfn.path_to_metres).  path_state as navfn.py lists it."""
        k = self._infl_source(source)
        B, _, cap, org, res, _ = self._navfn_last(k, "navfn_paths")
        paths = np.zeros((B, cap, 2), np.int32)
        n = np.zeros(B, np.int32)
        self._check(self._lib.pp_get_navfn(self._h, k, None, _ptr(paths), _ptr(n), B), "pp_get_navfn")
        state = self.navfn_info(source)["path_state"]
        out = [paths[b, :n[b]].copy() for b in range(B)]
        if metres:
            if org is None:
                raise RuntimeError("navfn_paths: the run was given cells, it has no frame in metres")
            out = [_nav.path_to_metres(p, org[b], res) for b, p in enumerate(out)]
        return out, state

    def navfn_info(self, source="costmap"):
        """Per grid of the source's last navfn_async (waits as navfn_fields does), int32 [B] each: `goal_state`,
        `path_state`, `rounds` (relaxation rounds the GPU ran) and `reached` (cells the field reaches)."""
        k = self._infl_source(source)
        n = self._navfn_run.get(k, (0,))[0]
        out = {key: np.zeros(max(n, 1), np.int32) for key in ("goal_state", "path_state", "rounds", "reached")}
        self._check(self._lib.pp_navfn_info(self._h, k, *(_ptr(v) for v in out.values()), n), "pp_navfn_info")
        return {key: v[:n] for key, v in out.items()}

    def plan(self, goals, source="costmap", starts=None):
        """(paths in metres, path_state int32 [B]) to `goals` (as navfn_async takes them).  "costmap": the costmap stage is
        queued first if no costmap_async is pending, exactly as `inflated_costmaps()` does, then the inflation, then the
        field and the paths.  "occupancy": the inflation and this stage are queued behind the caller's
        occupancy_update_async.  Only the paths travel to the host."""
        self._plan_async(goals, source, starts)
        return self.navfn_paths(source, metres=True)

    # ---- frontier clusters behind either inflation (pp_set_frontier, pp_frontier_async, pp_get_frontiers; frontier.py states the rule) ----
    def set_frontier(self, cfg, source="costmap"):
        """A frontier.FrontierConfig, a dict of its fields or True (the defaults) for the inflated grids of `source`,
        "costmap" or "occupancy": `frontier_async()` / `explore()` then find the clusters of the frontier cells -- free
        cells that touch unknown space -- and rank them as goals on the GPU, from the inflated grid where it lies; the
        inflated grids stay as they are.  None: the source's stage off (the default); its buffers are kept."""
        k = self._infl_source(source)
        pc = None if cfg is None or cfg is False else ctypes.byref(_lib.PPFrontierConfig(**_fr.FrontierConfig.from_any(cfg).to_dict()))
        self._check(self._lib.pp_set_frontier(self._h, k, pc), "pp_set_frontier")

    def frontier_config(self, source="costmap"):
        """The FrontierConfig in force for `source`, or None while its stage is off."""
        k = self._infl_source(source)
        on, pc = ctypes.c_int32(0), _lib.PPFrontierConfig()
        self._check(self._lib.pp_get_frontier_config(self._h, k, ctypes.byref(on), ctypes.byref(pc)), "pp_get_frontier_config")
        return _fr.FrontierConfig(**{f.name: getattr(pc, f.name) for f in dataclasses.fields(_fr.FrontierConfig)}) if on.value else None

    def frontier_async(self, source="costmap", refs=None):
        """Queues the frontier stage on the grids of the source's last inflation behind whatever the engine's stream holds
        (pp_frontier_async, five launches) and returns at once.  refs integer cells [B, 2] (or one (x, y)): the reference
        cell the distance D is taken from while use_field is 0; None: the sensor's own cell, as navfn_async(starts=None)
        defines it.  With use_field the field of the source's last navfn_async is read (its goal should be the robot's own
        cell).  The call records the batch, the shape, the origins and the resolution inflate_async recorded for those
        grids: `frontiers` reads that record, not the configurations in force."""
        k = self._infl_source(source)
        B, shape, org, res, _ = self._navfn_frame(k, "frontier_async")
        if refs is None:
            r = self._sensor_cells(k, B, org, res, shape)
        else:
            r = np.asarray(refs)
            if r.shape == (2,):
                r = np.broadcast_to(r, (B, 2))
            if r.shape != (B, 2) or not np.issubdtype(r.dtype, np.integer):
                raise ValueError(f"frontier_async: refs must be integer cells [{B}, 2] (the inflation run's grids) or one (x, y), got {r.dtype} {r.shape}")
        r = np.ascontiguousarray(np.clip(r, -(2 ** 31), 2 ** 31 - 1), np.int32)
        self._check(self._lib.pp_frontier_async(self._h, k, _ptr(r), B), "pp_frontier_async")
        self._frontier_run[k] = (B, shape, org, res)

    def frontiers(self, source="costmap", metres=False, labels=False):
        """(frontiers, info) of the source's last frontier_async (waits for it; under use_field the GPU first finishes the
        field's missing rounds and ranks again on the exact field).  frontiers: a list of B structured arrays, one row per
        returned frontier in rank order, with the fields x, y (the representative cell), cx, cy (the centroid cell), n,
        label and cost (D, uint64); metres=True: x, y, cx, cy are float64, the cells' centres in the grids' frame through
        the origins and the resolution of the run's own record.  info: frontier.INFO -> int32 [B].  labels=True adds the
        label arrays uint32 [B, H, W] as a third value."""
        k = self._infl_source(source)
        if k not in self._frontier_run:
            raise RuntimeError(f"frontiers: no frontier stage has run on the {_infl.SOURCES[k]} source (frontier_async first)")
        B, (H, W), org, res = self._frontier_run[k]
        words = np.zeros((B, _lib.PP_FRONTIER_MAX, 8), np.int32)
        info = np.zeros((B, _lib.PP_FRONTIER_INFO), np.int32)
        lab = np.zeros((B, H, W), np.uint32) if labels else None
        self._check(self._lib.pp_get_frontiers(self._h, k, _ptr(words), _ptr(info), _ptr(lab), B), "pp_get_frontiers")
        xy = np.float64 if metres else np.int32
        dt = np.dtype([("x", xy), ("y", xy), ("cx", xy), ("cy", xy), ("n", np.int32), ("label", np.uint32), ("cost", np.uint64)])
        out = []
        for b in range(B):
            w = words[b, :info[b, 5]]
            f = np.zeros(len(w), dt)
            rep, cen = w[:, 0:2], w[:, 2:4]
            if metres:
                rep, cen = _fr.cells_to_metres(rep, org[b], res), _fr.cells_to_metres(cen, org[b], res)
            f["x"], f["y"], f["cx"], f["cy"] = rep[:, 0], rep[:, 1], cen[:, 0], cen[:, 1]
            f["n"], f["label"] = w[:, 4], w[:, 5].view(np.uint32)
            f["cost"] = np.array(_fr.cost_of(w), np.uint64)
            out.append(f)
        d = {name: info[:, i].copy() for i, name in enumerate(_fr.INFO)}
        return (out, d, lab) if labels else (out, d)

    def explore(self, source="occupancy"):
        """The ranked exploration goals of every stream: a list of B entries, float64 [k, 2] metres (x, y) in the grids'
        frame -- the representative cells' centres, best first -- or None for a stream with no frontier.  Queues what
        `plan` queues in front of the field (the costmap stage if none is pending and the inflation, or the inflation
        behind the caller's occupancy_update_async), then, when the source's FrontierConfig has use_field set,
        navfn_async with the sensor's own cells as goals and no starts, then the frontier stage; only the goals travel to
        the host.  With use_field this USES THE SOURCE'S NAVFN SLOT: the field then holds the cost from the robot, so a
        `plan(goal)` afterwards replaces that field with the one towards `goal` (and a `frontiers()` after such a plan is
        refused until the next frontier_async)."""
        c = self.frontier_config(source)
        if c is None:
            raise RuntimeError(f"explore: the frontier stage of the {source} source is not configured (set_frontier first)")
        k = self._inflated_async(source)
        B, shape, org, res, poses = self._navfn_frame(k, "explore")
        if c.use_field:
            self._navfn_cells_async(k, self._sensor_cells(k, B, org, res, shape), None)
            self._navfn_run[k] = self._navfn_run[k][:3] + (org, res, poses)
        self.frontier_async(source)
        fr, _ = self.frontiers(source, metres=True)
        return [np.stack([f["x"], f["y"]], axis=1) if len(f) else None for f in fr]

    # ---- local planner behind either navigation function (pp_set_local_plan, pp_local_plan_async, pp_get_local_plan; local_planner.py states the rule) ----
    def set_local_planner(self, cfg, source="costmap"):
        """A local_planner.LocalPlanConfig, a dict of its fields or True (the defaults) for `source`, "costmap" or
        "occupancy": `local_plan_async(poses, windows)` / `drive(goals, velocities, limits)` then roll a window of (v, w)
        samples over the source's inflated grid and score them on its navigation function's field, on the GPU, where
        both lie; neither is written.  None: the source's stage off (the default); its buffers are kept."""
        k = self._infl_source(source)
        if cfg is None or cfg is False:
            self._check(self._lib.pp_set_local_plan(self._h, k, None, None, 0), "pp_set_local_plan")
            return
        pc = _to_struct(_lib.PPLocalPlanConfig, _loc.LocalPlanConfig.from_any(cfg))
        trig = np.ascontiguousarray(_loc.trig_table(), np.int32)
        self._check(self._lib.pp_set_local_plan(self._h, k, ctypes.byref(pc), _ptr(trig), len(trig)), "pp_set_local_plan")

    def local_planner_config(self, source="costmap"):
        """The LocalPlanConfig in force for `source`, or None while its stage is off."""
        k = self._infl_source(source)
        on, pc = ctypes.c_int32(0), _lib.PPLocalPlanConfig()
        self._check(self._lib.pp_get_local_plan_config(self._h, k, ctypes.byref(on), ctypes.byref(pc)), "pp_get_local_plan_config")
        return _from_struct(_loc.LocalPlanConfig, pc) if on.value else None

    def set_local_movers(self, cfg, source="costmap"):
        """A local_planner.MoverConfig, a dict of its fields or True (the defaults) for `source`: `local_plan_async(...,
        dt=)` / `drive` then turn the live tracks of stream b into the movers of grid b on the GPU, where the track table
        lies (set_tracking first), and test every sample, step by step, against each mover's position at that step
        (pp_set_local_movers, pp_local_plan_movers_async; local_planner.py states both rules).  The tracks are read in the
        sensor frame for "costmap" and carried into the fixed frame by the pose of the stream's last posed tracking step
        for "occupancy".  None: off (the default), and every launch and result is what it was."""
        k = self._infl_source(source)
        if cfg is None or cfg is False:
            self._check(self._lib.pp_set_local_movers(self._h, k, None), "pp_set_local_movers")
            return
        pc = _to_struct(_lib.PPLocalMoverConfig, _loc.MoverConfig.from_any(cfg))
        self._check(self._lib.pp_set_local_movers(self._h, k, ctypes.byref(pc)), "pp_set_local_movers")

    def local_movers_config(self, source="costmap"):
        """The MoverConfig in force for `source`, or None while its movers are off."""
        k = self._infl_source(source)
        on, pc = ctypes.c_int32(0), _lib.PPLocalMoverConfig()
        self._check(self._lib.pp_get_local_movers_config(self._h, k, ctypes.byref(on), ctypes.byref(pc)), "pp_get_local_movers_config")
        return _from_struct(_loc.MoverConfig, pc) if on.value else None

    def set_local_footprint(self, footprint, cfg=True, source="costmap"):
        """A local_planner.Footprint (or its probes, integers [P, 2]) for `source`, with cfg a local_planner.FootprintConfig,
        a dict of its fields or True (the defaults): `local_plan_async` / `drive` then roll the robot as that oriented
        polygon instead of a point -- every sample's probes are tested on the inflated grid at every step, in the rollout
        kernel, with or without movers (pp_set_local_footprint; local_planner.py states the rule).  Inflate by
        `footprint.inscribed_radius()`.  None: off (the default), and every launch and result is what it was.  A new
        footprint replaces the table a last run with a footprint read: fetch that run's results first."""
        k = self._infl_source(source)
        if footprint is None or footprint is False:
            self._check(self._lib.pp_set_local_footprint(self._h, k, None, None, 0), "pp_set_local_footprint")
            return
        fp, fc = _loc._foot_args(footprint, cfg, "set_local_footprint")
        pc = _to_struct(_lib.PPLocalFootprintConfig, fc)
        P = np.ascontiguousarray(fp, np.int32)
        self._check(self._lib.pp_set_local_footprint(self._h, k, ctypes.byref(pc), _ptr(P), len(P)), "pp_set_local_footprint")
        if self._local_foot_run.get(k) is not None:
            self._local_run.pop(k, None)

    def local_footprint_config(self, source="costmap"):
        """(Footprint, FootprintConfig) in force for `source`, or None while its footprint is off."""
        k = self._infl_source(source)
        on, n, pc = ctypes.c_int32(0), ctypes.c_int32(0), _lib.PPLocalFootprintConfig()
        P = np.zeros((_lib.PP_LOCAL_MAX_PROBES, 2), np.int32)
        self._check(self._lib.pp_get_local_footprint_config(self._h, k, ctypes.byref(on), ctypes.byref(pc), _ptr(P), ctypes.byref(n)),
                    "pp_get_local_footprint_config")
        if not on.value:
            return None
        return _loc.Footprint(P[:n.value]), _loc.FootprintConfig(foot_lethal=int(pc.foot_lethal))

    def local_footprint(self, source="costmap"):
        """`n_probes`, `n_footprint` (samples ended on a blocked probe) and `start_probe` (the first probe that is not free
        at the start pose, -1: none) int32 [B] each, of the source's last local_plan_async with a footprint (waits as
        local_commands does; pp_get_local_footprint)."""
        k = self._infl_source(source)
        B = self._local_last(k, "local_footprint")[0]
        if self._local_foot_run.get(k) is None:
            raise RuntimeError(f"local_footprint: the last local plan of the {source} source had no footprint (set_local_footprint first)")
        info = np.zeros((B, _lib.PP_LOCAL_FOOT_INFO), np.int32)
        self._check(self._lib.pp_get_local_footprint(self._h, k, _ptr(info), B), "pp_get_local_footprint")
        return {name: info[:, i].copy() for i, name in enumerate(_loc.FOOT_INFO)}

    def _local_cells_async(self, k, poses, windows, resolution=None, dt=None, frame=None):
        """pp_local_plan_async on integers: poses int32 [B, 3] (X, Y, h), windows int32 [B, 4] (v0, dv, w0, dw).  frame
        float64 [B, 4] (ox, oy, res, dt): pp_local_plan_movers_async, the source's movers in front."""
        P = np.ascontiguousarray(poses, np.int32)
        Wn = np.ascontiguousarray(windows, np.int32)
        mc = None
        if frame is None:
            self._check(self._lib.pp_local_plan_async(self._h, k, _ptr(P), _ptr(Wn), int(P.shape[0])), "pp_local_plan_async")
        else:
            F = np.ascontiguousarray(frame, np.float64)
            if F.shape != (P.shape[0], 4):
                raise ValueError(f"local_plan_async: frame must be (ox, oy, res, dt) [{P.shape[0]}, 4], got {F.shape}")
            self._check(self._lib.pp_local_plan_movers_async(self._h, k, _ptr(P), _ptr(Wn), _ptr(F), int(P.shape[0])), "pp_local_plan_movers_async")
            mc = self.local_movers_config(_infl.SOURCES[k])
        self._local_run[k] = (int(P.shape[0]), self.local_planner_config(_infl.SOURCES[k]), resolution, dt)
        self._local_movers_run[k] = mc
        self._local_foot_run[k] = self.local_footprint_config(_infl.SOURCES[k])

    def local_plan_async(self, poses=None, windows=None, source="costmap", dt=None):
        """Queues the rollout and the command on the grids and fields of the source's last navfn_async behind the
        relaxation rounds that call queued (pp_local_plan_async) and returns at once.  poses float64 [B, 3] (x, y, yaw) (or
        one for every grid), metres and radians in the grids' frame; None: the sensor at yaw 0 for the costmap, the
        translation and atan2(R10, R00) of the poses of the occupancy_update_async whose maps the field's inflation read
        (inflate_async records them) for the occupancy maps.  They become
        sub-cells and ticks through local_planner.pose_ticks with the navfn run's origins and resolution (its record), so
        a pose outside its window is no error (cmd_state 3).  The run's own record holds (batch, LocalPlanConfig,
        resolution, step dt) and the MoverConfig it used: the getters size and unpack by them and
        local_commands(metric=True) converts by them, whatever set_local_planner, set_local_movers or set_costmap give
        afterwards.  windows integers [B, 4] (v0, dv, w0, dw) (or one), as
        local_planner.LocalLimits.window makes them; None: sv from 0 to 1024 and sw from -512 to 512.  dt: the seconds of
        a step, which `local_commands(metric=True)` needs -- and the source's movers, while set_local_movers has them
        on: the call then builds their table from the streams' tracks first (pp_local_plan_movers_async)."""
        k = self._infl_source(source)
        B, _, _, org, res, T = self._navfn_last(k, "local_plan_async")
        c = self.local_planner_config(source)
        if c is None:
            raise RuntimeError(f"local_plan_async: the local planner of the {source} source is not configured (set_local_planner first)")
        movers = self.local_movers_config(source) is not None
        if movers and dt is None:
            raise ValueError(f"local_plan_async: dt is None and the movers of the {source} source are on: they need the seconds of a step (dt=)")
        if org is None:
            raise RuntimeError("local_plan_async: the navigation function was given cells, it has no frame in metres")
        if poses is None:
            if k == 0:
                P = np.zeros((B, 3))
            else:
                P = np.stack([T[:, 0, 3], T[:, 1, 3], np.arctan2(T[:, 1, 0], T[:, 0, 0])], axis=1)
        else:
            P = np.asarray(poses, np.float64)
            if P.shape not in ((3,), (B, 3)):
                raise ValueError(f"local_plan_async: poses must be (x, y, yaw) [{B}, 3] (the navigation function run's grids) or one, got {P.shape}")
            P = np.broadcast_to(P, (B, 3))
        ticks = _loc.pose_ticks(P[:, :2], P[:, 2], org, res)
        if windows is None:
            windows = (0, _loc.MAX_SV // max(c.nv - 1, 1), -_loc.MAX_SW, 2 * _loc.MAX_SW // max(c.nw - 1, 1))
        Wn = _loc._batch_ints(windows, B, 4, "local_plan_async", "windows")
        for b in range(B):
            _loc.check_window(Wn[b], c, f"local_plan_async: grid {b}")
        frame = None
        if movers:
            frame = np.empty((B, 4))
            frame[:, :2] = np.broadcast_to(np.atleast_2d(np.asarray(org, np.float64)), (B, 2))
            frame[:, 2], frame[:, 3] = float(res), float(dt)
        self._local_cells_async(k, ticks, Wn, res, None if dt is None else float(dt), frame)

    def _local_last(self, k, who):
        if k not in self._local_run:
            raise RuntimeError(f"{who}: no local plan has run on the {_infl.SOURCES[k]} source (local_plan_async first)")
        return self._local_run[k]

    def _local_fetch(self, k, who, traj=False, keys=False):
        B, c, _, _ = self._local_last(k, who)
        res = np.zeros((B, _lib.PP_LOCAL_RESULT), np.int32)
        score = np.zeros(B, np.uint64)
        tr = np.zeros((B, c.steps + 1, 3), np.int32) if traj else None
        kk = np.zeros((B, c.nv * c.nw), np.uint64) if keys else None
        self._check(self._lib.pp_get_local_plan(self._h, k, _ptr(res), _ptr(score), _ptr(tr), _ptr(kk), B), "pp_get_local_plan")
        return _loc.unpack_results(c, B, res, score, tr, kk)

    def local_commands(self, source="costmap", metric=False):
        """(sv int32 [B], sw int32 [B], cmd_state int32 [B]) of the source's last local_plan_async, sub-cells and ticks per
        step (waits for it; the field is settled first and the rollout queued again if that took a further round: a
        command always rests on the exact field).  metric=True: (v float64 [B] m/s, w float64 [B] rad/s, cmd_state)
        through local_planner.command_metric with the run's resolution and step dt.  cmd_state as local_planner.py lists
        it (5: the footprint is not free at the start pose); the command is (0, 0) unless it is 0."""
        k = self._infl_source(source)
        out = self._local_fetch(k, "local_commands")
        if not metric:
            return out["sv"], out["sw"], out["cmd_state"]
        _, _, res, dt = self._local_last(k, "local_commands")
        if res is None or dt is None:
            raise RuntimeError("local_commands: metric=True needs the run's resolution and step dt (local_plan_async(..., dt=), or drive)")
        v, w = _loc.command_metric(out["sv"], out["sw"], res, dt)
        return v, w, out["cmd_state"]

    def local_trajectories(self, source="costmap"):
        """A list of B arrays int32 [steps + 1, 3], the winners' poses (X, Y, h) with the start included ([0, 3] where
        cmd_state is not 0), of the source's last local_plan_async (waits as local_commands does)."""
        return self._local_fetch(self._infl_source(source), "local_trajectories", traj=True)["traj"]

    def local_keys(self, source="costmap"):
        """All keys uint64 [B, nv * nw] of the source's last local_plan_async (waits as local_commands does; the rollout
        runs once more to store them the first time): (score << 14) | sample, local_planner.INVALID for a sample that
        did not end ok."""
        return self._local_fetch(self._infl_source(source), "local_keys", keys=True)["keys"]

    def local_plan_info(self, source="costmap"):
        """Per grid of the source's last local_plan_async (waits as local_commands does): `cmd_state`, `best`, `sv`, `sw`,
        `n_ok`, `n_outside`, `n_collision`, `n_unreached` int32 [B] each and `score` uint64 [B]; where that run had movers
        also `n_movers`, `n_skipped`, `n_dynamic` and `near` int32 [B]; where it had a footprint also `n_probes`,
        `n_footprint` and `start_probe` int32 [B]."""
        k = self._infl_source(source)
        out = self._local_fetch(k, "local_plan_info")
        if self._local_movers_run.get(k) is not None:
            out.update(self.local_movers(source)[1])
        if self._local_foot_run.get(k) is not None:
            out.update(self.local_footprint(source))
        return out

    def local_movers(self, source="costmap"):
        """(movers int32 [B, 64, 6] -- (mx, my, mvx, mvy, r_hard, r_soft) per mover, zeros behind a grid's n_movers --, info:
        `n_movers` (-1: an occupancy stream that has had no posed tracking step), `n_skipped`, `n_dynamic`, `near` int32 [B]
        each) of the source's last local_plan_async with movers (waits as local_commands does; pp_get_local_movers)."""
        k = self._infl_source(source)
        B = self._local_last(k, "local_movers")[0]
        if self._local_movers_run.get(k) is None:
            raise RuntimeError(f"local_movers: the last local plan of the {source} source had no movers (set_local_movers first)")
        M = np.zeros((B, _lib.PP_LOCAL_MAX_MOVERS, 6), np.int32)
        info = np.zeros((B, _lib.PP_LOCAL_MOVER_INFO), np.int32)
        self._check(self._lib.pp_get_local_movers(self._h, k, _ptr(M), _ptr(info), B), "pp_get_local_movers")
        return M, {name: info[:, i].copy() for i, name in enumerate(_loc.MOVER_INFO)}

    def _inflated_async(self, source):
        """What `plan` and `explore` queue first: the costmap stage if no costmap_async is pending, and the source's inflation."""
        k = self._infl_source(source)
        if k == 0:
            if not self._costmap_queued:
                self.costmap_async()
            self.inflate_async("costmap")
            self._costmap_queued = False
        else:
            self.inflate_async("occupancy")
        return k

    def _plan_async(self, goals, source, starts):
        """What `plan` queues: the source's grids, their inflation, the field and the paths."""
        k = self._inflated_async(source)
        self.navfn_async(goals, source, starts)
        return k

    def drive(self, goals, velocities, limits, source="costmap", poses=None):
        """(v float64 [B] m/s, w float64 [B] rad/s, cmd_state int32 [B]) towards `goals` (as navfn_async takes them; with
        set_local_movers on, round the streams' moving tracks): what
        `plan` queues, then the local planner on the dynamic windows round the current `velocities` float64 [B, 2] (v m/s,
        w rad/s) (or one) under `limits`, a local_planner.LocalLimits; a step lasts limits.step_dt(resolution), so a
        rollout looks steps * step_dt ahead (LocalLimits.steps gives the steps for its sim_time).  poses as
        local_plan_async takes them.  Only the commands travel to the host."""
        if not isinstance(limits, _loc.LocalLimits):
            raise ValueError(f"drive: limits must be a local_planner.LocalLimits, got {limits!r}")
        c = self.local_planner_config(source)
        if c is None:
            raise RuntimeError(f"drive: the local planner of the {source} source is not configured (set_local_planner first)")
        k = self._plan_async(goals, source, None)
        B, res = self._navfn_last(k, "drive")[0], self._navfn_last(k, "drive")[4]
        V = np.asarray(velocities, np.float64)
        if V.shape not in ((2,), (B, 2)):
            raise ValueError(f"drive: velocities must be (v, w) [{B}, 2] or one, got {V.shape}")
        V = np.broadcast_to(V, (B, 2))
        Wn = np.array([limits.window(V[b, 0], V[b, 1], c.nv, c.nw, res) for b in range(B)], np.int32)
        self.local_plan_async(poses, Wn, source, dt=limits.step_dt(res))
        return self.local_commands(source, metric=True)

    def _pose_args(self, poses, stamps, batch, who):
        """poses= of a detect*: checked before anything is queued (None: no accumulation); stamps then serve the sweeps, and
        the tracker too when tracking is on.  Returns (what accumulate_sweeps takes or None, what _stamps_dt returns, the
        poses for the tracker or None); the last only under set_track_ego with tracking on, and then the poses are accepted
        without sweeps as well (and, the sweeps off, without stamps: the streams advance by the period)."""
        if poses is None:
            return None, self._stamps_dt(stamps, batch), None
        ego = self._track_ego and self.tracking_on
        if ego and not self._get_sweeps()[0]:
            if np.asarray(poses).shape[:1] != (batch,):
                raise ValueError(f"{who}: {np.asarray(poses).shape[0] if np.asarray(poses).ndim else 0} poses for {batch} frames")
            return None, self._stamps_dt(stamps, batch), _swp.check_poses(poses, batch)
        if stamps is None:
            raise ValueError(f"{who}: poses needs stamps (one time stamp in seconds per frame)")
        if np.asarray(poses).shape[:1] != (batch,):
            raise ValueError(f"{who}: {np.asarray(poses).shape[0] if np.asarray(poses).ndim else 0} poses for {batch} frames")
        P = self._sweep_call(poses, stamps, who)[0]
        return (poses, stamps), (self._stamps_dt(stamps, batch) if self.tracking_on else None), (P if ego else None)

    # ---- live-camera ingest (pp_ingest_*; ingest.py states the rule) ----
    def _ingest_sync(self, name, args, batch, cap, nf, cameras=None):
        """One synchronous pp_ingest_* call.  args: what the call takes between the handle and the parity tap; cap: the
        points the tap must hold, or None for no tap; nf: feature columns (None: x y z only); cameras: of a rig call.
        Returns the tap's points, one [n_b, 3 + nf] float32 array per frame, or None."""
        pts = None if cap is None else np.empty((max(cap, 1), 3 + (nf or 0)), np.float32)
        self._check(getattr(self._lib, name)(self._h, *args, _ptr(pts), ctypes.c_int64(cap or 0)), name)
        self._offsets = None          # the resident frames' sizes are device values (ingest_info reads them back)
        self._ing_batch = batch
        if cameras is not None:       # (a plain call leaves the last rig's shape: the library refuses ingest_rig_info then)
            self._rig_shape = (batch, cameras)
        if pts is None:
            return None
        off = np.concatenate([[0], np.cumsum(self.ingest_info()["kept"])])
        return [pts[off[b]:off[b + 1]].copy() for b in range(batch)]

    def _ingest_async(self, name, staging, args, batch, cameras=None):
        """One pp_ingest_*_async call from a staging.  args: what the call takes behind the bytes and their offsets."""
        self._check(getattr(self._lib, name)(self._h, _ptr(staging.bytes), _ptr(staging.byte_offsets), *args), name)
        self._offsets = None
        self._ing_batch = batch
        if cameras is not None:
            self._rig_shape = (batch, cameras)
        staging._users.add(self)
        self._staged.append(staging)      # kept alive while a copy may still read it (see upload_async)

    def _detect_after_ingest(self, batch, rect, trv2c, on_numeric, dts=None, sweep=None, ego=None):
        if rect is not None:
            self.set_calib(rect, trv2c, batch)
        return self._detect_resident(on_numeric, dts, sweep, ego)

    def ingest_pointcloud2(self, msgs, first=1, decimate=4, lift=None, return_points=False, features=None, mount=None):
        """Raw sensor_msgs/PointCloud2 messages -> the engine's resident frames, on the GPU: x y z out of the bytes,
        non-finite records dropped, every `decimate`-th survivor from index `first`, camera axes turned into lidar axes
        and lifted by `lift` (ingest.SENSOR_HEIGHT) -- `ingest.realsense_to_lidar(ingest.pointcloud2_to_xyz(...))`
        exactly.  msgs: list of messages (`ingest.as_tuple`).  The engine needs max_points_per_frame >=
        ingest.kept_bound(width, height, first, decimate) (76800 for a 640 x 480 cloud at 1, 4).  There is no host
        fallback: a layout the library refuses raises with its text.  return_points: the resident points, one [n_b, F]
        float32 array per frame (the parity tap).
        features: a list of F - 3 `ingest.FeatureField`s for an engine with num_point_features F > 3 (x y z intensity: one)
        -- row columns 3 ... come out of the messages' own fields, float32(float64(raw) * scale + bias), exactly
        `ingest.ingest_np(msg, ..., features=features)` (pp_ingest_pointcloud2_fields).  Validity and selection are x y
        z's alone; a non-finite feature value is carried through as it is.  None: x y z only, which an engine with F != 3
        refuses.  Messages that name or scale the field differently: a list with one such list per message
        (`ingest.rig_features`).  mount: an `ingest.Mount` in place of the reference's RealSense matrices and `lift` (a lidar:
        Mount(np.eye(3), np.eye(3), 0.0))."""
        from . import ingest
        tuples = [ingest.as_tuple(m) for m in msgs]
        offs, layouts, bufs = _pack_messages(tuples)
        cfg = _ingest_config(first, decimate, lift, mount)
        table, nf = _feature_table(tuples, None if features is None else ingest.rig_features(features, len(tuples)))
        name, args = "pp_ingest_pointcloud2", (_ptr(_concat(bufs, offs)), _ptr(offs), layouts, len(tuples), ctypes.byref(cfg))
        if table is not None:
            name, args = "pp_ingest_pointcloud2_fields", args + (table, nf)
        return self._ingest_sync(name, args, len(tuples), _tap_rows(tuples, first, decimate) if return_points else None, nf)

    def ingest_info(self):
        """Per frame of the last ingest: `finite` records and points `kept` (pp_ingest_info; waits for the ingest)."""
        return self._stage_info("pp_ingest_info", ("finite", "kept"), getattr(self, "_ing_batch", 0))

    def staging_pointcloud2(self, msgs, features=None, mount=None):
        """Packs messages into a page-locked MessageStaging for ingest_pointcloud2_async (the counterpart of staging()).
        features (as ingest_pointcloud2) are resolved against the messages here and kept with the staging; so is `mount`
        (an `ingest.Mount`), which ingest_pointcloud2_async then uses unless it is given one."""
        st = MessageStaging(self._lib, msgs, features)
        st.mount = mount
        return st

    def ingest_pointcloud2_async(self, staging, first=1, decimate=4, lift=None, features=None, mount=None):
        """ingest_pointcloud2 without waiting (pp_ingest_pointcloud2_async): the bytes of a MessageStaging travel on the
        copy stream and are ingested and voxelised there, beside the pass in flight; the buffer must not be rewritten
        before the sync() that follows the detect_async() consuming these frames.  Mixes freely with upload_async.
        features / mount: None -> the staging's own (staging_pointcloud2(msgs, features=..., mount=...)); given here, they
        are resolved against the staged messages' fields for this call (pp_ingest_pointcloud2_fields_async)."""
        from . import ingest
        B = staging.byte_offsets.shape[0] - 1
        if mount is None and lift is None:
            mount = getattr(staging, "mount", None)
        cfg = _ingest_config(first, decimate, lift, mount)
        table, nf = staging.features, staging.nfeat
        if features is not None:
            table, nf = _feature_table(staging.tuples(), ingest.rig_features(features, B))
        name, args = "pp_ingest_pointcloud2_async", (staging.layouts, B, ctypes.byref(cfg))
        if table is not None:
            name, args = "pp_ingest_pointcloud2_fields_async", args + (table, nf)
        self._ingest_async(name, staging, args, B)

    def detect_pointcloud2(self, msgs, rect=None, trv2c=None, on_numeric="f32", features=None, mount=None, first=1, decimate=4,
                           stamps=None, poses=None):
        """ingest_pointcloud2 + detect_async + sync + detections: `detect` for raw camera messages (the reference's
        production mode, train.py:810-828).  rect / trv2c / on_numeric as `detect`; features / mount / first / decimate as
        ingest_pointcloud2 (a lidar feeding a 4-feature model: features=[FeatureField("intensity")],
        mount=Mount(np.eye(3), np.eye(3), 0.0), first=0, decimate=1); stamps and poses as `detect`."""
        sweep, dts, ego = self._pose_args(poses, stamps, len(msgs), "detect_pointcloud2")
        self.ingest_pointcloud2(msgs, first=first, decimate=decimate, features=features, mount=mount)
        return self._detect_after_ingest(len(msgs), rect, trv2c, on_numeric, dts, sweep, ego)

    # ---- depth-image ingest (pp_ingest_depth*) ----
    def ingest_depth(self, images, intrinsics, first=1, decimate=4, lift=None, depth_scale=0.001, z_min=0.0, z_max=np.inf,
                     return_points=False):
        """Raw depth images (sensor_msgs/Image: 16UC1 / mono16 units of `depth_scale`, or 32FC1 metres) -> the engine's
        resident frames, on the GPU: valid pixels deprojected through the pinhole `intrinsics`, every `decimate`-th from
        index `first`, turned into lidar axes and lifted -- `ingest.depth_ingest_np` exactly, i.e. what
        ingest_pointcloud2 gives for the message a point-cloud node computes from the image
        (`ingest.depth_to_pointcloud2`).  images: list of images (`ingest.image_as_tuple`); intrinsics: one set for the
        batch (`ingest.intrinsics_of`: a CameraInfo, (K, D) or (fx, fy, ppx, ppy)) or a list with one per frame; a pixel
        is valid only when z_min < z <= z_max.  The engine needs max_points_per_frame >=
        ingest.depth_kept_bound(width, height, first, decimate).  No host fallback; return_points as ingest_pointcloud2;
        ingest_info() reads the valid and kept counts back."""
        from . import ingest
        tuples = [ingest.image_as_tuple(m) for m in images]
        layouts = _depth_layouts(tuples, intrinsics, depth_scale, z_min, z_max)
        offs, bufs = _pack_images(tuples)
        cfg = _ingest_config(first, decimate, lift)
        return self._ingest_sync("pp_ingest_depth", (_ptr(_concat(bufs, offs)), _ptr(offs), layouts, len(tuples), ctypes.byref(cfg)),
                                 len(tuples), _tap_rows(tuples, first, decimate) if return_points else None, None)

    def staging_depth(self, images):
        """Packs depth images into a page-locked DepthStaging for ingest_depth_async (the counterpart of staging())."""
        return DepthStaging(self._lib, images)

    def ingest_depth_async(self, staging, intrinsics, first=1, decimate=4, lift=None, depth_scale=0.001, z_min=0.0,
                           z_max=np.inf):
        """ingest_depth without waiting (pp_ingest_depth_async), from a DepthStaging: as ingest_pointcloud2_async, and
        mixes freely with it and with upload_async."""
        tuples = staging.tuples()
        layouts = _depth_layouts(tuples, intrinsics, depth_scale, z_min, z_max)
        cfg = _ingest_config(first, decimate, lift)
        self._ingest_async("pp_ingest_depth_async", staging, (layouts, len(tuples), ctypes.byref(cfg)), len(tuples))

    def detect_depth(self, images, intrinsics, rect=None, trv2c=None, on_numeric="f32", stamps=None, poses=None):
        """ingest_depth + detect_async + sync + detections: `detect_pointcloud2` for the depth images the messages are
        computed from.  rect / trv2c / on_numeric / stamps / poses as `detect`."""
        sweep, dts, ego = self._pose_args(poses, stamps, len(images), "detect_depth")
        self.ingest_depth(images, intrinsics)
        return self._detect_after_ingest(len(images), rect, trv2c, on_numeric, dts, sweep, ego)

    # ---- camera-rig ingest (pp_ingest_rig_*) ----
    def ingest_rig_depth(self, frames, rig, return_points=False):
        """The depth images of a camera rig -> the engine's resident frames, on the GPU: frame b holds the kept points of
        its cameras in rig order, back to back, each camera under its own mount, intrinsics and selection --
        `ingest.rig_depth_ingest_np(frames[b], rig)` exactly.  frames: list of B lists of images, one per camera of the
        rig (`ingest.CameraRig`).  The engine needs max_points_per_frame >= ingest.rig_kept_bound(sizes, rig).  No host
        fallback; return_points as ingest_depth; ingest_info() then reads the frames' sums, ingest_rig_info() the
        cameras' own counts."""
        from . import ingest
        flat, fmap = ingest.rig_frame_map(frames, rig, "ingest_rig_depth")
        tuples = [ingest.image_as_tuple(m) for m in flat]
        layouts = _rig_depth_layouts(tuples, rig)
        offs, bufs = _pack_images(tuples)
        B, cap = len(frames), _rig_tap_rows(tuples, rig)
        args = (_ptr(_concat(bufs, offs)), _ptr(offs), layouts, _rig_configs(rig, B), _ptr(fmap), len(fmap), B)
        return self._ingest_sync("pp_ingest_rig_depth", args, B, cap if return_points else None, None, len(rig))

    def ingest_rig_pointcloud2(self, frames, rig, return_points=False, features=None):
        """ingest_rig_depth for PointCloud2 messages: `ingest.rig_ingest_np(frames[b], rig)` exactly (the rig's intrinsics,
        depth_scale and clip are not read).  features (`ingest.rig_features`: one list of FeatureFields for every camera, or
        one list per camera): rows of 3 + nf floats as ingest_pointcloud2(features=...) writes them,
        `ingest.rig_ingest_np(frames[b], rig, features)` exactly (pp_ingest_rig_pointcloud2_fields)."""
        from . import ingest
        flat, fmap = ingest.rig_frame_map(frames, rig, "ingest_rig_pointcloud2")
        tuples = [ingest.as_tuple(m) for m in flat]
        offs, layouts, bufs = _pack_messages(tuples)
        B, cap = len(frames), _rig_tap_rows(tuples, rig)
        table, nf = _rig_feature_table(tuples, rig, features)
        name, args = "pp_ingest_rig_pointcloud2", (_ptr(_concat(bufs, offs)), _ptr(offs), layouts, _rig_configs(rig, B), _ptr(fmap),
                                                   len(fmap), B)
        if table is not None:
            name, args = "pp_ingest_rig_pointcloud2_fields", args + (table, nf)
        return self._ingest_sync(name, args, B, cap if return_points else None, nf, len(rig))

    def ingest_rig_info(self):
        """Per camera of the last rig ingest: `finite` records (valid pixels) and points `kept`, int32 [B, cameras]
        (pp_ingest_rig_info; waits for the ingest)."""
        B, C = getattr(self, "_rig_shape", (0, 0))
        return {k: v.reshape(B, C) for k, v in self._stage_info("pp_ingest_rig_info", ("finite", "kept"), B * C).items()}

    def staging_rig_depth(self, frames, rig):
        """Packs the depth images of B rig frames into a page-locked RigDepthStaging for ingest_rig_depth_async."""
        return RigDepthStaging(self._lib, frames, rig)

    def staging_rig_pointcloud2(self, frames, rig, features=None):
        """Packs the messages of B rig frames into a page-locked RigMessageStaging for ingest_rig_pointcloud2_async;
        features (as ingest_rig_pointcloud2) are resolved against the messages here and kept with the staging."""
        return RigMessageStaging(self._lib, frames, rig, features)

    @staticmethod
    def _rig_async_args(name, staging, layouts, rig):
        """What a pp_ingest_rig_*_async call takes behind the bytes and their offsets."""
        S, B = len(staging.source_frame), staging.batch
        if S != B * len(rig):
            raise ValueError(f"{name}: the staging holds {S} sources in {B} frames, the rig has {len(rig)} cameras")
        return (layouts, _rig_configs(rig, B), _ptr(staging.source_frame), S, B)

    def ingest_rig_depth_async(self, staging, rig):
        """ingest_rig_depth without waiting (pp_ingest_rig_depth_async), from a RigDepthStaging: as ingest_depth_async, and
        mixes freely with it, with ingest_pointcloud2_async and with upload_async."""
        name = "pp_ingest_rig_depth_async"
        args = self._rig_async_args(name, staging, _rig_depth_layouts(staging.tuples(), rig), rig)
        self._ingest_async(name, staging, args, staging.batch, len(rig))

    def ingest_rig_pointcloud2_async(self, staging, rig, features=None):
        """ingest_rig_pointcloud2 without waiting (pp_ingest_rig_pointcloud2_async), from a RigMessageStaging.  features:
        None -> the staging's own (staging_rig_pointcloud2(frames, rig, features=...)); given here, they are resolved
        against the staged messages' fields for this call."""
        table, nf = staging.features, staging.nfeat
        if features is not None:
            table, nf = _rig_feature_table(staging.tuples(), rig, features)
        name = "pp_ingest_rig_pointcloud2_async"
        args = self._rig_async_args(name, staging, staging.layouts, rig)
        if table is not None:
            name, args = "pp_ingest_rig_pointcloud2_fields_async", args + (table, nf)
        self._ingest_async(name, staging, args, staging.batch, len(rig))

    def detect_rig_depth(self, frames, rig, rect=None, trv2c=None, on_numeric="f32", stamps=None, poses=None):
        """ingest_rig_depth + detect_async + sync + detections: `detect_depth` for a rig's images.  rect / trv2c /
        on_numeric / stamps / poses as `detect`."""
        sweep, dts, ego = self._pose_args(poses, stamps, len(frames), "detect_rig_depth")
        self.ingest_rig_depth(frames, rig)
        return self._detect_after_ingest(len(frames), rect, trv2c, on_numeric, dts, sweep, ego)

    def detect_rig_pointcloud2(self, frames, rig, rect=None, trv2c=None, on_numeric="f32", features=None, stamps=None,
                               poses=None):
        """ingest_rig_pointcloud2 + detect_async + sync + detections; features as ingest_rig_pointcloud2, stamps and
        poses as `detect`."""
        sweep, dts, ego = self._pose_args(poses, stamps, len(frames), "detect_rig_pointcloud2")
        self.ingest_rig_pointcloud2(frames, rig, features=features)
        return self._detect_after_ingest(len(frames), rect, trv2c, on_numeric, dts, sweep, ego)

    def intermediates(self, canvas=False):
        d, B = self.d, max(self._batches()[1], 1)
        H, W, k = d.head_h, d.head_w, d.num_anchor_per_loc
        out = {
            "n_pillars": np.zeros((B,), np.int32),
            "coors": np.zeros((B, d.max_voxels, 3), np.int32),
            "num_points": np.zeros((B, d.max_voxels), np.int32),
            "anchors_mask": np.zeros((B, self.anchors.shape[0]), np.uint8),
            "box_preds": np.zeros((B, H, W, k * 7), np.float32),
            "cls_preds": np.zeros((B, H, W, k * d.num_class), np.float32),
            "dir_cls_preds": np.zeros((B, H, W, k * 2), np.float32) if d.use_direction_classifier else None,
        }
        cv = np.zeros((B, d.ny, d.nx, d.pfn_filters), np.float32) if canvas else None
        self._check(self._lib.pp_fetch_intermediates(
            self._h, _ptr(out["n_pillars"]), _ptr(out["coors"]), _ptr(out["num_points"]), _ptr(out["anchors_mask"]),
            _ptr(out["box_preds"]), _ptr(out["cls_preds"]), _ptr(out["dir_cls_preds"]), _ptr(cv)),
            "pp_fetch_intermediates")
        if canvas:
            out["canvas"] = cv
        if out["dir_cls_preds"] is None:
            del out["dir_cls_preds"]
        return out

    # ---- measurement ----
    def set_profiling(self, on):
        self._check(self._lib.pp_set_profiling(self._h, 1 if on else 0), "pp_set_profiling")

    def kernel_times(self):
        cap = 2048
        names = (ctypes.c_char_p * cap)()
        ms = (ctypes.c_float * cap)()
        n = ctypes.c_int32(0)
        self._check(self._lib.pp_get_kernel_times(self._h, cap, names, ms, ctypes.byref(n)), "pp_get_kernel_times")
        return [(names[i].decode(), float(ms[i])) for i in range(min(n.value, cap))]

    def layer_tags(self):
        n = ctypes.c_int32(0)
        self._check(self._lib.pp_layer_count(self._h, ctypes.byref(n)), "pp_layer_count")
        return [self._lib.pp_layer_tag(self._h, i).decode() for i in range(n.value)]

    def bench_layer(self, layer, batch, reps=20):
        t = ctypes.c_float(0)
        self._check(self._lib.pp_bench_layer(self._h, int(layer), int(batch), int(reps), 0, ctypes.byref(t)),
                    "pp_bench_layer")
        return float(t.value)

    def loss_config(self):
        """The reference's loss keys (model.second.loss..., configs/train.yaml:147-167) as the C-ABI struct."""
        s = self.d.config["model"]["second"]
        lc = _lib.PPLossConfig()
        focal = s["loss"]["classification_loss"]["weighted_sigmoid_focal"]
        l1 = s["loss"]["localization_loss"]["weighted_smooth_l1"]
        lc.alpha = -1.0 if focal["alpha"] is None else float(focal["alpha"])
        lc.gamma = float(focal["gamma"] or 0.0)
        lc.sigma = float(l1["sigma"])
        for i, v in enumerate(l1["code_weight"]):
            lc.code_weight[i] = float(v)
        lc.pos_class_weight = float(s["pos_class_weight"])
        lc.neg_class_weight = float(s["neg_class_weight"])
        lc.classification_weight = float(s["loss"]["classification_weight"])
        lc.localization_weight = float(s["loss"]["localization_weight"])
        lc.direction_loss_weight = float(s["direction_loss_weight"])
        lc.norm_by_num_positives = 1 if s["loss_norm_type"] == "NormByNumPositives" else 0
        lc.encode_rad_error_by_sin = 1 if s["encode_rad_error_by_sin"] else 0
        lc.use_direction_classifier = 1 if s["use_direction_classifier"] else 0
        return lc

    def head_loss(self, labels, reg_targets, want_grad=True):
        """Training loss of the head maps the last forward pass left on the device (VoxelNet.call in training
        mode, model/voxelnet.py:922-1049) and its gradient with respect to them.  labels [B, A] int32,
        reg_targets [B, A, 7] float32 (the dataloader's `labels` / `reg_targets`).  Returns the reference's
        scalar keys and, if asked, `box_preds_grad` / `cls_preds_grad` / `dir_cls_preds_grad` shaped like
        the head maps."""
        labels = _i32(np.asarray(labels))
        batch = labels.shape[0]
        reg_targets = _f32(np.asarray(reg_targets).reshape(batch, self.d.num_anchors, 7))
        if labels.shape != (batch, self.d.num_anchors):
            raise ValueError(f"labels must be [B, {self.d.num_anchors}]")
        losses = np.zeros(8, np.float32)
        hh, hw = self.d.head_h, self.d.head_w
        grad = np.zeros((batch, hh * hw, 32), np.float32) if want_grad else None
        lc = self.loss_config()
        self._check(self._lib.pp_head_loss(self._h, _ptr(labels), _ptr(reg_targets), batch, ctypes.byref(lc),
                                           _ptr(losses), _ptr(grad) if want_grad else None), "pp_head_loss")
        out = {"loss": float(losses[0]), "loc_loss_reduced": float(losses[1]), "cls_loss_reduced": float(losses[2]),
               "dir_loss_reduced": float(losses[3]), "cls_pos_loss": float(losses[4]), "cls_neg_loss": float(losses[5]),
               "num_positives": int(losses[6])}
        if want_grad:
            na = self.d.num_anchor_per_loc
            nb, nc = na * 7, na * self.d.num_class      # head row: [box na*7 | cls na*num_class | dir na*2 | pad]
            out["head_grad"] = grad
            out["box_preds_grad"] = grad[:, :, :nb].reshape(batch, hh, hw, nb)
            out["cls_preds_grad"] = grad[:, :, nb:nb + nc].reshape(batch, hh, hw, nc)
            if self.d.use_direction_classifier:
                out["dir_cls_preds_grad"] = grad[:, :, nb + nc:nb + nc + 2 * na].reshape(batch, hh, hw, 2 * na)
        return out

    # ---- training metrics (f8) ----
    def head_metrics(self, labels, cls_preds=None):
        """The monitoring counts of one step (pp_head_metrics; libraries/metrics.py's Accuracy and PrecisionRecall,
        metrics.py here): labels [B, A] int32 against the class logits of the head map the last forward pass or training
        step left on the device, or against cls_preds [B, A, num_class] (any shape of that size) when given.  Returns
        metrics.unpack_counts' dict (acc_hit, n_pos, n_neg, tp, fp, fn, tn) plus "counts", the raw int64[32]."""
        from . import metrics as _metrics
        labels = _i32(np.asarray(labels))
        batch = labels.shape[0]
        if labels.shape != (batch, self.d.num_anchors):
            raise ValueError(f"labels must be [B, {self.d.num_anchors}]")
        if cls_preds is not None:
            cls_preds = _f32(np.asarray(cls_preds))
            if cls_preds.size != batch * self.d.num_anchors * self.d.num_class or cls_preds.shape[0] != batch:
                raise ValueError(f"cls_preds must hold [B, {self.d.num_anchors}, {self.d.num_class}] logits")
        counts = np.zeros(_lib.PP_METRICS_COUNTS, np.int64)
        self._check(self._lib.pp_head_metrics(self._h, _ptr(labels), batch, _ptr(cls_preds) if cls_preds is not None else None,
                                              _ptr(counts)), "pp_head_metrics")
        out = _metrics.unpack_counts(counts)
        out["counts"] = counts
        return out

    def set_train_metrics(self, on):
        """Count the monitoring metrics inside every following training step (pp_set_train_metrics); off by default."""
        self._check(self._lib.pp_set_train_metrics(self._h, 1 if on else 0), "pp_set_train_metrics")

    @property
    def train_metrics(self):
        """Whether training steps count their metrics (pp_get_train_metrics_enabled)."""
        v = ctypes.c_int32(0)
        self._check(self._lib.pp_get_train_metrics_enabled(self._h, ctypes.byref(v)), "pp_get_train_metrics_enabled")
        return bool(v.value)

    def train_metrics_counts(self):
        """int64[32] counts of the last training step, after train_step_wait() (pp_get_train_metrics); raises when that
        step ran with the metrics off."""
        counts = np.zeros(_lib.PP_METRICS_COUNTS, np.int64)
        self._check(self._lib.pp_get_train_metrics(self._h, _ptr(counts)), "pp_get_train_metrics")
        return counts

    # ---- training step (f3) ----
    def train_layout(self):
        """[(name, offset, size, is_state)] of the flat parameter / BatchNorm-state buffers (pp_train_layout)."""
        n, npar, nst = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.pp_train_layout(self._h, ctypes.byref(n), ctypes.byref(npar), ctypes.byref(nst)), "pp_train_layout")
        out = []
        for i in range(n.value):
            name, off, size, st = ctypes.c_char_p(), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0)
            self._check(self._lib.pp_train_layout_entry(self._h, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(size),
                                                        ctypes.byref(st)), "pp_train_layout_entry")
            out.append((name.value.decode(), off.value, size.value, bool(st.value)))
        return out, npar.value, nst.value

    def train_set_frozen(self, units):
        """Freeze the named units for the following training steps (pp_train_set_frozen; () unfreezes everything)."""
        names = [u.encode() for u in units]
        arr = (ctypes.c_char_p * max(1, len(names)))(*names)
        self._check(self._lib.pp_train_set_frozen(self._h, arr, len(names)), "pp_train_set_frozen")

    def train_graph_stats(self):
        """(captures, replays) of pp_train_step's hipGraphs: steady-state steps must replay."""
        c, r = ctypes.c_int32(0), ctypes.c_int32(0)
        self._check(self._lib.pp_train_graph_stats(self._h, ctypes.byref(c), ctypes.byref(r)), "pp_train_graph_stats")
        return c.value, r.value

    def pinned(self, shape, dtype):
        """A page-locked numpy array (PinnedArray) for targets / frames the loader fills in place."""
        return PinnedArray(self._lib, shape, dtype)

    def stream_ptr(self):
        """The handle's HIP stream as an integer (pp_stream): device work enqueued on it runs behind the handle's own."""
        p = ctypes.c_void_p(0)
        self._check(self._lib.pp_stream(self._h, ctypes.byref(p)), "pp_stream")
        return int(p.value or 0)

    @staticmethod
    def _loss_dict(losses):
        return {"loss": float(losses[0]), "loc_loss_reduced": float(losses[1]), "cls_loss_reduced": float(losses[2]),
                "dir_loss_reduced": float(losses[3]), "cls_pos_loss": float(losses[4]), "cls_neg_loss": float(losses[5]),
                "num_positives": int(losses[6])}

    def train_step_async(self, params_ptr, grads_ptr, state_ptr, labels, reg_targets):
        """Enqueue forward (training mode) + loss + backward on the resident frames (pp_train_step_async) and return.
        Until train_step_wait() the next batch may be uploaded (upload_async: the handle's other input buffer, on the
        copy stream beside the running kernels); labels / reg_targets are held here until then."""
        labels = _i32(np.asarray(labels))
        batch = labels.shape[0]
        reg_targets = _f32(np.asarray(reg_targets).reshape(batch, self.d.num_anchors, 7))   # (no copy when already so)
        if labels.shape != (batch, self.d.num_anchors):
            raise ValueError(f"labels must be [B, {self.d.num_anchors}]")
        lc = self.loss_config()
        self._check(self._lib.pp_train_step_async(self._h, ctypes.c_void_p(int(params_ptr)),
                                                  ctypes.c_void_p(int(grads_ptr)), ctypes.c_void_p(int(state_ptr)),
                                                  _ptr(labels), _ptr(reg_targets), batch, ctypes.byref(lc)),
                    "pp_train_step_async")
        self._train_targets = (labels, reg_targets)      # the copy engine reads them while the forward pass runs

    # ---- training targets from ground-truth boxes (f3, data half) ----
    def target_config(self):
        """The assignment's thresholds as the C-ABI struct (target_assigner.gpu_target_config: raises ValueError for a
        configuration with positive-fraction sampling)."""
        from .target_assigner import gpu_target_config
        hi, lo = gpu_target_config(self.d)
        tc = _lib.PPTargetConfig()
        tc.matched_threshold, tc.unmatched_threshold = hi, lo
        return tc

    @staticmethod
    def pack_gt(gt_boxes, gt_classes=None):
        """Per-frame [G_b, 7] boxes (and [G_b] classes, or None: all 1) -> (boxes [sum G, 7] float32, classes [sum G]
        int32 or None, counts [B] int32), the layout pp_assign_targets / pp_train_step_gt* take."""
        boxes = [np.asarray(g, dtype=np.float32).reshape(-1, 7) for g in gt_boxes]
        counts = np.array([len(g) for g in boxes], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(boxes, axis=0) if boxes else np.zeros((0, 7), np.float32))
        cls = None
        if gt_classes is not None:
            if len(gt_classes) != len(boxes):
                raise ValueError(f"gt_classes: {len(gt_classes)} frames, gt_boxes: {len(boxes)}")
            parts = [np.asarray(c, dtype=np.int32).reshape(-1) for c in gt_classes]
            for b, (c, g) in enumerate(zip(parts, boxes)):
                if len(c) != len(g):
                    raise ValueError(f"frame {b}: {len(g)} boxes but {len(c)} classes")
            cls = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0,), np.int32))
        return flat, cls, counts

    def assign_targets(self, gt_boxes, gt_classes=None, anchors_mask=None):
        """The training targets of len(gt_boxes) frames on the GPU (pp_assign_targets): target_assigner.assign as the
        reference's loader calls it (load_data.py:3086-3101), one dict per frame with create_target_np's keys and dtypes.
        gt_boxes: per frame [G_b, 7] x y z w l h r; gt_classes: per frame [G_b] (1..num_class) or None (all 1);
        anchors_mask: [B, A] (bool / uint8), or None = the masks of the frames uploaded to this engine."""
        boxes, cls, counts = self.pack_gt(gt_boxes, gt_classes)
        B, A = len(counts), self.d.num_anchors
        tc = self.target_config()
        mask = None
        if anchors_mask is not None:
            mask = np.ascontiguousarray(np.asarray(anchors_mask).reshape(B, A) != 0, dtype=np.uint8)
        labels = np.empty((B, A), np.int32)
        reg = np.empty((B, A, 7), np.float32)
        gi = np.empty((B, A), np.int32)
        ov = np.empty((B, A), np.float32)
        self._check(self._lib.pp_assign_targets(self._h, _ptr(boxes), _ptr(cls), _ptr(counts), B, _ptr(mask),
                                                ctypes.byref(tc), _ptr(labels), _ptr(reg), _ptr(gi), _ptr(ov)),
                    "pp_assign_targets")
        out = []
        for b in range(B):
            pos = np.where(labels[b] > 0)[0]
            w = np.zeros((A,), np.float32)
            w[pos] = 1.0
            matched = counts[b] > 0 and bool((ov[b] >= 0).any())      # overlap -1: a masked-out anchor
            out.append({"labels": labels[b], "bbox_targets": reg[b], "bbox_outside_weights": w,
                        "assigned_anchors_overlap": ov[b][pos] if matched else None,
                        "positive_gt_id": gi[b][pos].astype(np.int32), "assigned_anchors_inds": pos.astype(np.int64)})
        return out

    def train_step_gt_async(self, params_ptr, grads_ptr, state_ptr, boxes, classes, counts):
        """train_step_async with the targets assigned on the GPU from the boxes (pp_train_step_gt_async); boxes / classes
        / counts as pack_gt returns them (page-locked arrays: Trainer.stage_gt).  They are held here until
        train_step_wait()."""
        boxes = _f32(boxes).reshape(-1, 7)
        counts = _i32(counts).reshape(-1)
        classes = None if classes is None else _i32(classes).reshape(-1)
        lc, tc = self.loss_config(), self.target_config()
        self._check(self._lib.pp_train_step_gt_async(self._h, ctypes.c_void_p(int(params_ptr)),
                                                     ctypes.c_void_p(int(grads_ptr)), ctypes.c_void_p(int(state_ptr)),
                                                     _ptr(boxes), _ptr(classes), _ptr(counts), len(counts),
                                                     ctypes.byref(lc), ctypes.byref(tc)), "pp_train_step_gt_async")
        self._train_targets = (boxes, classes, counts)   # the copy engine reads them while the forward pass runs

    @staticmethod
    def _aug_args(gt_valid, total, draws, aug_config, n_boxes=None):
        """total: the draw rows; n_boxes: the boxes the flags describe (None: one draw row per box, the same number)."""
        from . import augment
        if aug_config is None:
            aug_config = augment.AugmentConfig.from_input_reader(None)
        if not isinstance(draws, augment.Draws):
            raise ValueError("draws: an augment.Draws (augment.draw) is required")
        ac = _lib.PPAugmentConfig()
        ac.num_try, ac.global_rot_per_object = aug_config.num_try, int(aug_config.global_rot_per_object)
        valid = None
        if isinstance(gt_valid, np.ndarray) and gt_valid.dtype == np.uint8 and gt_valid.ndim == 1:
            valid = gt_valid            # already flat (Trainer.stage_gt's page-locked flags)
        elif gt_valid is not None:
            valid = np.ascontiguousarray(np.concatenate([np.asarray(v, bool).reshape(-1) for v in gt_valid])
                                         if len(gt_valid) and not np.isscalar(gt_valid[0]) else np.asarray(gt_valid, bool),
                                         dtype=np.uint8).reshape(-1)
        n_boxes = total if n_boxes is None else n_boxes
        if valid is not None and len(valid) != n_boxes:
            raise ValueError(f"gt_valid: {len(valid)} flags for {n_boxes} boxes")
        bd = np.ascontiguousarray(draws.boxes, np.float64)
        if bd.shape[0] != total or (total and bd.shape[1] != aug_config.num_try):
            raise ValueError(f"draws: {bd.shape[:2]} box draws for {total} boxes x {aug_config.num_try} tries")
        return ac, valid, draws.frames_struct(), bd

    def augment(self, gt_boxes, gt_classes=None, gt_valid=None, draws=None, aug_config=None):
        """Training-time augmentation of the frames uploaded to this engine, on the GPU (pp_augment; augment.py lists the
        stages).  The resident frames are replaced by the augmented ones (a following train step trains on them).
        gt_boxes / gt_classes per frame as assign_targets; gt_valid per frame [G_b] bool (or None: all valid); draws:
        augment.draw(rs, gt_boxes, aug_config).  Returns per frame (points [n_b, F], boxes [K_b, 7], classes [K_b]) --
        the reference's debug_save_points view of the frame."""
        boxes, cls, counts = self.pack_gt(gt_boxes, gt_classes)
        ac, valid, frames, bd = self._aug_args(gt_valid, len(boxes), draws, aug_config)
        B = len(counts)
        self._need_host_offsets("augment")
        off = np.asarray(self._offsets, np.int64)
        n_total = int(off[-1])
        pts = np.empty((max(n_total, 1), self.d.num_point_features), np.float32)
        bo = np.empty((max(len(boxes), 1), 7), np.float32)
        co = np.empty((max(len(boxes), 1),), np.int32)
        cnt = np.empty((B,), np.int32)
        self._check(self._lib.pp_augment(self._h, _ptr(boxes), _ptr(cls), _ptr(valid), _ptr(counts), B, ctypes.byref(ac),
                                         frames.ctypes.data, bd.ctypes.data, _ptr(pts), _ptr(bo), _ptr(co), _ptr(cnt)),
                    "pp_augment")
        out, g = [], 0
        for b in range(B):
            k = int(cnt[b])
            out.append((pts[off[b]:off[b + 1]].copy(), bo[g:g + k].copy(), co[g:g + k].copy()))
            g += k
        return out

    def augment_selected(self):
        """The try each input box of the last augmentation took (-1: none, or an invalid box), in gt_boxes order
        (pp_augment_selected)."""
        n = ctypes.c_int64(0)
        self._check(self._lib.pp_augment_selected(self._h, None, 0, ctypes.byref(n)), "pp_augment_selected")
        out = np.empty(max(n.value, 1), np.int32)
        self._check(self._lib.pp_augment_selected(self._h, _ptr(out), n.value, ctypes.byref(n)), "pp_augment_selected")
        return out[:n.value].copy()

    # ---- GT-database sampling (pp_gtdb_load / pp_gt_sample) ----
    def load_gt_database(self, db):
        """Uploads a gt_sampler.GtDatabase (pp_gtdb_load); it stays on the device until another one replaces it."""
        from . import gt_sampler
        if not isinstance(db, gt_sampler.GtDatabase):
            raise ValueError("db: a gt_sampler.GtDatabase is required")
        if db.num_point_features != self.d.num_point_features:
            raise ValueError(f"db: objects have {db.num_point_features} point features, the engine "
                             f"{self.d.num_point_features}")
        pts, off = _f32(db.points), np.ascontiguousarray(db.offsets, np.int64)
        boxes, cls = np.ascontiguousarray(db.boxes, np.float64), _i32(db.classes)
        self._check(self._lib.pp_gtdb_load(self._h, _ptr(pts), _ptr(off), _ptr(boxes), _ptr(cls), len(db)), "pp_gtdb_load")
        self._gt_db = db

    def gt_sample(self, gt_boxes, gt_classes=None, gt_valid=None, candidates=None, sampler_config=None):
        """GT-database sampling into the frames uploaded to this engine, on the GPU (pp_gt_sample; gt_sampler.py lists
        the rules).  The resident frames are replaced by the sampled ones (a following augment / train step works on
        them).  gt_boxes / gt_classes / gt_valid per frame as augment; candidates: gt_sampler.draw_candidates(...).
        Returns per frame (points [n_b + pasted, F], boxes [G_b + K_b, 7], classes, valid)."""
        from . import gt_sampler
        db = getattr(self, "_gt_db", None)
        cfg = sampler_config if sampler_config is not None else (db.config if db is not None else None)
        if not isinstance(candidates, gt_sampler.Candidates):
            raise ValueError("candidates: a gt_sampler.Candidates (gt_sampler.draw_candidates) is required")
        boxes, cls, counts = self.pack_gt(gt_boxes, gt_classes)
        B, total = len(counts), len(boxes)
        if len(candidates) != B:
            raise ValueError(f"candidates: {len(candidates)} frames, gt_boxes: {B}")
        valid = None
        if gt_valid is not None:
            valid = np.ascontiguousarray(np.concatenate([np.asarray(v, bool).reshape(-1) for v in gt_valid] or
                                                        [np.zeros(0, bool)]), dtype=np.uint8)
            if len(valid) != total:
                raise ValueError(f"gt_valid: {len(valid)} flags for {total} boxes")
        sc = _lib.PPGtSampleConfig()
        if cfg is not None:
            sc.max_point_collision, sc.min_point_collision = cfg.max_point_collision, cfg.min_point_collision
        self._need_host_offsets("gt_sample")
        n_in = int(self._offsets[-1])
        cap = n_in + (int(np.diff(db.offsets)[candidates.cands["object"].clip(0, len(db) - 1)].sum())
                      if db is not None and len(db) else 0)
        F = self.d.num_point_features
        pts = np.empty((max(cap, 1), F), np.float32)
        offs = np.zeros((B + 1,), np.int32)
        rows = total + B * gt_sampler.PP_GTS_MAX_CAND
        bo, co, vo = np.empty((rows, 7), np.float32), np.empty((rows,), np.int32), np.empty((rows,), np.uint8)
        cnt = np.empty((B,), np.int32)
        self._check(self._lib.pp_gt_sample(self._h, _ptr(boxes), _ptr(cls), _ptr(valid), _ptr(counts), B, ctypes.byref(sc),
                                           candidates.cands.ctypes.data, candidates.counts.ctypes.data, _ptr(pts), cap,
                                           _ptr(offs), _ptr(bo), _ptr(co), _ptr(vo), _ptr(cnt)), "pp_gt_sample")
        self._offsets = offs          # the resident frames grew
        self._gts_batch = B
        out, g = [], 0
        for b in range(B):
            k = int(cnt[b])
            out.append((pts[offs[b]:offs[b + 1]].copy(), bo[g:g + k].copy(), co[g:g + k].copy(),
                        vo[g:g + k].astype(bool)))
            g += k
        return out

    # ---- building the object database from the resident frames (pp_gtdb_build / pp_gtdb_count) ----
    @staticmethod
    def _pack_lidar_boxes(gt_boxes):
        boxes = [np.asarray(g, dtype=np.float64).reshape(-1, 7) for g in gt_boxes]
        counts = np.array([len(g) for g in boxes], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(boxes, axis=0) if boxes else np.zeros((0, 7), np.float64))
        return flat, counts

    def count_points_in_gt(self, gt_boxes):
        """The points of each frame uploaded to this engine inside each of its boxes, on the GPU (pp_gtdb_count;
        gt_database.py lists the rule): the reference's num_points_in_gt.  gt_boxes: per frame [G_b, 7] float64 lidar
        boxes x y z w l h r.  Returns per frame an int32 array [G_b].  The resident frames are only read."""
        boxes, counts = self._pack_lidar_boxes(gt_boxes)
        out = np.zeros(max(len(boxes), 1), np.int32)
        self._check(self._lib.pp_gtdb_count(self._h, _ptr(boxes), _ptr(counts), len(counts), _ptr(out)), "pp_gtdb_count")
        ends = np.cumsum(counts)
        return [out[e - c:e].copy() for c, e in zip(counts, ends)]

    def build_gt_objects(self, gt_boxes, return_counts=False, capacity=None):
        """The labelled objects of the frames uploaded to this engine, cut out on the GPU (pp_gtdb_build; gt_database.py
        lists the rule): per frame a list of G_b float32 arrays [n, F], the points inside each box in the frame's order,
        centred on the box -- what create_groundtruth_database writes per object.  gt_boxes as count_points_in_gt.
        return_counts: (per-frame counts as count_points_in_gt returns them, objects).  capacity: the size of the
        output buffer in points (default: sized here, and grown once from the returned counts when it is too small; a
        given capacity that is too small raises).  The resident frames are only read."""
        boxes, counts = self._pack_lidar_boxes(gt_boxes)
        B, total, F = len(counts), len(boxes), self.d.num_point_features
        cnt = np.full(max(total, 1), -1, np.int32)
        off = np.zeros(total + 1, np.int64)
        fixed = capacity is not None
        resident = getattr(self, "_offsets", None)
        cap = int(capacity) if fixed else max(getattr(self, "_gdb_cap", 0), int(resident[-1]) if resident is not None else 0)
        while True:
            pts = np.empty((max(cap, 1), F), np.float32)
            st = self._lib.pp_gtdb_build(self._h, _ptr(boxes), _ptr(counts), B, _ptr(cnt), _ptr(off), _ptr(pts), cap)
            # too small: only the counts were written; size the buffer from them and call again
            if st == 1 and not fixed and total and (cnt[:total] >= 0).all() and int(cnt[:total].sum()) > cap:
                cap = int(cnt[:total].sum())
                fixed = True
                continue
            self._check(st, "pp_gtdb_build")
            break
        self._gdb_cap = max(getattr(self, "_gdb_cap", 0), cap)
        objs, per_frame, g = [], [], 0
        for b in range(B):
            objs.append([pts[off[g + i]:off[g + i + 1]].copy() for i in range(counts[b])])
            per_frame.append(cnt[g:g + counts[b]].copy())
            g += counts[b]
        return (per_frame, objs) if return_counts else objs

    def train_step_sample_async(self, params_ptr, grads_ptr, state_ptr, boxes, classes, counts, valid, candidates,
                                sampler_config, draws=None, aug_config=None):
        """train_step_gt_async on frames sampled -- and, with `draws`, augmented -- on the GPU first
        (pp_train_step_sample_async): boxes / classes / counts as pack_gt returns them, valid the concatenated flags (or
        None), candidates a gt_sampler.Candidates; draws: an augment.Draws with counts[b] + (slots of frame b's largest
        round) box rows per frame."""
        boxes = _f32(boxes).reshape(-1, 7)
        counts = _i32(counts).reshape(-1)
        classes = None if classes is None else _i32(classes).reshape(-1)
        B = len(counts)
        if len(candidates) != B:
            raise ValueError(f"candidates: {len(candidates)} frames, gt_boxes: {B}")
        sc = _lib.PPGtSampleConfig()
        sc.max_point_collision, sc.min_point_collision = sampler_config.max_point_collision, sampler_config.min_point_collision
        ac = frames = bd = None
        if draws is not None:
            rows = int((counts + candidates.counts.max(axis=1)).sum())
            ac, valid, frames, bd = self._aug_args(valid, rows, draws, aug_config, n_boxes=len(boxes))
        elif valid is not None:
            if not (isinstance(valid, np.ndarray) and valid.ndim == 1):
                valid = np.concatenate([np.asarray(v, bool).reshape(-1) for v in valid] or [np.zeros(0, bool)])
            valid = np.ascontiguousarray(valid, np.uint8).reshape(-1)
            if len(valid) != len(boxes):
                raise ValueError(f"gt_valid: {len(valid)} flags for {len(boxes)} boxes")
        lc, tc = self.loss_config(), self.target_config()
        self._check(self._lib.pp_train_step_sample_async(
            self._h, ctypes.c_void_p(int(params_ptr)), ctypes.c_void_p(int(grads_ptr)), ctypes.c_void_p(int(state_ptr)),
            _ptr(boxes), _ptr(classes), _ptr(counts), B, ctypes.byref(lc), ctypes.byref(tc), _ptr(valid), ctypes.byref(sc),
            candidates.cands.ctypes.data, candidates.counts.ctypes.data, None if ac is None else ctypes.byref(ac),
            None if frames is None else frames.ctypes.data, None if bd is None else bd.ctypes.data),
            "pp_train_step_sample_async")
        self._train_targets = (boxes, classes, counts, valid, candidates, frames, bd)
        self._gts_batch = B           # frames of the last sampling (gt_sample_info): a prefetch may replace _offsets

    def gt_sample_info(self):
        """Parity tap of the last gt_sample / sampled training step (pp_gt_sample_info): per frame and candidate slot its status
        (gt_sampler.STATUS_NAMES) and the frame points inside its box, and per frame the round that was pasted (-1:
        none)."""
        from . import gt_sampler
        B = getattr(self, "_gts_batch", 0)
        if B < 1:
            raise RuntimeError("gt_sample_info: no sampling has run on this engine")
        st = np.empty((B, gt_sampler.PP_GTS_MAX_CAND), np.int32)
        pc = np.empty((B, gt_sampler.PP_GTS_MAX_CAND), np.int32)
        ru = np.empty((B,), np.int32)
        self._check(self._lib.pp_gt_sample_info(self._h, _ptr(st), _ptr(pc), _ptr(ru), B), "pp_gt_sample_info")
        return {"status": st, "point_counts": pc, "round_used": ru}

    def train_step_aug_async(self, params_ptr, grads_ptr, state_ptr, boxes, classes, counts, valid, draws, aug_config):
        """train_step_gt_async on the frames augmented on the GPU first (pp_train_step_aug_async): boxes / classes /
        counts as pack_gt returns them, valid the concatenated flags (or None), draws an augment.Draws."""
        boxes = _f32(boxes).reshape(-1, 7)
        counts = _i32(counts).reshape(-1)
        classes = None if classes is None else _i32(classes).reshape(-1)
        ac, valid, frames, bd = self._aug_args(valid, len(boxes), draws, aug_config)
        lc, tc = self.loss_config(), self.target_config()
        self._check(self._lib.pp_train_step_aug_async(self._h, ctypes.c_void_p(int(params_ptr)),
                                                      ctypes.c_void_p(int(grads_ptr)), ctypes.c_void_p(int(state_ptr)),
                                                      _ptr(boxes), _ptr(classes), _ptr(counts), len(counts),
                                                      ctypes.byref(lc), ctypes.byref(tc), _ptr(valid), ctypes.byref(ac),
                                                      frames.ctypes.data, bd.ctypes.data), "pp_train_step_aug_async")
        self._train_targets = (boxes, classes, counts, valid, frames, bd)

    def train_step_wait(self):
        """Wait for the step train_step_async() launched; returns the reference's loss scalars."""
        losses = np.zeros(8, np.float32)
        self._check(self._lib.pp_train_step_wait(self._h, _ptr(losses)), "pp_train_step_wait")
        self._train_targets = None
        return self._loss_dict(losses)

    def train_step(self, params_ptr, grads_ptr, state_ptr, labels, reg_targets):
        """Forward (training mode) + loss + backward on the resident frames (pp_train_step).  The three pointers
        are integer device addresses of the flat float32 buffers; returns the reference's loss scalars."""
        self.train_step_async(params_ptr, grads_ptr, state_ptr, labels, reg_targets)
        return self.train_step_wait()

    def timer_start(self):
        self._check(self._lib.pp_timer_start(self._h), "pp_timer_start")

    def timer_stop(self):
        t = ctypes.c_float(0)
        self._check(self._lib.pp_timer_stop(self._h, ctypes.byref(t)), "pp_timer_stop")
        return float(t.value)

    def device_mem_free(self):
        v = ctypes.c_int64(0)
        self._check(self._lib.pp_device_mem_free(self._h, ctypes.byref(v)), "pp_device_mem_free")
        return v.value

    def device_copy_GBps(self, nbytes=1 << 30, reps=5):
        """Device-to-device copy rate (read + written GB/s) measured on the engine's stream."""
        g = ctypes.c_float(0)
        self._check(self._lib.pp_device_copy_bench(self._h, ctypes.c_int64(int(nbytes)), int(reps), ctypes.byref(g)),
                    "pp_device_copy_bench")
        return float(g.value)

    def device_info(self):
        name = ctypes.create_string_buffer(256)
        cu = ctypes.c_int32(0)
        mem = ctypes.c_int64(0)
        self._check(self._lib.pp_device_info(self._h, name, 256, ctypes.byref(cu), ctypes.byref(mem)), "pp_device_info")
        return {"name": name.value.decode(), "compute_units": cu.value, "hbm_bytes": mem.value}
