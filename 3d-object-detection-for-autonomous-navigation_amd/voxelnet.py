"""VoxelNet with the reference's call surface, backed by the HIP engine.

Mirror of model/voxelnet.py::VoxelNet for the eval path (train.py:575-771):
    net = VoxelNet(config, writer, training=False)
    net.load_weights(path_or_dict)
    preds_dict = net(voxels, num_points, coors, batch_anchors)      # NHWC head maps
    predictions_dicts = net.predict(example, preds_dict)            # list of dicts
`example` is the positional 10-tuple (voxels, num_points, coordinates, rect,
Trv2c, P2, anchors, anchors_mask, image_idx, image_shape); elements may be
numpy arrays or anything with `.numpy()` (the reference passes TF tensors).
`detect(frames, ...)` is the fused raw-points path the reference does not have; `detect_pointcloud2(msgs, ...)` is the
same from raw sensor_msgs/PointCloud2 messages (the reference's production mode, ingested on the GPU), and
`detect_depth(images, intrinsics, ...)` from the depth images those messages are computed from;
`detect_rig_depth(frames, rig, ...)` / `detect_rig_pointcloud2` put the cameras of a rig into one frame each.

Training mode (model/voxelnet.py:922-1049 + train.py:265-304), `VoxelNet(config, writer, training=True)`:
    ret = net(voxels, num_points, coors, batch_anchors, labels, reg_targets)   # the reference's loss dict (scalars)
    net.apply_gradients(dist=None)        # optimizer.apply_gradients: one all-reduce over the ranks + AdamW
or, from raw clouds, `net.train_step(frames, labels, reg_targets, dist)` -- or `net.train_step(frames, gt_boxes=boxes)`,
which assigns the targets on the GPU (the loader's target_assigner.assign, csrc/targets.hip).  A training net detects
with its current weights (`detect`, `detect_pointcloud2`, `detect_depth`): they are folded into the detector on the GPU first
(Trainer.publish, csrc/weight_publish.hip).  The forward pass, the loss and the
gradients of a call come from one `pp_train_step` (csrc/train.hip); the padded voxel tensor is unpadded on the
host into the pillar-ordered point list it was built from (the voxeliser then reproduces the same pillars).
"""
import os

import numpy as np

from . import tracking as _tracking
from . import weights as _weights
from .config import Derived
from .engine import Engine
from .trainer import Trainer


def _np(x):
    return x.numpy() if hasattr(x, "numpy") else np.asarray(x)


class VoxelNet:
    def __init__(self, config, writer=None, training=False, max_batch=None, max_points_per_frame=32768, device=0,
                 augment=None, seed=None, metrics=False, grad_clip=None):
        self.config = config
        self.training = bool(training)
        self.d = Derived(config)
        self.batch_size = self.d.batch_size
        self.box_code_size = 7
        self.trainer = None
        self._ctor = dict(max_batch=max_batch or self.batch_size, max_points_per_frame=max_points_per_frame, device=device)
        # training only: the loader's augmentation on the GPU (Trainer's augment= / seed=)
        self._train_kw = dict(augment=augment, seed=seed, metrics=bool(metrics), grad_clip=grad_clip)
        if not self.training and metrics:
            raise ValueError("metrics is a training option: build the net with training=True")
        if not self.training and augment:
            raise ValueError("augment is a training option: build the net with training=True")
        if self.training:
            self.engine = None      # the Trainer (created by load_weights: it needs initial values) owns the engine
        else:
            self.engine = Engine(self.d, **self._ctor)

    def _bboxes(self, batch):
        """The image boxes of the pass that has just run; None (the placeholder) without model.second.project_bbox."""
        return self.engine.bboxes(batch) if self.d.project_bbox else None

    def costmaps(self, batch=None, counts=False):
        """Engine.costmaps of the pass that has just run (model.second.costmap, or engine.set_costmap)."""
        return self.engine.costmaps(batch, counts)

    def occupancy_update(self, poses):
        """Engine.occupancy_update_async on the resident frames (engine.set_occupancy first): call it between the upload
        or ingest and a sweep accumulation."""
        return self.engine.occupancy_update_async(poses)

    def localize(self, poses):
        """Engine.localize on the resident frames (engine.set_occupancy and engine.set_scan_match first): the priors
        corrected by a scan match against the streams' maps, then the frames fused under the corrected poses.  Returns
        (corrected poses [B, 3, 4], words [B, 8])."""
        return self.engine.localize(poses)

    def object_mask(self, poses=None, dt=None):
        """Engine.object_mask_async on the resident frames (engine.set_object_mask first): in front of localize with the
        frames' poses and dt, or behind the pass without either.  Returns nothing; engine.object_mask() fetches the bits."""
        return self.engine.object_mask_async(poses, dt)

    def ground(self, triples=None):
        """Engine.ground_async on the resident frames (engine.set_ground first): behind the upload or ingest and in front of
        object_mask and localize, and again behind a crop or the sweeps.  Returns nothing; engine.ground() fetches the
        planes, the info words and the bits."""
        return self.engine.ground_async(triples)

    def occupancy_maps(self, batch=None, logodds=False):
        """Engine.occupancy_maps of the last occupancy_update."""
        return self.engine.occupancy_maps(batch, logodds)

    def inflated_costmaps(self, batch=None, clearance=False):
        """Engine.inflated_costmaps of the pass that has just run (engine.set_inflation(cfg, "costmap") first)."""
        return self.engine.inflated_costmaps(batch, clearance)

    def inflated_occupancy_maps(self, batch=None, clearance=False):
        """Engine.inflated_occupancy_maps of the last occupancy_update (engine.set_inflation(cfg, "occupancy") first)."""
        return self.engine.inflated_occupancy_maps(batch, clearance)

    def plan(self, goals, source="costmap", starts=None):
        """Engine.plan: the paths in metres to `goals` over the inflated grids of the pass that has just run, or of the
        last occupancy_update (engine.set_inflation and engine.set_navfn for that source first)."""
        return self.engine.plan(goals, source, starts)

    def drive(self, goals, velocities, limits, source="costmap", poses=None):
        """Engine.drive: the velocity commands in m/s and rad/s towards `goals` over the inflated grids of the pass that has
        just run, or of the last occupancy_update (engine.set_inflation, engine.set_navfn and engine.set_local_planner for
        that source first; engine.set_local_movers to avoid the streams' moving tracks too, engine.set_local_footprint to roll
        the robot as an oriented polygon instead of a point)."""
        return self.engine.drive(goals, velocities, limits, source, poses)

    def explore(self, source="occupancy"):
        """Engine.explore: the ranked exploration goals in metres per stream (None where a stream has no frontier) over the
        inflated grids of the pass that has just run, or of the last occupancy_update (engine.set_inflation and
        engine.set_frontier for that source first, and engine.set_navfn when its FrontierConfig has use_field set)."""
        return self.engine.explore(source)

    def _need_p2(self, p2, who):
        if self.d.project_bbox and p2 is None:
            raise ValueError(f"{who}: model.second.project_bbox is on: pass p2 (the frames' camera matrices)")

    # net.load_weights (train.py:731-734).  Accepts a dict name -> array (Keras layouts, weights.py), an .npz written by
    # weights.save_npz, or the reference's own checkpoint file (`model_weights_<epoch>.h5`, Keras save_weights,
    # train.py:407,436: weights.load_keras_h5, with h5py when it is installed and the built-in reader otherwise).
    def load_weights(self, src):
        w = _weights.load_any(src, self.d) if isinstance(src, (str, os.PathLike)) else src
        if self.training:
            if self.trainer is None:
                self.trainer = Trainer(self.config, w, **self._ctor, **self._train_kw)
                self.engine = self.trainer.engine
            else:
                self.trainer.set_weights(w)
            return
        self.engine.load_weights(w)

    def __call__(self, voxels, num_points, coors, batch_anchors, labels=None, reg_targets=None):
        if self.training:
            if labels is None or reg_targets is None:
                raise ValueError("training mode needs labels and reg_targets (model/voxelnet.py:850)")
            return self.train_step(self._unpad(_np(voxels), _np(num_points), _np(coors), int(_np(batch_anchors).shape[0])),
                                   _np(labels), _np(reg_targets), apply=False)
        if labels is not None or reg_targets is not None:
            raise ValueError("labels / reg_targets are training inputs: build the net with training=True")
        if not self.engine.weights_loaded:
            raise RuntimeError("VoxelNet: load_weights() has not been called")
        batch = int(_np(batch_anchors).shape[0])
        return self.engine.forward_voxels(_np(voxels), _np(num_points), _np(coors), batch)

    call = __call__

    # ---- training mode ----
    @staticmethod
    def _unpad(voxels, num_points, coors, batch):
        """Padded [P,T,F] + num_points + coors[b,z,y,x] -> per-frame point lists in pillar order."""
        frames = []
        for b in range(batch):
            rows = np.nonzero(coors[:, 0] == b)[0]
            frames.append(np.concatenate([voxels[p, :num_points[p]] for p in rows], axis=0).astype(np.float32)
                          if len(rows) else np.zeros((0, voxels.shape[2]), np.float32))
        return frames

    def train_step(self, frames, labels=None, reg_targets=None, dist=None, apply=True, gt_boxes=None, gt_classes=None,
                   gt_valid=None):
        """Forward (training mode) + loss + backward on raw clouds; apply=True also runs the optimizer step.
        Targets: exactly one of labels + reg_targets (dense, per anchor) or gt_boxes (per frame [G_b, 7], with
        gt_classes per frame or None: all 1; assigned on the GPU).  With augmentation on (VoxelNet(..., augment=True,
        seed=...)) the frames and boxes are augmented on the GPU first; gt_valid marks the boxes that are only obstacles.
        Returns the reference's loss scalars
        (model/voxelnet.py:1032-1043); a net built with metrics=True adds "metrics", the reference's update_metrics dict."""
        if self.trainer is None:
            raise RuntimeError("VoxelNet(training=True): load_weights() with the initial values first")
        dense = labels is not None or reg_targets is not None
        if dense == (gt_boxes is not None):
            raise ValueError("train_step needs exactly one of labels + reg_targets or gt_boxes")
        if dense and (labels is None or reg_targets is None):
            raise ValueError("train_step: labels and reg_targets go together")
        out = self.trainer.forward_backward(frames, labels, reg_targets, gt_boxes=gt_boxes, gt_classes=gt_classes,
                                            gt_valid=gt_valid)
        if apply:
            self.apply_gradients(dist)
        if self._train_kw["metrics"]:      # the reference's update_metrics dict over the steps so far (Trainer.metrics)
            out = dict(out)
            out["metrics"] = self.trainer.metrics(dist)
        return out

    def set_trainable(self, trainable):
        """The reference's set_trainable(net, trainable) (train.py:62-113) on a training net after load_weights():
        False freezes the PFN and rpn/block<b>/0..2 for the following steps, True unfreezes everything
        (Trainer.set_trainable)."""
        if not self.training:
            raise ValueError("set_trainable is a training option: build the net with training=True")
        if self.trainer is None:
            raise RuntimeError("VoxelNet(training=True): load_weights() with the initial values first")
        self.trainer.set_trainable(trainable)

    def apply_gradients(self, dist=None):
        """optimizer.apply_gradients (train.py:301) on the flat buffers, after the data-parallel all-reduce."""
        self.trainer.apply_gradients(dist)      # ends with a stream synchronisation (see Trainer.apply_gradients)

    def get_weights(self):
        return self.trainer.weights() if self.training else None

    def predict(self, example, preds_dict):
        rect, trv2c = _np(example[3]), _np(example[4])
        mask, img_idx = _np(example[7]), _np(example[8])
        batch = int(_np(example[6]).shape[0])
        dirp = _np(preds_dict["dir_cls_preds"]) if self.d.use_direction_classifier else None
        # model.second.project_bbox: "bbox" is the projection by example[5] (P2), as upstream SECOND's predict()
        p2 = _np(example[5]) if self.d.project_bbox else None
        self._need_p2(p2, "predict")
        dets, n = self.engine.predict(_np(preds_dict["box_preds"]), _np(preds_dict["cls_preds"]), dirp, mask, rect, trv2c, p2=p2)
        bb = self._bboxes(batch)
        return [self._to_dict(dets[b], int(n[b]), img_idx[b], None if bb is None else bb[b]) for b in range(batch)]

    def _detector(self):
        """What detects: the engine, or -- training mode -- the trainer, whose current weights are published first."""
        if not self.training:
            return self.engine
        if self.trainer is None:
            raise RuntimeError("VoxelNet(training=True): load_weights() with the initial values first")
        if self.trainer._prefetched is not None:
            raise RuntimeError("VoxelNet.detect: a prefetched training batch is pending; run its step first")
        self.trainer.publish()
        return self.trainer

    def _dicts(self, dets, n, batch, image_idx):
        """The prediction dicts of the pass that has just run.  With tracking on (model.second.tracking, or
        engine.set_tracking) each carries "track_id" ([n] int32, -1 for a row without a track) and "velocity" ([n, 3] float64,
        the matched track's; zeros for none) -- None, like the other values, when nothing survives."""
        bb = self._bboxes(batch)
        idx = image_idx if image_idx is not None else list(range(batch))
        out = [self._to_dict(dets[b], int(n[b]), idx[b], None if bb is None else bb[b]) for b in range(batch)]
        if isinstance(self.engine, Engine) and self.engine.tracking_on:
            tr, nt, _ = self.engine.tracks(batch)
            for b, o in enumerate(out):
                k = int(n[b])
                o["track_id"] = _tracking.det_track_ids(tr[b], nt[b], k) if k else None
                o["velocity"] = _tracking.det_track_velocity(tr[b], nt[b], k) if k else None
        return out

    def detect(self, frames, rect=None, trv2c=None, image_idx=None, p2=None, stamps=None):
        """Fused path: list of raw clouds -> list of prediction dicts.  p2 ([4,4] or [B,4,4]): required with
        model.second.project_bbox, which puts the projected image boxes into "bbox".  stamps (tracking on): the frames'
        time stamps in seconds (Engine.detect)."""
        self._need_p2(p2, "detect")
        on = self.d.project_bbox
        dets, n = self._detector().detect(frames, rect, trv2c, p2=p2 if on else None, bbox=on, stamps=stamps)
        return self._dicts(dets, n, len(frames), image_idx)

    def detect_pointcloud2(self, msgs, rect=None, trv2c=None, image_idx=None, p2=None, features=None, mount=None, first=1,
                           decimate=4, stamps=None):
        """Fused path from raw sensor_msgs/PointCloud2 messages (the reference's production mode: ingest on the GPU,
        Engine.detect_pointcloud2) -> the same list of prediction dicts as `detect`; p2 as there.  features / mount / first /
        decimate as Engine.ingest_pointcloud2: a model with 4 point features takes its intensity column from the messages'
        own field (features=[ingest.FeatureField("intensity")]), a lidar the identity mount."""
        self._need_p2(p2, "detect_pointcloud2")
        self._detector()
        if self.d.project_bbox:
            self.engine.set_projection(np.broadcast_to(np.asarray(p2, np.float64), (len(msgs), 4, 4)))
        dets, n = self.engine.detect_pointcloud2(msgs, rect, trv2c, features=features, mount=mount, first=first, decimate=decimate,
                                                 stamps=stamps)
        return self._dicts(dets, n, len(msgs), image_idx)

    def detect_depth(self, images, intrinsics, rect=None, trv2c=None, image_idx=None, p2=None, stamps=None):
        """Fused path from raw depth images (sensor_msgs/Image, 16UC1 or 32FC1) and the camera's intrinsics
        (Engine.detect_depth: deprojection and ingest on the GPU) -> the same list of prediction dicts as
        `detect_pointcloud2` on the messages a point-cloud node computes from those images; p2 as in `detect`."""
        self._need_p2(p2, "detect_depth")
        self._detector()
        if self.d.project_bbox:
            self.engine.set_projection(np.broadcast_to(np.asarray(p2, np.float64), (len(images), 4, 4)))
        dets, n = self.engine.detect_depth(images, intrinsics, rect, trv2c, stamps=stamps)
        return self._dicts(dets, n, len(images), image_idx)

    def _detect_rig(self, who, frames, rig, rect, trv2c, image_idx, p2, **feed):
        self._need_p2(p2, who)
        self._detector()
        if self.d.project_bbox:
            self.engine.set_projection(np.broadcast_to(np.asarray(p2, np.float64), (len(frames), 4, 4)))
        dets, n = getattr(self.engine, who)(frames, rig, rect, trv2c, **feed)
        return self._dicts(dets, n, len(frames), image_idx)

    def detect_rig_depth(self, frames, rig, rect=None, trv2c=None, image_idx=None, p2=None, stamps=None):
        """Fused path from the depth images of a camera rig (Engine.detect_rig_depth: every frame holds the points of all
        its cameras, each under its own mount -- ingest.CameraRig) -> the same list of prediction dicts as `detect` on
        the host-concatenated frames; p2 as there."""
        return self._detect_rig("detect_rig_depth", frames, rig, rect, trv2c, image_idx, p2, stamps=stamps)

    def detect_rig_pointcloud2(self, frames, rig, rect=None, trv2c=None, image_idx=None, p2=None, features=None, stamps=None):
        """`detect_rig_depth` for the PointCloud2 messages of a camera rig (Engine.detect_rig_pointcloud2); features as
        Engine.ingest_rig_pointcloud2."""
        return self._detect_rig("detect_rig_pointcloud2", frames, rig, rect, trv2c, image_idx, p2, features=features, stamps=stamps)

    @staticmethod
    def _to_dict(dets, n, img_idx, bbox=None):
        # model/voxelnet.py:1362-1379: all-None dict (except batch_idx) when nothing survives
        if n == 0:
            return {"bbox": None, "box3d_camera": None, "box3d_lidar": None, "scores": None,
                    "label_preds": None, "batch_idx": img_idx}
        d = dets[:n]
        return {
            # the placeholder of model/voxelnet.py:1357-1360, or (model.second.project_bbox) the projected rows
            "bbox": np.tile(np.array([[400., 200., 500., 400.]]), (n, 1)) if bbox is None else np.array(bbox[:n], np.float64),
            "box3d_camera": d["box3d_camera"].copy(),
            "box3d_lidar": d["box3d_lidar"].copy(),
            "scores": d["score"].copy(),
            "label_preds": d["label"].astype(np.int64),
            "batch_idx": img_idx,
        }
