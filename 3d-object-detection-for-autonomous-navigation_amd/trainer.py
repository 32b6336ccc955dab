"""Training loop body of train.py:228-304 on the HIP engine.

    trainer = Trainer(config, weights, max_batch=2)            # one per GPU / rank
    out = trainer.step(frames, labels, reg_targets, dist)      # forward + loss + backward, all-reduce, AdamW
    out = trainer.step(frames, gt_boxes=boxes, dist=dist)      # ... with the targets assigned on the GPU from the boxes
    trainer = Trainer(config, weights, augment=True, seed=0)   # ... and the frames augmented on the GPU first
    trainer.weights()                                          # Keras-layout dict (Engine.load_weights, save_npz)
    trainer = Trainer(config, weights, frozen="reference")     # fine-tuning with the early layers frozen
    trainer.set_trainable(False)                               # ... the reference's set_trainable(net, False)
    trainer = Trainer(config, weights, metrics=True)           # every step counts accuracy / precision / recall on the GPU
    trainer.metrics(dist)                                      # ... the reference's update_metrics dict (metrics.py)
    trainer = Trainer(config, weights, grad_clip=optim.GradClip("global_norm", 1.0, skip_nonfinite=True))
    trainer.grad_stats()                                       # ... the last step's gradient norm, scale, skip flag
    dets, n = trainer.detect(frames)                           # detect with the CURRENT weights (published on the GPU)

What runs where: the frames are uploaded and voxelised by the engine, `pp_train_step` (csrc/train.hip) runs the
training-mode forward pass, the loss and the backward pass and leaves the gradients of all trainable tensors in one
flat float32 buffer; that buffer is averaged over the ranks with ONE all-reduce (`torch.distributed`, backend
"nccl" = RCCL over xGMI; BatchNorm statistics stay per replica, as in the single-GPU reference) and consumed by the
AdamW kernel (csrc/optim.hip).  torch owns the flat device buffers and the communicator; no torch operator touches
the numbers.  Labels / regression targets come either from `target_assigner` on the host (the reference's training
dataloader) or, given the ground-truth boxes (`gt_boxes=`), from the same assignment on the GPU between the forward and
the backward half of the step (csrc/targets.hip).  With `augment` on, a step given boxes first augments the frames
and the boxes on the GPU as the reference's training loader does (csrc/augment.hip, augment.py); the random numbers
are drawn from the trainer's own RandomState (`seed`) in the reference's order.

Frozen layers (`frozen=`, `set_frozen`, `set_trainable`): the reference's second training stage loads a checkpoint and
fine-tunes it with the early layers frozen (train.py:62-113 set_trainable, :356-368).  A freeze unit is the PFN
("pfn"), one separable layer with its BatchNorm ("rpn/block<b>/<j>"), one transposed convolution ("rpn/deconv<b>") or
one head ("rpn/conv_box", "rpn/conv_cls", "rpn/conv_dir_cls").  A frozen unit behaves as a Keras layer with
trainable = False does in TF 2.x: its BatchNorm normalises with the moving statistics even in the training step and does
not update them, its tensors get no gradient (their entries of the flat gradient buffer are 0) and AdamW neither updates
nor decays them.  The gradient still flows through a frozen unit to trainable units in front of it.  These are the
documented Keras semantics; the reference flips `trainable` after its tf.function was first traced, and whether TF 2.2
re-traces at that point has not been checked against a TF run.

Gradient clipping (`grad_clip=`): the lines trainStep carries commented out above optimizer.apply_gradients
(train.py:293-294) and the non-finite step guard, inside the optimizer step (optim.GradClip, csrc/grad_clip.hip).  The
norm is taken AFTER the all-reduce, from the averaged buffer, so every rank takes the same decision; only the trainable
tensors take part.  The clipped gradient exists inside the update kernel only: `grads` / gradients() keep the raw values
and grad_stats() says which scale was applied.  A skipped step (guard on, a NaN or Inf gradient) leaves parameters,
moments and the optimizer's step count as they were and is counted in `steps_skipped`.

Detection during training (`detect`, `publish`): the reference evaluates with the current weights after every epoch
(train.py:403-444).  `publish()` folds the flat `params` / `state` buffers into the engine's inference weights on the GPU
(csrc/weight_publish.hip) -- the bytes `engine.load_weights(trainer.weights())` would leave, without the host round trip,
written in place so the captured inference graphs survive -- and does nothing while the weights have not changed since
the last publish.  `detect()` publishes when needed and is `Engine.detect`; training is not disturbed by it.
"""
import numpy as np

from . import optim
from .engine import Engine


def train_units(d):
    """Every freeze unit of config `d` (config.Derived), in the order of the network."""
    from . import weights as _w
    return ["pfn"] + [name for _, name, _ in _w.layer_table(d)]


def unit_of(tensor_name):
    """The freeze unit a tensor of the layout belongs to: "rpn/block2/3/bn/gamma" -> "rpn/block2/3"."""
    parts = tensor_name.split("/")
    if parts[0] == "pfn":
        return "pfn"
    return "/".join(parts[:3] if parts[1].startswith("block") else parts[:2])


def reference_frozen_units(d):
    """The units set_trainable(net, False) freezes (train.py:62-113): the PFN's Dense, BatchNorm and ReLU
    (net.layers[1].layers[0].layers[0..2]) and, in each RPN block, layers 0..9 -- ZeroPadding and the first three
    (SeparableConv2D, BatchNorm, ReLU) triples, i.e. rpn/block<b>/0..2.  A block with fewer than three separable layers
    (layer_nums[b] < 2) makes the reference raise IndexError; this raises ValueError."""
    for b, n in enumerate(d.layer_nums):
        if n < 2:
            raise ValueError(f"the reference's set_trainable needs layer_nums[{b}] >= 2 (block{b + 1} has {n + 1} "
                             f"separable layers, it indexes layers 0..9 of the block)")
    return ["pfn"] + [f"rpn/block{b + 1}/{j}" for b in range(3) for j in range(3)]


def trainable_segments(layout, frozen):
    """(offset, size) ranges of the parameter buffer that hold the tensors of units not in `frozen`, merged where
    they touch (layout: Engine.train_layout()'s entries)."""
    fz = set(frozen)
    segs = []
    for name, off, size, is_state in layout:
        if is_state or unit_of(name) in fz:
            continue
        if segs and segs[-1][0] + segs[-1][1] == off:
            segs[-1][1] += size
        else:
            segs.append([off, size])
    return [tuple(s) for s in segs]


def trainable_tensor_segments(layout, frozen):
    """One (offset, size) segment per trainable tensor, unmerged, and the tensors' names: the groups of per-tensor
    clipping (optim.GradClip("norm"))."""
    fz = set(frozen)
    keep = [(name, off, size) for name, off, size, is_state in layout if not is_state and unit_of(name) not in fz]
    return [(off, size) for _, off, size in keep], [name for name, _, _ in keep]


def resolve_frozen(d, frozen):
    """None / () -> (); "reference" -> reference_frozen_units(d); an iterable of unit names -> those, in network order.
    ValueError for an unknown or repeated name and when every unit would be frozen."""
    if frozen is None:
        return ()
    if isinstance(frozen, str):
        if frozen != "reference":
            raise ValueError(f"frozen: None, 'reference' or an iterable of unit names, not {frozen!r}")
        frozen = reference_frozen_units(d)
    names = list(frozen)
    units = train_units(d)
    for n in names:
        if not isinstance(n, str) or n not in units:
            raise ValueError(f"unknown freeze unit {n!r} (units: {', '.join(units)})")
    if len(set(names)) != len(names):
        raise ValueError(f"a freeze unit is named twice: {names}")
    if names and len(names) == len(units):
        raise ValueError("every unit frozen: nothing left to train")
    return tuple(u for u in units if u in names)


class TrainBatch:
    """Page-locked staging of one training batch (Trainer.stage)."""

    labels = reg_targets = None          # stage(): the dense targets
    gt = None                            # stage_gt(): (boxes, classes or None, counts) as Engine.pack_gt lays them out
    aug = None                           # stage_gt() of an augmenting trainer: (valid flags or None, augment.Draws)
    cand = None                          # stage_gt() of a sampling trainer: the gt_sampler.Candidates

    def close(self):
        for k in ("points", "_lab", "_reg", "_gtb", "_gtc", "_gtn", "_gtv", "_aug_frames", "_aug_boxes", "_cands", "_candn"):
            o = getattr(self, k, None)
            if o is not None:
                o.close()
                setattr(self, k, None)
        self.labels = self.reg_targets = self.gt = self.aug = self.cand = None


class Trainer:
    def __init__(self, config, weights, max_batch=None, max_points_per_frame=32768, device=0, learning_rate=None,
                 weight_decay=None, augment=None, seed=None, frozen=None, gt_database=None, sampler=None, metrics=False,
                 grad_clip=None):
        import random
        import torch
        from . import augment as _augment
        from . import gt_sampler as _gts
        # sampler: None / False = off; True = the config's train_input_reader keys (the shipped values without them);
        # a gt_sampler.SamplerConfig = those settings.  It needs gt_database (a gt_sampler.GtDatabase) and the reverse:
        # no configuration key turns sampling on by itself.
        if sampler is True:
            tir = config.get("train_input_reader") if isinstance(config, dict) else None
            sampler = _gts.SamplerConfig.from_input_reader(tir)
            if sampler is None:
                raise ValueError("sampler=True, but train_input_reader switches sampling off (sample_classes: None)")
        elif sampler is False:
            sampler = None
        elif sampler is not None and not isinstance(sampler, _gts.SamplerConfig):
            raise ValueError("sampler: None, True or a gt_sampler.SamplerConfig")
        if (sampler is None) != (gt_database is None):
            raise ValueError("sampler and gt_database go together: pass both or neither")
        if gt_database is not None and not isinstance(gt_database, _gts.GtDatabase):
            raise ValueError("gt_database: a gt_sampler.GtDatabase is required")
        if augment is not None and augment is not False and sampler is not None:
            ac = augment if isinstance(augment, _augment.AugmentConfig) else _augment.AugmentConfig.from_input_reader(
                config.get("train_input_reader") if isinstance(config, dict) else None)
            if ac.global_rot_per_object:
                raise ValueError("sampler with global_random_rotation_range_per_object: those draws depend on the box, "
                                 "which the sampler chooses on the GPU")
        self.sampler, self.gt_database = sampler, gt_database
        self.pyrandom = random.Random(seed)
        self.frames_left_without_boxes = 0     # frames without boxes whose sampling rounds all failed (counted per step)
        self._boxless = None
        # augment: None / False = off; True = the config's train_input_reader keys (the shipped values without them);
        # an augment.AugmentConfig = those settings
        if augment is True:
            tir = config.get("train_input_reader") if isinstance(config, dict) else None
            augment = _augment.AugmentConfig.from_input_reader(tir)
        elif augment is False:
            augment = None
        elif augment is not None and not isinstance(augment, _augment.AugmentConfig):
            raise ValueError("augment: None, True or an augment.AugmentConfig")
        self.augment = augment
        # grad_clip: None / False = off; True = train_config.gradient_clipping (an error when the key is absent); an
        # optim.GradClip = those settings.  No configuration key turns it on by itself.
        if grad_clip is True:
            tcfg = config.get("train_config") if isinstance(config, dict) else None
            grad_clip = optim.GradClip.from_config(tcfg)
            if grad_clip is None:
                raise ValueError("grad_clip=True, but train_config has no gradient_clipping key")
        elif grad_clip is False:
            grad_clip = None
        elif grad_clip is not None and not isinstance(grad_clip, optim.GradClip):
            raise ValueError("grad_clip: None, True or an optim.GradClip")
        self.grad_clip = grad_clip
        self.grad_groups = None      # with per-tensor norms: the tensor name of each group of grad_stats()["norms"]
        self.steps_skipped = 0       # steps the non-finite guard left without an update
        self._grad_stats = None
        self._stats_host = None      # page-locked copy of the statistics block, filled behind the update
        self._stats_pinned = None
        self._stats_pending = False
        self.rs = np.random.RandomState(seed)
        self.torch = torch
        self.engine = Engine(config, max_batch=max_batch, max_points_per_frame=max_points_per_frame, device=device)
        if gt_database is not None:
            self.engine.load_gt_database(gt_database)
        self._prefetched = None      # the TrainBatch whose points are already on their way (forward_backward(prefetch=))
        self._dirty = True           # params / state changed since the last publish() (set_weights, every step and update)
        self._ext_stream = None      # torch.cuda.ExternalStream over the engine's stream (_engine_stream)
        self.time_allreduce = False  # True: every step's gradient all-reduce is bracketed by an event pair (allreduce_ms)
        self._allreduce_events = []
        d = self.engine.d
        self.layout, n_params, n_state = self.engine.train_layout()
        self.device = torch.device("cuda", device)
        self.params = torch.zeros(n_params, dtype=torch.float32, device=self.device)
        self.grads = torch.zeros_like(self.params)
        self.state = torch.zeros(n_state, dtype=torch.float32, device=self.device)
        self.set_weights(weights)
        # train_config absent: the shipped YAML's values (configs/train.yaml: learning rate 2e-4, weight decay 1e-4).
        # train_config present but without the keys train.py:224-239 reads: an error, not a silent default.
        tc = config.get("train_config") if isinstance(config, dict) else None
        if learning_rate is None:
            if tc:
                try:
                    learning_rate = optim.ExponentialDecay.from_config(tc, max_batch or d.batch_size)
                except (KeyError, TypeError) as ex:
                    raise ValueError(f"train_config: learning-rate schedule keys missing or malformed ({ex!r})") from ex
            else:
                learning_rate = 2e-4
        if weight_decay is None:
            if tc:
                try:
                    weight_decay = float(tc["optimizer"]["adam_optimizer"]["weight_decay"])
                except (KeyError, TypeError) as ex:
                    raise ValueError(f"train_config: optimizer.adam_optimizer.weight_decay missing or malformed ({ex!r})") from ex
            else:
                weight_decay = 1e-4
        self.optimizer = optim.AdamW(self.params, learning_rate, weight_decay)
        self._frozen = ()
        self.set_frozen(frozen)
        # metrics: True = every step counts the reference's monitoring metrics on the GPU (csrc/metrics.hip) and feeds a
        # metrics.TrainMetrics; no configuration key turns it on.  metrics_steps is how often the reference's loop would
        # report them (train_config.net_metrics_steps, 500 in the shipped YAML): informational
        from . import metrics as _metrics
        self.metrics_steps = int(tc["net_metrics_steps"]) if tc and "net_metrics_steps" in tc else 500
        self._metrics = _metrics.TrainMetrics() if metrics else None
        if metrics:
            self.engine.set_train_metrics(True)

    # ---- frozen layers (the reference's set_trainable) ----
    @property
    def frozen(self):
        """The frozen units, in network order (() = everything trains)."""
        return self._frozen

    def set_frozen(self, units):
        """Freeze `units` for the following steps: None / () = train everything, "reference" = the selection of the
        reference's set_trainable(net, False), or an iterable of unit names (train_units).  Parameters, moving
        statistics and AdamW moments of the units are kept as they are; unfreezing continues from them."""
        names = resolve_frozen(self.engine.d, units)
        self.engine.train_set_frozen(names)
        self._frozen = names
        self.optimizer.set_segments(trainable_segments(self.layout, names) if names else None)
        if self.grad_clip is not None:      # segments and groups of the clipped step follow the freeze
            self._drop_stats_buffer()
            if self.grad_clip.mode == "norm":
                segs, self.grad_groups = trainable_tensor_segments(self.layout, names)
                self.optimizer.set_segments(segs)
                self.optimizer.set_clip(self.grad_clip, np.arange(len(segs), dtype=np.int32))
            else:
                self.optimizer.set_segments(trainable_segments(self.layout, names))
                self.optimizer.set_clip(self.grad_clip)

    def set_trainable(self, trainable):
        """The reference's set_trainable(net, trainable) (train.py:62-113): False freezes its selection (the PFN and
        rpn/block<b>/0..2, reference_frozen_units), True unfreezes everything."""
        self.set_frozen(None if trainable else "reference")

    # ---- Keras-layout dict <-> flat buffers ----
    def set_weights(self, w):
        self._dirty = True
        p = np.zeros(self.params.numel(), np.float32)
        s = np.zeros(self.state.numel(), np.float32)
        for name, off, size, is_state in self.layout:
            a = np.ascontiguousarray(w[name], dtype=np.float32).reshape(-1)
            if a.size != size:
                raise ValueError(f"weight {name!r}: {a.size} values, the layout expects {size}")
            (s if is_state else p)[off:off + size] = a
        self.params.copy_(self.torch.from_numpy(p))
        self.state.copy_(self.torch.from_numpy(s))

    def _unflatten(self, flat_params, flat_state, like):
        out = {}
        for name, off, size, is_state in self.layout:
            src = flat_state if is_state else flat_params
            out[name] = src[off:off + size].reshape(like[name].shape).copy()
        return out

    def weights(self):
        """Every tensor (frozen ones included) as a Keras-layout dict under its usual name.  The reference brackets its
        save_weights with set_trainable(True) / set_trainable(False) (train.py:406-408) only to keep Keras's variable
        order stable; names here do not depend on the freeze, so nothing of the kind is needed."""
        from . import weights as _w
        shapes = _w.expected_shapes(self.engine.d)
        like = {k: np.empty(v, np.float32) for k, v in shapes.items()}
        return self._unflatten(self.params.cpu().numpy(), self.state.cpu().numpy(), like)

    def gradients(self):
        """The last step's gradients as a Keras-layout dict (trainable tensors only: the tensors of frozen units are
        left out, as they are not among net.trainable_variables; their entries of `grads` are 0).  With grad_clip on
        these are still the RAW gradients: clipping happens inside the update kernel, grad_stats() reports the scales."""
        from . import weights as _w
        shapes = _w.expected_shapes(self.engine.d)
        g = self.grads.cpu().numpy()
        fz = set(self._frozen)
        return {name: g[off:off + size].reshape(shapes[name]).copy() for name, off, size, st in self.layout
                if not st and unit_of(name) not in fz}

    def decisions(self):
        """Parity tap (pp_train_fetch_decisions): what the last step decided at its non-differentiable points.
        {"pfn": int32 [batch, max_voxels, C] winning row of every pillar slot (-1 a padded row, -2 no gradient),
         "<layer>/bn": bool mask of the layer's ReLU in NCHW order (as a torch graph of the network holds the tensor)}
        for every separable layer and transposed convolution, forward order."""
        import ctypes
        from . import weights as _w
        eng = self.engine
        d = eng.d
        L = eng._lib

        def fetch(layer, itemsize):
            n = ctypes.c_int64(0)
            eng._check(L.pp_train_fetch_decisions(eng._h, layer, None, 0, ctypes.byref(n)), "pp_train_fetch_decisions")
            buf = np.empty(n.value * itemsize, np.uint8)
            eng._check(L.pp_train_fetch_decisions(eng._h, layer, buf.ctypes.data_as(ctypes.c_void_p), buf.size,
                                                  ctypes.byref(n)), "pp_train_fetch_decisions")
            return buf
        out = {}
        arg = fetch(-1, 4).view(np.int32)
        out["pfn"] = arg.reshape(-1, d.max_voxels, d.pfn_filters)
        B = out["pfn"].shape[0]
        k = 0
        for kind, name, s in _w.layer_table(d):
            if kind == "head":
                continue
            m = fetch(k, 1).astype(bool)
            k += 1
            if kind == "sep":
                out[name + "/bn"] = m.reshape(B, -1, s["cout"])             # [b][pixels][c]; the caller knows H x W
            else:
                out[name + "/bn"] = m.reshape(B, -1, s["k"], s["k"], s["cout"])   # [b][input pixels][ti][tj][c]
        return out

    # ---- one optimizer step ----
    def stage(self, frames, labels, reg_targets):
        """A training batch in page-locked host memory: the points as an engine Staging, labels / regression targets
        as pinned arrays (`.labels`, `.reg_targets`: refill them in place for the next batch of the same shape).  A
        staged batch goes to the GPU as three DMA transfers; ordinary numpy arrays take the runtime's pageable path
        (an extra host copy of ~0.5 MB per frame at the shipped configuration)."""
        d = self.engine.d
        B = len(frames)
        st = TrainBatch()
        st.points = self.engine.staging(frames)
        st._lab = self.engine.pinned((B, d.num_anchors), np.int32)
        st._reg = self.engine.pinned((B, d.num_anchors, 7), np.float32)
        st.labels, st.reg_targets = st._lab.array, st._reg.array
        st.labels[...] = np.asarray(labels, dtype=np.int32).reshape(B, d.num_anchors)
        st.reg_targets[...] = np.asarray(reg_targets, dtype=np.float32).reshape(B, d.num_anchors, 7)
        return st

    def stage_gt(self, frames, gt_boxes, gt_classes=None, gt_valid=None, draws=None):
        """stage() with ground-truth boxes instead of dense targets: the points as an engine Staging, the boxes (per frame
        [G_b, 7]), their classes (per frame [G_b], or None: all 1) and the per-frame counts packed into page-locked
        arrays (`.gt`).  The step assigns the targets on the GPU (csrc/targets.hip).  On an augmenting trainer the batch
        also holds its augmentation draws (`draws`, or drawn here from the trainer's RandomState) and the valid flags."""
        boxes, cls, counts = self.engine.pack_gt(gt_boxes, gt_classes)
        if len(counts) != len(frames):
            raise ValueError(f"{len(frames)} frames but boxes for {len(counts)}")
        st = TrainBatch()
        st.points = self.engine.staging(frames)
        st._gtb = self.engine.pinned(boxes.shape, np.float32)
        st._gtb.array[...] = boxes
        st._gtn = self.engine.pinned(counts.shape, np.int32)
        st._gtn.array[...] = counts
        if cls is not None:
            st._gtc = self.engine.pinned(cls.shape, np.int32)
            st._gtc.array[...] = cls
        st.gt = (st._gtb.array, st._gtc.array if cls is not None else None, st._gtn.array)
        if self.sampler is not None:
            cand = self._draw_candidates(gt_boxes, gt_classes)
            from . import gt_sampler as _gts
            st._cands = self.engine.pinned(cand.cands.shape, _gts.CAND_DTYPE)
            st._cands.array[...] = cand.cands
            st._candn = self.engine.pinned(cand.counts.shape, np.int32)
            st._candn.array[...] = cand.counts
            st.cand = _gts.Candidates(st._cands.array, st._candn.array)
        if self.augment is not None:
            if draws is None:
                draws = self._draw_augment(gt_boxes, st.cand)
            # the draws in page-locked memory next to the boxes: the step's copies are DMA transfers
            from . import augment as _augment
            if gt_valid is not None:
                v = np.concatenate([np.asarray(x, bool).reshape(-1) for x in gt_valid]) if len(gt_valid) else \
                    np.zeros(0, bool)
                st._gtv = self.engine.pinned(v.shape, np.uint8)
                st._gtv.array[...] = v
                gt_valid = st._gtv.array
            st._aug_frames = self.engine.pinned(draws.flip.shape, _augment.FRAME_DTYPE)
            st._aug_frames.array[...] = draws.frames_struct()
            st._aug_boxes = self.engine.pinned(draws.boxes.shape, np.float64)
            st._aug_boxes.array[...] = draws.boxes
            draws = _augment.Draws(draws.flip, draws.theta, draws.scale, draws.t, draws.seed, st._aug_boxes.array,
                                   draws.counts, frames=st._aug_frames.array)
            st.aug = (gt_valid, draws)
        elif draws is not None:
            raise ValueError("draws need a trainer with augment on")
        elif gt_valid is not None:
            if self.sampler is None:
                raise ValueError("gt_valid needs a trainer with augment or sampler on")
            v = np.concatenate([np.asarray(x, bool).reshape(-1) for x in gt_valid] or [np.zeros(0, bool)])
            st._gtv = self.engine.pinned(v.shape, np.uint8)
            st._gtv.array[...] = v
            st.aug = (st._gtv.array, None)       # the flags ride through the sampling; no draws
        return st

    def _draw_candidates(self, gt_boxes, gt_classes):
        from . import gt_sampler as _gts
        cls = [np.ones(len(np.asarray(g).reshape(-1, 7)), np.int32) for g in gt_boxes] if gt_classes is None else gt_classes
        return _gts.draw_candidates(self.gt_database, cls, self.pyrandom)

    def _draw_augment(self, gt_boxes, cand):
        """The augmentation draws of a batch; on a sampling trainer for counts[b] + (slots of frame b's largest round)
        rows per frame, of which the step uses the first counts[b] + accepted."""
        from . import augment as _augment
        if cand is not None:
            extra = cand.counts.max(axis=1)
            gt_boxes = [np.concatenate([np.asarray(g, np.float64).reshape(-1, 7), np.zeros((int(x), 7))], 0)
                        for g, x in zip(gt_boxes, extra)]
        return _augment.draw(self.rs, gt_boxes, self.augment)

    def _enqueue_step(self, labels, reg_targets, gt, aug=None, cand=None):
        ptrs = (self.params.data_ptr(), self.grads.data_ptr(), self.state.data_ptr())
        self._boxless = None
        if cand is not None:
            valid, draws = aug if aug is not None else (None, None)
            self.engine.train_step_sample_async(*ptrs, *gt, valid, cand, self.sampler, draws, self.augment)
            self._boxless = np.flatnonzero(np.asarray(gt[2]) == 0)
        elif aug is not None:
            self.engine.train_step_aug_async(*ptrs, *gt, aug[0], aug[1], self.augment)
        elif gt is not None:
            self.engine.train_step_gt_async(*ptrs, *gt)
        else:
            self.engine.train_step_async(*ptrs, labels, reg_targets)

    def _launch(self, frames, labels, reg_targets, prefetch, gt_boxes=None, gt_classes=None, gt_valid=None):
        """Enqueue the step (and the upload of the next batch beside it); the caller waits with engine.train_step_wait().
        Targets: a TrainBatch's own (stage / stage_gt), else labels / reg_targets, else gt_boxes (+ gt_classes)."""
        self._dirty = True      # every step moves the BatchNorm statistics, whether or not an update follows
        if isinstance(frames, TrainBatch):
            tb = frames
            if gt_boxes is not None or gt_classes is not None:
                raise ValueError("a TrainBatch carries its own targets")
            if self._prefetched is not tb:
                self.engine.upload_async(tb.points)
            self._prefetched = None
            if self.augment is not None and tb.aug is None:
                raise ValueError("an augmenting trainer trains on stage_gt() batches (dense labels cannot follow moved boxes)")
            if self.sampler is not None and tb.cand is None:
                raise ValueError("a sampling trainer trains on stage_gt() batches (dense labels cannot follow pasted objects)")
            self._enqueue_step(tb.labels, tb.reg_targets, tb.gt, tb.aug, tb.cand)
            if isinstance(prefetch, TrainBatch):
                self.engine.upload_async(prefetch.points)
                self._prefetched = prefetch
            return
        gt = None
        if gt_boxes is not None:
            if labels is not None or reg_targets is not None:
                raise ValueError("pass either labels / reg_targets or gt_boxes, not both")
            gt = self.engine.pack_gt(gt_boxes, gt_classes)
            if len(gt[2]) != len(frames):
                raise ValueError(f"{len(frames)} frames but boxes for {len(gt[2])}")
        elif gt_classes is not None:
            raise ValueError("gt_classes needs gt_boxes")
        aug = cand = None
        if self.sampler is not None:
            if gt is None:
                raise ValueError("sampling needs gt_boxes= (dense labels cannot follow pasted objects)")
            cand = self._draw_candidates(gt_boxes, gt_classes)
        if self.augment is not None:
            if gt is None:
                raise ValueError("augmentation needs gt_boxes= (dense labels cannot follow moved boxes)")
            aug = (gt_valid, self._draw_augment(gt_boxes, cand))
        elif gt_valid is not None and cand is None:
            raise ValueError("gt_valid needs a trainer with augment or sampler on")
        elif gt_valid is not None:
            v = np.concatenate([np.asarray(x, bool).reshape(-1) for x in gt_valid] or [np.zeros(0, bool)])
            aug = (np.ascontiguousarray(v, np.uint8), None)      # the flags ride through the sampling; no draws
        self._prefetched = None
        self.engine.upload(frames)
        self._enqueue_step(labels, reg_targets, gt, aug, cand)

    def forward_backward(self, frames, labels=None, reg_targets=None, prefetch=None, gt_boxes=None, gt_classes=None,
                         gt_valid=None):
        """frames: a list of clouds with labels / reg_targets (or gt_boxes / gt_classes: the targets are then assigned
        on the GPU), or one TrainBatch from stage() / stage_gt().
        prefetch: the TrainBatch of the NEXT step -- its points go to the GPU (the handle's other input buffer, the copy
        stream) while this step's kernels run, the loader's hand-over of train.py:228-304; pass that same batch as
        `frames` of the next call."""
        self._launch(frames, labels, reg_targets, prefetch, gt_boxes, gt_classes, gt_valid)
        return self._wait()

    def _wait(self):
        losses = self.engine.train_step_wait()
        if self._boxless is not None and len(self._boxless):
            # frames that came without boxes: the sampler's rounds may all have failed (the reference would go on trying)
            used = self.engine.gt_sample_info()["round_used"]
            self.frames_left_without_boxes += int((used[self._boxless] < 0).sum())
        self._boxless = None
        if self._metrics is not None:
            self._metrics.update(self.engine.train_metrics_counts(), losses["cls_loss_reduced"], losses["loc_loss_reduced"])
        if self._stats_pending:      # step(): the update ran behind the backward pass, its statistics came along
            self._take_stats()
            gs = self._grad_stats      # (None: "value" without the guard measures nothing)
            losses["grad_norm"] = gs["global_norm"] if gs else None
            losses["step_skipped"] = bool(gs and gs["skipped"])
        return losses

    # ---- gradient clipping / non-finite guard (optim.GradClip) ----
    def _take_stats(self):
        """The statistics block of the update that has just been waited for; a skipped step gives the optimizer its
        step count back, so the next step runs with the learning rate this one would have had."""
        self._stats_pending = False
        if not self.grad_clip.needs_norm:
            self._grad_stats = None
            return
        self._grad_stats = optim.AdamW.decode_stats(self._stats_pinned.array)
        if self._grad_stats["skipped"]:
            self.optimizer.iterations -= 1
            self.steps_skipped += 1

    def set_grad_clip(self, grad_clip):
        """Switch clipping on a live trainer: an optim.GradClip, or None = off (the step is the unclipped calls again)."""
        if grad_clip is not None and not isinstance(grad_clip, optim.GradClip):
            raise ValueError("set_grad_clip: an optim.GradClip or None")
        self.grad_clip = grad_clip
        self.grad_groups = self._grad_stats = None
        self.optimizer.set_clip(None)
        self.set_frozen(self._frozen)

    def _drop_stats_buffer(self):
        """Frees the page-locked statistics copy (nothing may be in flight into it: callers have waited)."""
        self._stats_host, self._stats_pending = None, False
        if self._stats_pinned is not None:
            self._stats_pinned.close()
            self._stats_pinned = None

    def grad_stats(self):
        """The last waited step's gradient statistics: global_norm, scale, nonfinite, skipped, norms, scales (per
        group: one group, or one per trainable tensor -- `grad_groups` -- with GradClip("norm")).  The norms are those
        of the raw, all-reduced gradient over the trainable tensors.  None before the first update; a GradClip("value")
        without the guard measures nothing (None, too).  Needs Trainer(..., grad_clip=...)."""
        if self.grad_clip is None:
            raise RuntimeError("Trainer(..., grad_clip=...) takes the statistics; this trainer was built without")
        return self._grad_stats

    # ---- monitoring (the reference's update_metrics) ----
    def metrics(self, dist=None):
        """The reference's metrics dict (libraries/metrics.py:187-196: cls_loss, cls_loss_rt, loc_loss, loc_loss_rt,
        rpn_acc, prec@10, rec@10, ... rec@95) over the steps since the last reset_metrics(); with `dist`
        (torch.distributed) the totals of all ranks.  Needs Trainer(..., metrics=True)."""
        if self._metrics is None:
            raise RuntimeError("Trainer(..., metrics=True) counts the metrics; this trainer was built without")
        if dist is not None and dist.is_initialized() and dist.get_world_size() > 1:
            dev = self.device if dist.get_backend() == "nccl" else None
            return self._metrics.allreduce(dist, device=dev).result()
        return self._metrics.result()

    def reset_metrics(self):
        if self._metrics is None:
            raise RuntimeError("Trainer(..., metrics=True) counts the metrics; this trainer was built without")
        self._metrics.reset()

    def _engine_stream(self):
        """torch's view of the engine's own stream: the all-reduce and the AdamW kernel are enqueued THERE, behind the
        backward pass, so nothing needs a host round trip between trainStep's halves (and nothing can overtake)."""
        if self._ext_stream is None:
            self._ext_stream = self.torch.cuda.ExternalStream(self.engine.stream_ptr(), device=self.device)
        return self._ext_stream

    def _enqueue_update(self, dist):
        with self.torch.cuda.stream(self._engine_stream()):
            if self.time_allreduce:      # an event pair around the exchange alone, on the stream it runs on
                ev = (self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True))
                ev[0].record()
            optim.allreduce_gradients(self.grads, dist)        # one collective per step over the flat buffer
            if self.time_allreduce:
                ev[1].record()
                self._allreduce_events.append(ev)
            self.optimizer.apply_gradients(self.grads)
            if self.grad_clip is not None and self.grad_clip.needs_norm:
                words = self.optimizer.stats_words()
                if self._stats_host is None:
                    # the engine's own page-locked memory, not torch's: torch's host allocator would note the engine's
                    # stream against the block and record an event on it when the block is freed -- after close(), on a
                    # stream that no longer exists
                    self._stats_pinned = self.engine.pinned((words.numel(),), np.int32)
                    self._stats_host = self.torch.from_numpy(self._stats_pinned.array)
                self._stats_host.copy_(words, non_blocking=True)      # read at the wait the step has anyway
            self._stats_pending = self.grad_clip is not None

    def allreduce_ms(self):
        """Device time (ms) of each gradient exchange since `time_allreduce` was set (call after the steps were waited
        for); the list is emptied."""
        evs, self._allreduce_events = self._allreduce_events, []
        return [a.elapsed_time(b) for a, b in evs]

    def apply_gradients(self, dist=None):
        """optimizer.apply_gradients (train.py:301) after the data-parallel mean of the flat gradient buffer.  The
        all-reduce and the AdamW kernel run on the engine's stream (behind the step that produced the gradients); this
        returns when both are through, so a caller may read the parameters."""
        self._dirty = True
        self._enqueue_update(dist)
        self._engine_stream().synchronize()
        if self._stats_pending:
            self._take_stats()

    def step(self, frames, labels=None, reg_targets=None, dist=None, prefetch=None, gt_boxes=None, gt_classes=None,
             gt_valid=None):
        """One optimizer step: forward + loss + backward, gradient exchange, AdamW -- enqueued back to back on the engine's
        stream, ONE host wait at the end.  Targets as forward_backward takes them."""
        self._launch(frames, labels, reg_targets, prefetch, gt_boxes, gt_classes, gt_valid)
        try:
            self._enqueue_update(dist)
        except BaseException:
            # the step is in flight: wait for it (its own error is secondary) so the engine is not left "pending",
            # and forget the prefetch -- the next call uploads its batch itself
            self._abandon_step()
            raise
        return self._wait()

    # ---- detection with the current weights (the reference's per-epoch evaluation, train.py:403-444) ----
    def publish(self):
        """The engine's inference weights from `params` / `state`, on the GPU (Engine.publish_weights); nothing when
        they have not changed since the last publish.  Returns whether it published."""
        if not self._dirty:
            return False
        self.engine.publish_weights(self.params.data_ptr(), self.state.data_ptr())
        self._dirty = False
        return True

    def detect(self, frames, rect=None, trv2c=None, **kw):
        """Engine.detect(frames, rect, trv2c, **kw) with the trainer's current weights (publish() first when they
        changed).  Between steps only: a batch prefetched by forward_backward(prefetch=) is resident in the engine and
        the detection's upload would replace it."""
        if self._prefetched is not None:
            raise RuntimeError("Trainer.detect: a prefetched training batch is pending (forward_backward(prefetch=...)); "
                               "run its step first -- detect() would replace the resident points")
        self.publish()
        return self.engine.detect(frames, rect, trv2c, **kw)

    def _abandon_step(self):
        self._prefetched = None
        self._stats_pending = False
        try:
            self.engine.train_step_wait()
        except Exception:      # noqa: BLE001 -- the caller's exception is the one to report
            pass

    def close(self):
        self.engine.close()          # waits for the handle's streams
        self._drop_stats_buffer()
