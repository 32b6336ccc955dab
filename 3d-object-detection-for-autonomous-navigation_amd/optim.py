"""Optimizer step and gradient exchange of the training loop.

  ExponentialDecay     tf.keras.optimizers.schedules.ExponentialDecay as built at train.py:224-229
                       (decay_steps is divided by the batch size there)
  AdamW                tfa.optimizers.AdamW(learning_rate=schedule, weight_decay, epsilon=1e-8), train.py:231-236,
                       applied by optimizer.apply_gradients (train.py:301): one HIP launch per step over ONE flat
                       float32 buffer (parameters, gradients and both moments live in HBM; torch owns the memory)
  allreduce_gradients  the data-parallel exchange BASELINE.json configs[4] names: the flat gradient buffer is
                       summed over the ranks and divided by the world size -- one collective per step
                       (RCCL through torch.distributed's "nccl" backend on the GPUs, gloo in the CPU tests)
  GradClip             gradient clipping and the non-finite step guard in front of the update: the lines train.py:293-294
                       carries commented out (tf.clip_by_value, tf.clip_by_norm per tensor) and tf.clip_by_global_norm.
                       Opt-in; the norms are taken on the GPU (csrc/grad_clip.hip: float64 sums in a fixed order), the
                       update kernel reads the finished scales there, the host reads a few words at the step's one wait
  clip_gradients_np    the same rules on the host: the tests' reference
The arithmetic of the update is in csrc/optim.hip; this module only holds the step counter and the schedule.
"""
import ctypes
import math
import os


class ExponentialDecay:
    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False):
        self.initial_learning_rate = float(initial_learning_rate)
        self.decay_steps = float(decay_steps)
        self.decay_rate = float(decay_rate)
        self.staircase = bool(staircase)

    def __call__(self, step):
        p = float(step) / self.decay_steps
        if self.staircase:
            p = math.floor(p)
        return self.initial_learning_rate * self.decay_rate ** p

    @classmethod
    def from_config(cls, train_config, batch_size):
        """train.py:224-229: the YAML's decay_steps counts samples, the schedule counts optimizer steps."""
        c = train_config["optimizer"]["adam_optimizer"]["learning_rate"]["exponential_decay_learning_rate"]
        return cls(c["initial_learning_rate"], c["decay_steps"] / batch_size, c["decay_factor"], c["staircase"])


class GradClip:
    """mode: None (monitor: norms only), "value", "norm" (per tensor) or "global_norm"; clip: the bound c (> 0, finite)
    of a clipping mode; skip_nonfinite: a step whose trainable gradient holds a NaN or Inf changes nothing.  The
    clipped gradient g' exists inside the update kernel only: the gradient buffer keeps the raw values (what
    Trainer.gradients() returns); the reported scales say what was applied."""
    MODES = (None, "value", "norm", "global_norm")      # index = enum pp_grad_clip_mode

    def __init__(self, mode=None, clip=None, skip_nonfinite=False):
        if mode not in self.MODES:
            raise ValueError(f"GradClip mode: None, 'value', 'norm' or 'global_norm', not {mode!r}")
        if mode is not None:
            if clip is None:
                raise ValueError(f"GradClip mode {mode!r} needs clip")
            if isinstance(clip, bool) or not isinstance(clip, (int, float)) and not hasattr(clip, "__float__"):
                raise ValueError(f"GradClip clip: a positive number, not {clip!r}")
            clip = float(clip)
            if not (clip > 0.0 and math.isfinite(clip)):
                raise ValueError(f"GradClip clip must be positive and finite, not {clip!r}")
        else:
            clip = None if clip is None else float(clip)
        self.mode, self.clip, self.skip_nonfinite = mode, clip, bool(skip_nonfinite)

    @property
    def needs_norm(self):
        """Whether the reduction runs in front of the update ("value" without the guard is the one case without)."""
        return self.mode != "value" or self.skip_nonfinite

    @classmethod
    def from_config(cls, train_config):
        """train_config.gradient_clipping: {mode, clip, skip_nonfinite} -- a key of this project, not of the reference's
        YAML; absent: None (nothing is switched on)."""
        c = train_config.get("gradient_clipping") if isinstance(train_config, dict) else None
        if c is None:
            return None
        if not isinstance(c, dict) or set(c) - {"mode", "clip", "skip_nonfinite"}:
            raise ValueError(f"train_config.gradient_clipping: a dict of mode, clip, skip_nonfinite, not {c!r}")
        mode = c.get("mode")
        if isinstance(mode, str) and mode.lower() in ("none", ""):
            mode = None
        return cls(mode, c.get("clip"), bool(c.get("skip_nonfinite", False)))

    def __repr__(self):
        return f"GradClip(mode={self.mode!r}, clip={self.clip!r}, skip_nonfinite={self.skip_nonfinite!r})"


def clip_gradients_np(flat, segments, groups, clip):
    """The rules of csrc/grad_clip.hip on the host (TensorFlow 2.2's published tf.clip_by_value / clip_by_norm /
    clip_by_global_norm): float64 sums of squares per group, summed over the groups in group order, float32 norms, then
    the float32 arithmetic of the rule, one rounding per operation.  flat: float32 [n]; segments: (offset, size) pairs,
    None = the whole buffer; groups: an int per segment, None = one group; clip: a GradClip.
    Returns (a float32 copy with the segments clipped, the statistics dict of AdamW.clip_stats())."""
    import numpy as np
    f32 = np.float32
    flat = np.ascontiguousarray(flat, dtype=f32).reshape(-1)
    seg = np.asarray([(0, flat.size)] if segments is None else segments, dtype=np.int64).reshape(-1, 2)
    grp = np.zeros(len(seg), np.int64) if groups is None else np.asarray(groups, dtype=np.int64).reshape(-1)
    if len(grp) != len(seg):
        raise ValueError("one group per segment")
    G = int(grp.max()) + 1 if len(grp) else 1
    with np.errstate(all="ignore"):
        sums = np.zeros(G, np.float64)
        for (off, size), k in zip(seg, grp):
            x = flat[off:off + size].astype(np.float64)
            sums[k] += float(np.sum(x * x))
        total = np.float64(0.0)
        for k in range(G):
            total = total + sums[k]
        norms = np.sqrt(sums).astype(f32)
        gnorm = f32(np.sqrt(total))
        nonfinite = not np.isfinite(total)
        c = f32(clip.clip) if clip.mode is not None else None
        scale = f32(1.0)
        scales = np.ones(G, f32)
        out = flat.copy()
        if clip.mode == "global_norm":
            scale = c * np.minimum(f32(1.0) / gnorm, f32(1.0) / c) if np.isfinite(gnorm) else f32(np.nan)
            scales[:] = scale
        elif clip.mode == "norm":
            scales = c / np.maximum(norms, c)           # (np.maximum keeps a NaN norm)
        for (off, size), k in zip(seg, grp):
            g = flat[off:off + size]
            if clip.mode == "value":
                out[off:off + size] = np.minimum(np.maximum(g, -c), c)          # (both keep a NaN)
            elif clip.mode == "norm":
                out[off:off + size] = (g * c) / np.maximum(norms[k], c)
            elif clip.mode == "global_norm":
                out[off:off + size] = g * scale
    return out, {"global_norm": float(gnorm), "scale": float(scale), "nonfinite": bool(nonfinite),
                 "skipped": bool(clip.skip_nonfinite and (nonfinite or not np.isfinite(gnorm))), "norms": norms, "scales": scales.astype(f32)}


class AdamW:
    """params / grads: flat contiguous float32 torch tensors on the same GPU (the caller keeps `grads` filled)."""

    def __init__(self, params, learning_rate, weight_decay, beta_1=0.9, beta_2=0.999, epsilon=1e-8):
        import torch
        if params.dtype != torch.float32 or not params.is_contiguous() or params.dim() != 1:
            raise ValueError("params must be a flat contiguous float32 tensor")
        if not params.is_cuda:
            raise RuntimeError("AdamW runs on the GPU only (HIP kernel k_adamw); there is no CPU path")
        self.params = params
        self.m = torch.zeros_like(params)
        self.v = torch.zeros_like(params)
        self.learning_rate = learning_rate
        self.weight_decay = float(weight_decay)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self.iterations = 0
        self.segments = None      # None: the whole buffer; else the trainable (offset, size) segments
        self.clip = None          # a GradClip (set_clip): the step goes through pp_adamw_step_clipped_device
        self._clip_state = None

    def set_segments(self, segments):
        """Update only these (offset, size) segments of the buffers (frozen layers: the trainable ones); None = all.
        Entries outside them -- parameters and both moments -- are neither read nor written."""
        import numpy as np
        if segments is None:
            self.segments = None
            return
        arr = np.ascontiguousarray(np.asarray(segments, dtype=np.int64).reshape(-1, 2))
        n = self.params.numel()
        if ((arr[:, 0] < 0) | (arr[:, 1] < 0) | (arr[:, 0] + arr[:, 1] > n)).any():
            raise ValueError("segments must lie inside the parameter buffer")
        self.segments = arr

    def set_clip(self, clip, groups=None):
        """Clip the gradient inside the update (a GradClip; None = off: the step is the unclipped calls again).
        groups: an int per segment of set_segments (one segment, the whole buffer, without), None = one group; "norm"
        clips per group.  Call it again after set_segments: the groups belong to the segment table."""
        import numpy as np
        import torch
        from . import _lib
        if clip is None:
            self.clip = self._clip_state = None
            return
        if not isinstance(clip, GradClip):
            raise ValueError("set_clip: a GradClip or None")
        n = self.params.numel()
        seg = self.segments if self.segments is not None else np.asarray([[0, n]], dtype=np.int64)
        if groups is None:
            grp, n_groups = None, 1
        else:
            grp = np.ascontiguousarray(np.asarray(groups, dtype=np.int32).reshape(-1))
            if len(grp) != len(seg) or (len(grp) and (grp.min() < 0)):
                raise ValueError("groups: one non-negative int per segment")
            n_groups = int(grp.max()) + 1 if len(grp) else 1
        nbytes = ctypes.c_int64(0)
        if _lib.lib().pp_grad_clip_workspace_bytes(n, len(seg), n_groups, ctypes.byref(nbytes)) != 0:
            raise ValueError("pp_grad_clip_workspace_bytes: " + _lib.lib().pp_last_error(None).decode())
        ws = torch.zeros(nbytes.value // 4, dtype=torch.int32, device=self.params.device)
        cfg = _lib.PPGradClipConfig(GradClip.MODES.index(clip.mode), clip.clip if clip.mode is not None else 0.0,
                                    1 if clip.skip_nonfinite else 0)
        self.clip = clip
        self._clip_state = (seg, grp, n_groups, ws, cfg)

    def stats_words(self):
        """The device tensor (int32 view) of the statistics block: 4 + 2 * n_groups words (pp_hip.h)."""
        _, _, n_groups, ws, _ = self._clip_state
        return ws[:4 + 2 * n_groups]

    @staticmethod
    def decode_stats(words):
        """The statistics block (a host int32 array of 4 + 2 G words) as the dict clip_stats() returns."""
        import numpy as np
        w = np.ascontiguousarray(words, dtype=np.int32)
        G = (len(w) - 4) // 2
        f = w.view(np.float32)
        return {"global_norm": float(f[0]), "scale": float(f[1]), "nonfinite": bool(w[2]), "skipped": bool(w[3]),
                "norms": f[4:4 + G].copy(), "scales": f[4 + G:4 + 2 * G].copy()}

    def clip_stats(self):
        """What the last clipped step measured and applied (synchronises): global_norm, scale, nonfinite, skipped, and
        per group norms / scales.  A GradClip("value") without the guard takes no norms: its block is never written."""
        if self.clip is None:
            raise RuntimeError("clip_stats: no clip is set (AdamW.set_clip)")
        return self.decode_stats(self.stats_words().cpu().numpy())

    def lr_t(self):
        lr = self.learning_rate(self.iterations) if callable(self.learning_rate) else float(self.learning_rate)
        t = self.iterations + 1
        return lr * math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)

    def apply_gradients(self, grads):
        import torch
        from . import _lib
        if grads.shape != self.params.shape or grads.dtype != torch.float32 or not grads.is_contiguous() or \
                grads.device != self.params.device:
            raise ValueError("grads must match params (flat float32, same device)")
        stream = torch.cuda.current_stream(self.params.device).cuda_stream
        if self.clip is not None:
            seg, grp, n_groups, ws, cfg = self._clip_state
            if (self.segments is None and len(seg) != 1) or (self.segments is not None and seg is not self.segments):
                raise RuntimeError("the segments changed after set_clip: call set_clip again")
            st = _lib.lib().pp_adamw_step_clipped_device(
                self.params.device.index or 0, ctypes.c_void_p(stream), ctypes.c_void_p(self.params.data_ptr()),
                ctypes.c_void_p(grads.data_ptr()), ctypes.c_void_p(self.m.data_ptr()), ctypes.c_void_p(self.v.data_ptr()),
                self.params.numel(), seg.ctypes.data_as(ctypes.c_void_p), len(seg),
                grp.ctypes.data_as(ctypes.c_void_p) if grp is not None else None, n_groups, ctypes.byref(cfg),
                ctypes.c_void_p(ws.data_ptr()), self.lr_t(), self.beta_1, self.beta_2, self.epsilon, self.weight_decay)
            if st != 0:
                raise RuntimeError("pp_adamw_step_clipped_device failed: " + _lib.lib().pp_last_error(None).decode())
            self.iterations += 1      # (a guarded step that was skipped: whoever reads `skipped` puts it back)
            return
        if self.segments is not None:
            st = _lib.lib().pp_adamw_step_segments_device(
                self.params.device.index or 0, ctypes.c_void_p(stream), ctypes.c_void_p(self.params.data_ptr()),
                ctypes.c_void_p(grads.data_ptr()), ctypes.c_void_p(self.m.data_ptr()), ctypes.c_void_p(self.v.data_ptr()),
                self.segments.ctypes.data_as(ctypes.c_void_p), len(self.segments), self.lr_t(), self.beta_1,
                self.beta_2, self.epsilon, self.weight_decay)
            if st != 0:
                raise RuntimeError("pp_adamw_step_segments_device failed: " + _lib.lib().pp_last_error(None).decode())
            self.iterations += 1
            return
        st = _lib.lib().pp_adamw_step_device(self.params.device.index or 0, ctypes.c_void_p(stream),
                                             ctypes.c_void_p(self.params.data_ptr()), ctypes.c_void_p(grads.data_ptr()),
                                             ctypes.c_void_p(self.m.data_ptr()), ctypes.c_void_p(self.v.data_ptr()),
                                             self.params.numel(), self.lr_t(), self.beta_1, self.beta_2, self.epsilon,
                                             self.weight_decay)
        if st != 0:
            raise RuntimeError("pp_adamw_step_device failed: " + _lib.lib().pp_last_error(None).decode())
        self.iterations += 1


def allreduce_gradients(flat_grads, dist=None):
    """Mean of the flat gradient buffer over the ranks, in place; a single collective.  `dist` is
    torch.distributed (or None / uninitialised / world size 1: nothing to do)."""
    if dist is None or not dist.is_initialized():
        return flat_grads
    if dist.get_world_size() == 1 and os.environ.get("PP_FORCE_ALLREDUCE") != "1":
        return flat_grads       # (PP_FORCE_ALLREDUCE=1: the one-rank rehearsal still sends the buffer through the backend)
    dist.all_reduce(flat_grads, op=dist.ReduceOp.SUM)
    flat_grads /= dist.get_world_size()
    return flat_grads
