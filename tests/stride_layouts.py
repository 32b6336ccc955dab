"""The backbone layouts of tests/test_stride_layouts_host.py and tests/test_gpu_train_layouts.py: tiny_config with other
layer_strides / upsample_strides (first block at stride 2 as the KITTI-shaped configuration has it, kernel == stride 1, 2,
4 and 8 in the transposed convolutions, a stride-1 block in front of a k = 1 deconv), a block without in-block layers
(layer_nums [1, 0, 2]) and three frames, so that every map's row count ends inside a 64- and a 128-row tile.  Test
infrastructure only."""
import copy

import numpy as np

B = 3
COUNTS = (900, 400, 150)          # points per frame, uniform over the whole range
POSITIVES = (40, 13, 13)          # positives per frame (capped at a quarter of the anchors)
VOXEL = 0.08
CLOUD_SEED = 4
TARGET_SEED = 11
MARGIN_BAR = 5e-6                 # test_training_step_matches_autograd's: no pre-ReLU value / PFN max nearer its kink
GRAD_BAR = 1e-4                   # test_gradients_match_autograd_small_grids': of a tensor's largest gradient

# name: (nx, ny, layer_strides, upsample_strides, wide, weight seed)
# The weight seed is the first of 21, 22, ... under which the float32 restatement of the step keeps every pre-ReLU value
# and PFN max at least MARGIN_BAR from its kink and stays within GRAD_BAR / 4 of the float64 graph under its own decisions;
# measured on the CPU (tests/test_stride_layouts_host.py asserts both and prints them), never searched at run time.
# The float32 restatement is not bit-identical between CPUs (s222-u248 at seed 22: 5.33e-6 on one machine, 5.00e-6 on
# another), so a seed counts as passing only from 6e-6 on; the asserted bar stays MARGIN_BAR.
LAYOUTS = {
    "s222-u124": (24, 16, (2, 2, 2), (1, 2, 4), False, 21),
    "s222-u248": (24, 16, (2, 2, 2), (2, 4, 8), False, 24),
    "s212-u112": (24, 16, (2, 1, 2), (1, 1, 2), False, 21),
    "s112-u112": (20, 12, (1, 1, 2), (1, 1, 2), False, 22),
    "s121-u122": (20, 12, (1, 2, 1), (1, 2, 2), False, 22),
    "s111-u111": (20, 12, (1, 1, 1), (1, 1, 1), False, 28),
    "s222-u124-wide": (24, 16, (2, 2, 2), (1, 2, 4), True, 22),
}
NAMES = list(LAYOUTS)

# what the table intends, written out: (h, w) of the three blocks' maps, the head map, anchors (two per location)
MAPS = {
    "s222-u124": (((8, 12), (4, 6), (2, 3)), (8, 12), 192),
    "s222-u248": (((8, 12), (4, 6), (2, 3)), (16, 24), 768),
    "s212-u112": (((8, 12), (8, 12), (4, 6)), (8, 12), 192),
    "s112-u112": (((12, 20), (12, 20), (6, 10)), (12, 20), 480),
    "s121-u122": (((12, 20), (6, 10), (6, 10)), (12, 20), 480),
    "s111-u111": (((12, 20), (12, 20), (12, 20)), (12, 20), 480),
    "s222-u124-wide": (((8, 12), (4, 6), (2, 3)), (8, 12), 192),
}


def layout_config(pp, name, batch=B):
    """tiny_config(batch) on the layout's grid (range, feature_map_size, anchor strides and offsets rescaled to the grid
    and the out-size factor, as test_gpu_parity._random_config does)."""
    nx, ny, ls, us, wide, _ = LAYOUTS[name]
    cfg = copy.deepcopy(pp.config.tiny_config(batch))
    s = cfg["model"]["second"]
    osf = ls[0] // us[0]
    x0, y0 = 0.0, -ny * VOXEL / 2
    cfg["eval_input_reader"]["feature_map_size"] = [1, ny // osf, nx // osf]
    s["voxel_generator"].update(point_cloud_range=[x0, y0, -3.0, x0 + nx * VOXEL, y0 + ny * VOXEL, 3.0],
                                voxel_size=[VOXEL, VOXEL, 4.0])
    s["rpn"].update(layer_nums=[1, 0, 2], layer_strides=list(ls), upsample_strides=list(us))
    if wide:      # the KITTI-shaped configuration's widths
        s["rpn"].update(layer_nums=[1, 1, 1], num_filters=[64, 128, 256], num_upsample_filters=[128, 128, 128])
        s["voxel_feature_extractor"]["num_filters"] = 128
    s["target_assigner"]["anchor_generators"]["anchor_generator_stride"].update(
        strides=[VOXEL * osf, VOXEL * osf, 0.0], offsets=[x0 + VOXEL * osf, y0, -1.465])
    return cfg


def layer_rows(d, batch=B):
    """{layer: BatchNorm rows} of every separable layer (B * h * w) and transposed convolution (B * h * w * k * k), and
    {block: (h, w)}."""
    rows, maps, h, w = {}, [], d.ny, d.nx
    for b in range(3):
        for j in range(d.layer_nums[b] + 1):
            if j == 0 and d.layer_strides[b] == 2:
                h, w = (h + 1) // 2, (w + 1) // 2
            rows[f"rpn/block{b + 1}/{j}/bn"] = batch * h * w
        k = d.upsample_strides[b]
        rows[f"rpn/deconv{b + 1}/bn"] = batch * h * w * k * k
        maps.append((h, w))
    return rows, tuple(maps)


def step_targets(d, batch=B, seed=TARGET_SEED):
    """Random targets as test_gpu_anchor_layouts._step_targets draws them: positives on any anchor."""
    rng = np.random.default_rng(seed)
    A = d.num_anchors
    labels = rng.choice([-1, 0, 0, 0, 0], size=(batch, A)).astype(np.int32)
    reg = np.zeros((batch, A, 7), np.float32)
    for b in range(batch):
        pos = rng.choice(A, min(POSITIVES[b], A // 4), replace=False)
        labels[b, pos] = rng.integers(1, d.num_class + 1, len(pos))
        reg[b, pos] = rng.normal(0, 0.4, (len(pos), 7)).astype(np.float32)
    return labels, reg


class LayoutProblem:
    """One layout: config, Derived, frames, targets, weights, the oracle example, and -- computed on first use, once, and
    left unchanged -- the restated step in float32 (with its margins and its own decisions) and in float64."""

    def __init__(self, pp, name, weight_seed=None):
        import util_ref
        self.name = name
        self.cfg = layout_config(pp, name)
        d = self.d = pp.config.Derived(self.cfg)
        rng = np.random.default_rng(CLOUD_SEED)
        lo, hi = d.pc_range[:3], d.pc_range[3:]
        self.frames = [rng.uniform(lo, hi, (n, 3)).astype(np.float32) for n in COUNTS]
        self.labels, self.reg = step_targets(d)
        self.num_positives = int((self.labels > 0).sum())
        self.weight_seed = LAYOUTS[name][5] if weight_seed is None else weight_seed
        self.w = pp.weights.init_weights(d, seed=self.weight_seed)
        self.calib = pp.synth.default_calib()
        rect, trv, p2 = self.calib
        self.ex, _ = util_ref.oracle_example(d, self.frames, rect, trv, p2)
        self.anchors = self.ex[6][0]
        self._ref32 = self._ref64 = None

    @property
    def ref32(self):
        """(vals, grads, stats, preds, margins, record) of the float32 restatement"""
        if self._ref32 is None:
            from oracle import train_ref
            margins, record = {}, {}
            out = train_ref.training_step(self.d, self.w, self.ex, self.labels, self.reg, self.anchors, margins=margins,
                                          record=record)
            self._ref32 = out + (margins, record)
        return self._ref32

    @property
    def margin(self):
        return min(v for k, v in self.ref32[4].items() if not k.startswith("#"))

    @property
    def stats64(self):
        """the float64 restatement's batch statistics {layer: (mean, biased variance)}"""
        if self._ref64 is None:
            import torch
            from oracle import train_ref
            self._ref64 = train_ref.training_step(self.d, self.w, self.ex, self.labels, self.reg, self.anchors,
                                                  dtype=torch.float64)
        return self._ref64[2]

    def grads64(self, forced):
        """gradients of the float64 graph that takes the given decisions"""
        import torch
        from oracle import train_ref
        return train_ref.training_step(self.d, self.w, self.ex, self.labels, self.reg, self.anchors, dtype=torch.float64,
                                       forced=forced)[1]


_CACHE = {}


def layout_problem(pp, name):
    if name not in _CACHE:
        _CACHE[name] = LayoutProblem(pp, name)
    return _CACHE[name]
