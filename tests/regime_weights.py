"""Trained-regime problems for the training step: weights (and frames) whose pre-BatchNorm maps have channels with
|mean| / std >= R, the regime of a checkpoint trained to convergence and the one where a single-pass float32 variance
(sum z^2 / n - mean^2) cancels.  Built from init_weights(d, seed) by three edits:

  * in-block separable layer L (stride 1): the BatchNorm in front of it gets an "always on" channel c (gamma 1, beta
    beta0 >> 1, so relu(gamma * zhat + beta) = zhat + beta0 everywhere); L's depthwise kernel of channel c is its centre
    tap alone (the zero padding at the map borders would otherwise pull the border pixels' mean down) and the targeted
    output columns of L's pointwise kernel take channel c with weight 1 and every other channel scaled by 1e-3;
  * transposed convolution: the same always-on channel on the block-final layer in front of it, every tap of the
    targeted output columns taking channel c alone (the ntaps > 1 layout of the statistics partials);
  * the PFN's BatchNorm: targeted Dense columns read the point's absolute z alone, and the frames (regime_frames) put
    every point in a narrow z band around Z0 with every occupied pillar full (more points than T in every pillar).  The
    reference normalises over all P * T rows of the padded tensor -- it zeroes the padded rows and runs Dense +
    BatchNorm on the whole of it (model/pointpillars.py:200-211) -- so a pillar with fewer than T points would put
    zero rows into the statistic; full pillars keep the band's |mean| / std.

The ratios are checked against the float64 oracle's own statistics by tests/test_train_regime.py (CPU)."""
import copy

import numpy as np

import util_ref

IN_BLOCK = ("rpn/block1/1", "rpn/block2/1")      # targeted separable layers (BatchNorm in front: <block>/0)
DECONV = "rpn/deconv2"                            # targeted transposed convolution (kernel == stride 2: 4 taps)
DECONV_SRC = "rpn/block2/1"                       # the block-final layer in front of it
SRC_CH = 0                                        # the always-on channel of a source BatchNorm
PFN_CH = (0, 5)                                   # targeted PFN channels (Dense columns reading z alone)
Z_FEATURE = 2                                     # the point's absolute z among the decorated PFN features
Z0 = 2.0                                          # centre of the frames' z band
T_POINTS = 4                                      # points per pillar of the regime's configuration
MARGIN = 1.3                                      # built ratio / requested ratio


def regime_config(pp, B):
    """tiny_config(B) with T = 4 points per pillar (the frames fill every occupied pillar)."""
    cfg = copy.deepcopy(pp.config.tiny_config(B))
    cfg["model"]["second"]["voxel_generator"]["max_number_of_points_per_voxel"] = T_POINTS
    return cfg


def targets(d):
    """BatchNorm layer -> the channels built to |mean| / std >= R."""
    t = {pre + "/bn": list(range(0, _cout(d, pre), 2)) for pre in IN_BLOCK}
    t[DECONV + "/bn"] = list(range(0, _cout(d, DECONV), 2))
    t["pfn/bn"] = list(PFN_CH)
    return t


def _cout(d, name):
    from pp_amd import weights as W
    return next(s["cout"] for _, n, s in W.layer_table(d) if n == name)


def _always_on(w, bn, beta0):
    w[bn + "/gamma"][SRC_CH] = 1.0
    w[bn + "/beta"][SRC_CH] = beta0


def regime_weights(d, R, seed=21, moving=None):
    """init_weights(d, seed) edited so that the targets(d) channels reach |mean| / std >= R (the source channels'
    beta is MARGIN * R: the targeted map is about beta + zhat, zhat of unit variance).  moving: None keeps the
    initial moving statistics; a dict {bn layer: (mean, var)} sets them (e.g. far from (0, 1), or 0 / 0 so that the
    step's update carries the batch term alone)."""
    from pp_amd import weights as W
    w = {k: np.array(v, dtype=np.float32, copy=True) for k, v in W.init_weights(d, seed).items()}
    beta0 = np.float32(MARGIN * R)
    small = np.float32(1e-3)
    for pre in IN_BLOCK:
        src = pre.rsplit("/", 1)[0] + "/0/bn"
        _always_on(w, src, beta0)
        dw = w[pre + "/depthwise_kernel"]                  # [3, 3, cin, 1]
        dw[:, :, SRC_CH, 0] = 0.0
        dw[1, 1, SRC_CH, 0] = 1.0
        pw = w[pre + "/pointwise_kernel"]                  # [1, 1, cin, cout]
        for o in targets(d)[pre + "/bn"]:
            pw[0, 0, :, o] *= small
            pw[0, 0, SRC_CH, o] = 1.0
    _always_on(w, DECONV_SRC + "/bn", beta0)
    k = w[DECONV + "/kernel"]                              # [k, k, cout, cin]
    for o in targets(d)[DECONV + "/bn"]:
        k[:, :, o, :] *= small
        k[:, :, o, SRC_CH] = 1.0
    kern = w["pfn/dense/kernel"]                           # [features, C]
    for c in PFN_CH:
        kern[:, c] = 0.0
        kern[Z_FEATURE, c] = 1.0
    if moving is not None:
        for bn, (m, v) in moving.items():
            w[bn + "/moving_mean"][...] = np.asarray(m, np.float32)
            w[bn + "/moving_variance"][...] = np.asarray(v, np.float32)
    return w


def regime_frames(d, R, B, seed=3, pillars=(220, 160), points=6):
    """B frames of `points` (> T) points in each of `pillars[b]` distinct cells, z uniform in a band around Z0 whose
    |mean| / std is MARGIN * R."""
    assert points > d.max_points
    rng = np.random.default_rng(seed)
    half = Z0 * np.sqrt(3.0) / (MARGIN * R)               # uniform on [Z0 - half, Z0 + half]: std = half / sqrt(3)
    vx, vy = float(d.voxel_size[0]), float(d.voxel_size[1])
    x0, y0 = float(d.pc_range[0]), float(d.pc_range[1])
    frames = []
    for b in range(B):
        n = pillars[b % len(pillars)]
        cells = rng.choice(d.nx * d.ny, n, replace=False)
        cx, cy = cells % d.nx, cells // d.nx
        # strictly inside the cell: a point on a cell edge could round into the neighbour
        u = rng.uniform(0.05, 0.95, (n, points, 2))
        xs = x0 + (cx[:, None] + u[..., 0]) * vx
        ys = y0 + (cy[:, None] + u[..., 1]) * vy
        zs = rng.uniform(Z0 - half, Z0 + half, (n, points))
        frames.append(np.stack([xs, ys, zs], axis=-1).reshape(-1, 3).astype(np.float32))
    return frames


def ratios(stats, tg):
    """{bn layer: smallest |mean| / sqrt(var) over its targeted channels} from (mean, biased var) statistics."""
    out = {}
    for bn, ch in tg.items():
        m, v = (np.asarray(a, np.float64)[ch] for a in stats[bn])
        out[bn] = float((np.abs(m) / np.sqrt(v)).min())
    return out


def regime_problem(pp, R, B=2, seed=11):
    """(cfg, d, frames, labels, reg_targets, oracle example, oracle frames) of a regime problem of ratio R"""
    cfg = regime_config(pp, B)
    d = pp.config.Derived(cfg)
    frames = regime_frames(d, R, B)
    rng = np.random.default_rng(seed)
    labels = rng.choice([-1, 0, 0, 0, 0], size=(B, d.num_anchors)).astype(np.int32)
    reg = np.zeros((B, d.num_anchors, 7), np.float32)
    for b in range(B):
        pos = rng.choice(d.num_anchors, 30 if b == 0 else 10, replace=False)
        labels[b, pos] = 1
        reg[b, pos] = rng.normal(0, 0.4, (len(pos), 7)).astype(np.float32)
    rect, trv, p2 = pp.synth.default_calib()
    ex, fr = util_ref.oracle_example(d, frames, rect, trv, p2)
    return cfg, d, frames, labels, reg, ex, fr
