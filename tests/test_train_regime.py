"""CPU check of the trained-regime problems (tests/regime_weights.py) that tests/test_gpu_train_regime.py runs on the
GPU: the targeted BatchNorm layers must reach the requested |mean| / std in the float64 oracle's own statistics, so
that the regime cannot silently become an easy one."""
import numpy as np
import pytest
import torch

from oracle import train_ref
import regime_weights as rw


@pytest.mark.parametrize("R", [100, 300, 1000])
def test_regime_weights_reach_the_ratio(pp, R):
    cfg, d, frames, labels, reg, ex, fr = rw.regime_problem(pp, R)
    # every occupied pillar is full: no padded zero row enters the PFN's statistic
    assert all(np.all(f["num_points"] == d.max_points) for f in fr)
    w = rw.regime_weights(d, R)
    _, _, stats, _ = train_ref.training_step(d, w, ex, labels, reg, ex[6][0], dtype=torch.float64)
    got = rw.ratios(stats, rw.targets(d))
    assert set(got) == {"rpn/block1/1/bn", "rpn/block2/1/bn", "rpn/deconv2/bn", "pfn/bn"}
    for bn, r in got.items():
        assert r >= R, (bn, r, R)
        assert r <= 3 * R, (bn, r, R)          # the regime asked for, not an arbitrarily harder one
    print(f"R={R}: " + ", ".join(f"{k} {v:.0f}" for k, v in got.items()))
