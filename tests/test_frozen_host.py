"""Frozen-layer fine-tuning on the host (trainer.reference_frozen_units / resolve_frozen / trainable_segments): the
reference's set_trainable selection (train.py:62-113) against the Keras layer indices it flips, and what is refused."""
import numpy as np
import pytest

import keras_tree


def _cfg(pp, layer_nums=None):
    cfg = pp.config.pedestrian_d435i_config(2)
    if layer_nums is not None:
        cfg["model"]["second"]["rpn"]["layer_nums"] = list(layer_nums)
    return pp.config.Derived(cfg)


def _keras_set_trainable_tensors(d):
    """The package tensors of the Keras layers set_trainable(net, False) flips, through keras_tree's variable tree:
    net.layers[1].layers[0].layers[0..2] (the PFN's Dense, BatchNorm, ReLU) and net.layers[3].layers[{0,2,4}]
    .layers[0..9] (RPN.layers = block1, deconv1, block2, ...; a block's Sequential = ZeroPadding2D, then a
    SeparableConv2D, BatchNormalization, ReLU triple per separable layer)."""
    tree = keras_tree.keras_variables(d)
    out = {ours for _, ours in tree["pillar_feature_net"]}       # Dense + BatchNorm (+ ReLU: no variables)
    for b in range(3):
        base = f"voxel_net/rpn/block{b + 1}/"
        owners = []                                              # Keras layer names of the block, creation order
        for kname, _ in tree["rpn"]:
            if kname.startswith(base):
                layer = kname[len(base):].split("/")[0]
                if layer not in owners:
                    owners.append(layer)
        seps = [o for o in owners if o.startswith("separable_conv2d")]
        bns = [o for o in owners if o.startswith("batch_normalization")]
        seq = ["zero_padding2d"]
        for s, n in zip(seps, bns):
            seq += [s, n, "re_lu"]
        frozen_layers = set(seq[i] for i in range(10))           # raises IndexError where the reference does
        out |= {ours for kname, ours in tree["rpn"]
                if kname.startswith(base) and kname[len(base):].split("/")[0] in frozen_layers}
    return out


def test_reference_selection_is_pfn_and_first_three_separable_layers(pp):
    from pp_amd import trainer
    d = _cfg(pp)
    assert d.layer_nums == [3, 5, 5]
    units = trainer.reference_frozen_units(d)
    assert units == ["pfn"] + [f"rpn/block{b}/{j}" for b in (1, 2, 3) for j in (0, 1, 2)]
    # the same tensors as the Keras layers the reference flips
    shapes = pp.weights.expected_shapes(d)
    ours = {n for n in shapes if trainer.unit_of(n) in set(units)}
    assert ours == _keras_set_trainable_tensors(d)
    # what stays trainable with the shipped layer counts
    rest = [u for u in trainer.train_units(d) if u not in units]
    assert rest == ["rpn/block1/3", "rpn/deconv1", "rpn/block2/3", "rpn/block2/4", "rpn/block2/5", "rpn/deconv2",
                    "rpn/block3/3", "rpn/block3/4", "rpn/block3/5", "rpn/deconv3", "rpn/conv_box", "rpn/conv_cls",
                    "rpn/conv_dir_cls"]
    assert trainer.resolve_frozen(d, "reference") == tuple(units)


@pytest.mark.parametrize("layer_nums", [[1, 5, 5], [3, 1, 5], [3, 5, 0], [1, 1, 1]])
def test_reference_selection_needs_three_separable_layers_per_block(pp, layer_nums):
    from pp_amd import trainer
    d = _cfg(pp, layer_nums)
    with pytest.raises(IndexError):          # the reference itself
        _keras_set_trainable_tensors(d)
    with pytest.raises(ValueError):
        trainer.reference_frozen_units(d)
    with pytest.raises(ValueError):
        trainer.resolve_frozen(d, "reference")


def test_two_separable_layers_per_block_freeze_whole_blocks(pp):
    from pp_amd import trainer
    d = _cfg(pp, [2, 2, 2])
    units = trainer.reference_frozen_units(d)
    shapes = pp.weights.expected_shapes(d)
    assert {n for n in shapes if trainer.unit_of(n) in set(units)} == _keras_set_trainable_tensors(d)


def test_unknown_repeated_and_total_freezes_are_refused(pp):
    from pp_amd import trainer
    d = _cfg(pp)
    for bad in (["rpn/block4/0"], ["rpn/block1/6"], ["pfn/dense"], ["rpn/block1/0/bn"], ["PFN"], [3], "everything"):
        with pytest.raises(ValueError):
            trainer.resolve_frozen(d, bad)
    with pytest.raises(ValueError):
        trainer.resolve_frozen(d, ["pfn", "rpn/deconv1", "pfn"])
    with pytest.raises(ValueError):
        trainer.resolve_frozen(d, trainer.train_units(d))
    # one unit short of everything is fine; names come back in network order
    assert trainer.resolve_frozen(d, trainer.train_units(d)[1:][::-1]) == tuple(trainer.train_units(d)[1:])
    assert trainer.resolve_frozen(d, None) == () and trainer.resolve_frozen(d, ()) == ()
    # without a direction head there is no such unit
    cfg = pp.config.tiny_config(2)
    cfg["model"]["second"]["use_direction_classifier"] = False
    d2 = pp.config.Derived(cfg)
    assert "rpn/conv_dir_cls" not in trainer.train_units(d2)
    with pytest.raises(ValueError):
        trainer.resolve_frozen(d2, ["rpn/conv_dir_cls"])


def test_trainable_segments_cover_exactly_the_trainable_tensors(pp):
    """The AdamW segments of a freeze, on a layout laid out as the training step's (parameters in network order, the
    moving statistics in a buffer of their own)."""
    from pp_amd import trainer
    d = _cfg(pp)
    layout, po, so = [], 0, 0
    for name, shape in pp.weights.expected_shapes(d).items():
        size = int(np.prod(shape))
        st = name.endswith(("moving_mean", "moving_variance"))
        layout.append((name, so if st else po, size, st))
        if st:
            so += size
        else:
            po += size
    for frozen in (trainer.reference_frozen_units(d), ["pfn"], ["rpn/conv_cls", "rpn/block2/4"], []):
        segs = trainer.trainable_segments(layout, frozen)
        covered = np.zeros(po, bool)
        for off, size in segs:
            assert not covered[off:off + size].any()
            covered[off:off + size] = True
        want = np.zeros(po, bool)
        for name, off, size, st in layout:
            if not st and trainer.unit_of(name) not in set(frozen):
                want[off:off + size] = True
        assert np.array_equal(covered, want)
        assert all(a[0] + a[1] < b[0] for a, b in zip(segs, segs[1:]))     # merged where they touch
    assert trainer.trainable_segments(layout, []) == [(0, po)]
