"""The stride / upsample layouts of tests/stride_layouts.py, on the host: Derived accepts each, the maps and row counts are
what the table intends (every block's B * h * w ends inside a 64-row tile where the first stride is 2), the fixed weight
seed keeps the restated step at least 5e-6 from every ReLU / max kink, and the reference alone -- float32 restatement
against the float64 graph under the float32 run's own decisions -- stays within a quarter of the bar the GPU test uses.

Measured (smallest distance to a kink at weight seeds 21, 22, ...; the table fixes the first at 6e-6 or more -- the
float32 restatement differs between CPUs by a few 1e-7, and 5.3e-6 on one machine was 5.0e-6 on another):
  s222-u124       1.0e-5                                   -> 21
  s222-u248       4.1e-6, 5.3e-6, 1.5e-6, 8.5e-6           -> 24
  s212-u112       2.0e-5                                   -> 21
  s112-u112       2.2e-6, 7.1e-6                           -> 22
  s121-u122       1.1e-6, 7.1e-6                           -> 22
  s111-u111       2.0e-6, 5.4e-6, 4.1e-6, 1.8e-7, 1.8e-6, 4.2e-6, 4.1e-6, 1.1e-5   -> 28
  s222-u124-wide  4.6e-6, 7.6e-6                           -> 22
"""
import pytest

import stride_layouts as SL
from test_gpu_train import _rel_errors

# B * h * w of the three blocks (B = 3)
BLOCK_ROWS = {
    "s222-u124": (288, 72, 18), "s222-u248": (288, 72, 18), "s222-u124-wide": (288, 72, 18),
    "s212-u112": (288, 288, 72),          # block 2 at stride 1 keeps block 1's 12 x 8 map
    "s112-u112": (720, 720, 180), "s121-u122": (720, 180, 180), "s111-u111": (720, 720, 720),
}
# B * h * w * k * k of the three transposed convolutions: each fills the head map
DECONV_ROWS = {n: (3 * v[1][0] * v[1][1],) * 3 for n, v in SL.MAPS.items()}


@pytest.mark.parametrize("name", SL.NAMES)
def test_layout_maps_and_rows(pp, name):
    nx, ny, ls, us, wide, _ = SL.LAYOUTS[name]
    d = pp.config.Derived(SL.layout_config(pp, name))
    maps, head, A = SL.MAPS[name]
    assert (d.nx, d.ny) == (nx, ny) and tuple(d.layer_strides) == ls and tuple(d.upsample_strides) == us
    assert d.out_size_factor == ls[0] // us[0] and (d.head_h, d.head_w) == head
    assert d.num_anchor_per_loc == 2 and d.num_anchors == A
    assert d.layer_nums == ([1, 1, 1] if wide else [1, 0, 2])
    assert (d.num_filters, d.pfn_filters) == (([64, 128, 256], 128) if wide else ([32, 32, 64], 32))
    rows, got_maps = SL.layer_rows(d)
    assert got_maps == maps
    assert tuple(rows[f"rpn/block{b + 1}/0/bn"] for b in range(3)) == BLOCK_ROWS[name]
    assert tuple(rows[f"rpn/deconv{b + 1}/bn"] for b in range(3)) == DECONV_ROWS[name]
    for b, (h, w) in enumerate(maps):      # every transposed convolution meets the head map
        assert (h * us[b], w * us[b]) == head
    # B = 3: every block's rows end inside a 64- and a 128-row tile (at B = 2 on 20 x 16 block 1 is an exact multiple)
    assert all(r % 64 != 0 and r % 128 != 0 for r in BLOCK_ROWS[name]), BLOCK_ROWS[name]
    if ls[0] == 2:
        assert BLOCK_ROWS[name][0] == 288
    # the anchors cover the range: first centre half a head cell in, last one half a head cell from the far edge
    a = pp.anchors.build_anchors(d)
    step = SL.VOXEL * d.out_size_factor
    assert a.shape == (A, 7) and abs(a[:, 0].max() - a[:, 0].min() - step * (head[1] - 1)) < 1e-5
    assert abs(a[:, 1].max() - a[:, 1].min() - step * (head[0] - 1)) < 1e-5


def test_layout_table_covers_what_it_is_for():
    """k = 1, 2, 4 and 8 among the transposed convolutions, deconv1 with k = 2, k = 1 behind a stride-1 block for deconv2
    and deconv3, first stride 1 and 2, blocks 2 and 3 at each of (2,2), (1,2), (2,1), (1,1)."""
    ks = {k for v in SL.LAYOUTS.values() for k in v[3]}
    assert ks == {1, 2, 4, 8}
    assert any(v[3][0] == 2 for v in SL.LAYOUTS.values())
    assert any(v[2][1] == 1 and v[3][1] == v[3][0] for v in SL.LAYOUTS.values())
    assert any(v[2][2] == 1 and v[3][2] == v[3][1] for v in SL.LAYOUTS.values())
    assert {v[2][0] for v in SL.LAYOUTS.values()} == {1, 2}
    assert {v[2][1:] for v in SL.LAYOUTS.values()} == {(2, 2), (1, 2), (2, 1), (1, 1)}


@pytest.mark.parametrize("name", SL.NAMES)
def test_layout_problem_margin_targets_and_reference_error(pp, name):
    p = SL.layout_problem(pp, name)
    d = p.d
    assert len(p.frames) == SL.B == 3 and [len(f) for f in p.frames] == list(SL.COUNTS)
    for f in p.frames:      # uniform over the whole range: points in every quadrant of the map
        mid = (d.pc_range[:2] + d.pc_range[3:5]) / 2
        assert {(bool(x), bool(y)) for x, y in (f[:, :2] > mid)} == {(False, False), (False, True), (True, False), (True, True)}
    assert p.labels.shape == (3, d.num_anchors) and p.reg.shape == (3, d.num_anchors, 7)
    assert [int((p.labels[b] > 0).sum()) for b in range(3)] == [40, 13, 13] and p.num_positives == 66
    assert max(SL.POSITIVES) <= d.num_anchors // 4
    assert (p.labels == -1).any() and (p.labels == 0).any()
    vals, g32, _, _, margins, record = p.ref32
    assert vals["num_positives"] == 66
    print(f"{name}: weight seed {p.weight_seed}, smallest distance of a pre-ReLU value / PFN max to its kink {p.margin:.2e}")
    assert p.margin >= SL.MARGIN_BAR, margins
    # the reference alone: float32 against float64 under the float32 run's own decisions
    (wn, wmax), _ = _rel_errors(g32, p.grads64(record))
    print(f"{name}: float32 restatement against float64 under its decisions: worst max-relative gradient difference "
          f"{wmax:.2e} ({wn})")
    assert wmax <= SL.GRAD_BAR / 4, (wn, wmax)
