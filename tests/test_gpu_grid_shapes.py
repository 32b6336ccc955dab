"""The grid shapes of tests/grid_shape_cases.py on the GPU, whole path against the oracle (`-m gpu`): z cells beyond two,
odd and non-multiple-of-4 widths, the anchor mask's scans past one trip, both sides of the LDS / three-kernel boundary,
the column scan's tail, the sparse canvas with z cells and the occupancy bitmap at a second width.  Per case, through
`detect`: pillar counts, coordinates, point counts and the anchor mask EQUAL to the oracle's, the canvas within 1e-5, the
head maps within TOL * max(1, max |reference map|) (TOL = 1e-4 of test_gpu_parity.py; the scale term is 1 wherever the
older tests run -- nine pillars summed into a cell raise the magnitudes the split-float16 products round against), the
detections through _assert_dets; then the standalone anchor mask and the padded-voxel entry, which are other kernels.
The route is proven, not assumed: the launch names of a profiled pass and the first layer's tag are asserted per case,
and the unprofiled pass (which voxelises on the copy stream and replays a graph) must give the same integer products.

Measured on the MI355X (worst |head map - oracle| / max(1, largest |oracle head map|), through detect and through the
padded-voxel entry; largest |canvas - oracle|; the kernel of block1.0).  Integer products and masks equal everywhere.

  case        largest |head|   detect     padded     canvas     block1.0
  z3               2.01        6.9e-07    7.5e-07    1.9e-06    k_sep_u<32,1,3,1,0>
  z8               4.17        6.6e-07    5.7e-07    3.8e-06    k_sep_u<32,1,3,1,0>
  z9               5.05        7.7e-07    7.7e-07    2.9e-06    k_sep_u<32,1,3,1,0>
  odd              1.33        4.2e-07    5.7e-07    9.5e-07    k_gemm_layer<32,0>
  straddle         1.33        6.1e-07    6.1e-07    1.9e-06    k_sep_u<32,1,3,1,0>
  tall             4.60        7.5e-07    8.2e-07    3.8e-06    k_sep_u<32,1,3,1,0>
  wide             4.23        6.6e-07    7.3e-07    3.8e-06    k_sep_u<32,1,3,1,0>
  lds-in           3.10        6.7e-07    6.9e-07    3.8e-06    k_gemm_layer<32,0>
  lds-out          1.38        7.2e-07    7.0e-07    2.9e-06    k_sep_u<32,1,3,1,0>
  col-tail         3.09        6.5e-07    6.8e-07    3.8e-06    k_sep_u<32,1,3,1,0>
  sparse-z2        3.64        1.3e-06    1.1e-06    7.6e-06    k_sep_u<64,1,3,1,1>
  sparse-z1        3.63        1.1e-06    1.1e-06    4.8e-06    k_sep_u<64,1,3,1,1>

What the cases found:
  * No kernel computed a wrong value on any of these shapes; every case takes the route it is listed for.  The engine
    accepts `odd` and `straddle`: a 27-wide (and the 127-wide lds-in) map runs the generic k_gemm_layer, heads as a layer
    of their own.
  * The profiler named the PFN launch "k_pfn_canvas" whichever kernel ran, so the route could not be read off
    kernel_times(); the launch now goes under the name of the kernel launch_pfn chooses.
  * sparse-z1: pp_anchor_mask after a pass on a one-z-cell sparse grid launched k_anchor_lookup_bits on the occupancy
    BITMAP that pass had left, not the three kernels on the cell map it had just built from the caller's coordinates
    (the pass's `occbits_live` outlived it; seen as the launch name, once, without the fix).  The standalone call here
    swaps the two frames so that nothing of the pass before can answer for it; pp_anchor_mask now clears the flag.
  * With the first seeds tried, lds-out and sparse-z2 had the oracle keep boxes 61 m and 746 m long (exp of a large size
    logit under random weights); there the head maps agreed to 7e-7 and 1.3e-6 of their scale and the decoded boxes
    differed by 1.4e-4 and 7.3e-4 -- the logit's float32 rounding times the box's own length, which an absolute 1e-4
    cannot resolve (the fuzz sweep's qualification (2)).  The bar stays; the two seeds were replaced and
    test_grid_shape_cases_host.py asserts, on the oracle's values alone, that a case's boxes are resolvable.
"""
import re

import numpy as np
import pytest

import grid_shape_cases as gc
from test_gpu_parity import TOL, _assert_dets

pytestmark = pytest.mark.gpu

MASK_KERNELS = {"k_anchor_mask_frame", "k_occ_rowscan", "k_colscan", "k_anchor_lookup", "k_anchor_lookup_bits"}
THREE = {"k_occ_rowscan", "k_colscan", "k_anchor_lookup"}
# case -> (the PFN kernel, the mask launches of `detect`, the mask launches of the standalone call)
ROUTE = {
    "z3": ("k_pfn_canvas2", set(), {"k_anchor_mask_frame"}),
    "z8": ("k_pfn_canvas2", set(), {"k_anchor_mask_frame"}),
    "z9": ("k_pfn_canvas", {"k_anchor_mask_frame"}, {"k_anchor_mask_frame"}),
    "odd": ("k_pfn_canvas2", set(), {"k_anchor_mask_frame"}),
    "straddle": ("k_pfn_canvas2", set(), {"k_anchor_mask_frame"}),
    "tall": ("k_pfn_canvas2", set(), {"k_anchor_mask_frame"}),
    "wide": ("k_pfn_canvas2", set(), {"k_anchor_mask_frame"}),
    "lds-in": ("k_pfn_canvas2", set(), {"k_anchor_mask_frame"}),
    "lds-out": ("k_pfn_canvas2", THREE, THREE),
    "col-tail": ("k_pfn_canvas2", THREE, THREE),
    "sparse-z2": ("k_pfn_canvas2", THREE, THREE),
    "sparse-z1": ("k_pfn_canvas2", {"k_anchor_lookup_bits"}, THREE),
}
SPARSE_TAG = re.compile(r"^k_sep_u<\d+,1,\d+,1,1>:block1\.0$")     # the form of test_gpu_parity._TAGS_K32[0]: OCC = 1
HEADS = ("box_preds", "cls_preds", "dir_cls_preds")


def _names(eng):
    return [n.split(":")[0] for n, _ in eng.kernel_times()]


def _head_errors(got, ref, worst):
    for k in HEADS:
        scale = max(1.0, float(np.abs(ref[k]).max()))
        err = float(np.abs(got[k] - ref[k]).max())
        worst[k] = max(worst.get(k, 0.0), err / scale)
        assert got[k].shape == ref[k].shape
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=TOL * scale, err_msg=k)


def _integer_products(im, ref):
    out = []
    for b, fr in enumerate(ref["frames"]):
        P = fr["coordinates"].shape[0]
        assert im["n_pillars"][b] == P, (b, im["n_pillars"][b], P)
        assert np.array_equal(im["coors"][b, :P], fr["coordinates"]), b
        assert np.array_equal(im["num_points"][b, :P], fr["num_points"]), b
        assert np.array_equal(im["anchors_mask"][b].astype(bool), fr["anchors_mask"]), b
        out.append(im["coors"][b, :P].tobytes() + im["num_points"][b, :P].tobytes() + im["anchors_mask"][b].tobytes())
    return out


@pytest.mark.parametrize("name", gc.NAMES)
def test_grid_shape_against_the_oracle(pp, hip_lib, name):
    case = gc.BY_NAME[name]
    d, w, frames, ref = gc.reference(case)
    pfn_kernel, mask_in_detect, mask_alone = ROUTE[name]
    B = gc.B
    eng = pp.Engine(gc.config(case), max_batch=B, max_points_per_frame=gc.NMAX)
    try:
        eng.load_weights(w)
        rect, trv, _ = pp.synth.default_calib()
        rects, trvs = np.stack([rect] * B), np.stack([trv] * B)
        # ---- a profiled pass: plain launches, the voxeliser on the main stream; every launch under its kernel's name ----
        eng.set_profiling(True)
        dets_p, n_p = eng.detect(frames, rects, trvs)
        names = _names(eng)
        eng.set_profiling(False)
        assert {n for n in names if n.startswith("k_pfn_canvas")} == {pfn_kernel}, names
        assert {n for n in names if n in MASK_KERNELS} == mask_in_detect, names
        tags = eng.layer_tags()
        sparse = name.startswith("sparse")
        assert bool(SPARSE_TAG.match(tags[0])) == sparse, tags[0]
        prods_p = _integer_products(eng.intermediates(), ref)
        # ---- the pass as it runs in production ----
        dets, n = eng.detect(frames, rects, trvs)
        im = eng.intermediates(canvas=True)
        assert _integer_products(im, ref) == prods_p
        assert np.array_equal(n, n_p) and dets.tobytes() == dets_p.tobytes()
        np.testing.assert_allclose(im["canvas"], ref["canvas"], rtol=1e-5, atol=1e-5)
        if sparse:
            assert (np.abs(im["canvas"]).sum(axis=-1) == 0).mean() > 0.9, "mostly empty grid"
        worst = {}
        _head_errors(im, ref["preds"], worst)
        _assert_dets([pp.VoxelNet._to_dict(dets[b], int(n[b]), b) for b in range(B)], ref["dets"])
        assert eng.layer_tags() == tags
        # ---- the standalone anchor mask (k_anchor_mask_frame at 1024 threads, or the three kernels; never the bitmap, which
        # belongs to the pass before): the oracle's coordinates with the two frames swapped, so nothing of that pass answers
        ex = ref["example"]
        swapped = ex[2].copy()
        swapped[:, 0] = B - 1 - swapped[:, 0]
        eng.set_profiling(True)
        m = eng.anchor_mask(swapped, B)
        alone = _names(eng)
        eng.set_profiling(False)
        assert set(alone) == mask_alone, alone
        for b in range(B):
            assert np.array_equal(m[B - 1 - b].astype(bool), ref["frames"][b]["anchors_mask"]), b
        assert not np.array_equal(m[0], m[1])
        # ---- the padded-voxel entry: k_pfn_canvas on the whole pseudo-image; on the sparse grids block1.0 looks every window
        # position up in the cell map built from the given coordinates (occ_nz cells deep), without the bitmap
        eng.set_profiling(True)
        out = eng.forward_voxels(ex[0], ex[1], ex[2], B, want_canvas=True)
        padded = _names(eng)
        eng.set_profiling(False)
        assert {n for n in padded if n.startswith("k_pfn_canvas")} == {"k_pfn_canvas"}, padded
        assert eng.layer_tags() == tags
        np.testing.assert_allclose(out["canvas"], ref["canvas"], rtol=1e-5, atol=1e-5)
        worst_padded = {}
        _head_errors(out, ref["preds"], worst_padded)
        scale = max(float(np.abs(ref["preds"][k]).max()) for k in HEADS)
        print(f"{name}: block1.0 {tags[0]}; largest |reference head map| {scale:.3g}; worst head error / max(1, scale) "
              f"detect {max(worst.values()):.2e}, padded entry {max(worst_padded.values()):.2e} (bar {TOL:.0e}); canvas "
              f"{float(np.abs(im['canvas'] - ref['canvas']).max()):.2e}")
    finally:
        eng.close()
