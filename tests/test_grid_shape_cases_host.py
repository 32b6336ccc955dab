"""The cases of tests/grid_shape_cases.py land where they are aimed, checked on the host alone (no GPU): the launch
predicates are restated from the constants READ OUT OF THE SOURCES, so a later change of AM_MAX_CELLS, PFN2_CW or the
sparse-canvas thresholds fails here instead of silently emptying a case of tests/test_gpu_grid_shapes.py; and the oracle's
result on every case has what makes the case mean something (a column full in z, a mask that is neither all set nor all
clear, no max_voxels break in the large frame, a detection)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import grid_shape_cases as gc

CSRC = os.path.join(ROOT, "3d-object-detection-for-autonomous-navigation_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constants():
    am, pfn, api, mask = (_source(n) for n in ("anchor_mask_dev.h", "pfn.hip", "pp_api.hip", "anchor_mask.hip"))
    c = {"AM_MAX_CELLS": int(re.search(r"#define\s+AM_MAX_CELLS\s+(\d+)\b", am).group(1)),
         "PFN2_CW": int(re.search(r"#define\s+PFN2_CW\s+(\d+)\b", pfn).group(1)),
         "MASK_IN_PFN_MAX_BATCH": int(re.search(r"kAnchorMaskInPfnMaxBatch = (\d+);", api).group(1))}
    m = re.search(r"cells >= (\d+) && (\d+)ll \* e->cfg\.max_voxels <= cells", api)
    c["SPARSE_MIN_CELLS"], c["SPARSE_VOXEL_FACTOR"] = int(m.group(1)), int(m.group(2))
    # the forms of the predicates the restatements copy
    assert "ny * (nx | 1) <= AM_MAX_CELLS" in mask and "p.ny * (p.nx | 1) <= AM_MAX_CELLS" in pfn
    assert pfn.count("PFN2_CW * p.nz <= 64") == 3                 # the mask's ride, the pillar-centric kernel, launch_pfn_t
    assert "if ((plane & 3) == 0 && nz <= 2) {" in am and "ls = nx | 1" in am
    assert "for (int x0 = 0; x0 < nx; x0 += 64)" in am and "for (int y0 = 0; y0 < ny; y0 += 64)" in am
    assert "for (; y + 8 <= ny; y += 8)" in mask
    assert "if (e->occbits_live && e->nz == 1)" in api
    return c


def _route(case, c):
    """What a two-frame detect launches for the case, from the restated predicates."""
    sparse = gc.sparse_canvas(case.nx, case.ny, case.max_voxels, c["SPARSE_MIN_CELLS"], c["SPARSE_VOXEL_FACTOR"])
    pfn2 = gc.pfn_second_generation(case.nz, c["PFN2_CW"])
    fits = gc.lds_image_fits(case.nx, case.ny, c["AM_MAX_CELLS"])
    if sparse and pfn2:
        return ("k_pfn_canvas2:pillars", "bits" if case.nz == 1 else ("frame" if fits else "three"))
    if pfn2 and fits and not sparse and gc.B <= c["MASK_IN_PFN_MAX_BATCH"]:
        return ("k_pfn_canvas2", "in-pfn")
    return ("k_pfn_canvas2" if pfn2 else "k_pfn_canvas", "frame" if fits else "three")


ROUTES = {"z3": ("k_pfn_canvas2", "in-pfn"), "z8": ("k_pfn_canvas2", "in-pfn"), "z9": ("k_pfn_canvas", "frame"),
          "odd": ("k_pfn_canvas2", "in-pfn"), "straddle": ("k_pfn_canvas2", "in-pfn"), "tall": ("k_pfn_canvas2", "in-pfn"),
          "wide": ("k_pfn_canvas2", "in-pfn"), "lds-in": ("k_pfn_canvas2", "in-pfn"), "lds-out": ("k_pfn_canvas2", "three"),
          "col-tail": ("k_pfn_canvas2", "three"), "sparse-z2": ("k_pfn_canvas2:pillars", "three"),
          "sparse-z1": ("k_pfn_canvas2:pillars", "bits")}


def test_every_case_lands_on_its_side_of_the_launch_predicates():
    c = _constants()
    assert gc.NAMES == list(ROUTES)
    for case in gc.CASES:
        d = gc.pp.config.Derived(gc.config(case))
        assert (d.nx, d.ny, d.nz) == (case.nx, case.ny, case.nz), case.name
        assert d.layer_strides == list(case.strides) and d.layer_nums == [1, 1, 1] and d.max_voxels == case.max_voxels
        assert (d.head_h, d.head_w) == (case.ny, case.nx) and d.num_point_features == 3
        assert _route(case, c) == ROUTES[case.name], case.name
    by = gc.BY_NAME
    cw = c["PFN2_CW"]
    # 1: lane / nz with nz no power of two; a full wave of slots.  2: one z cell more and the wave does not hold them
    assert by["z3"].nz & (by["z3"].nz - 1) and cw * by["z3"].nz < 64
    assert cw * by["z8"].nz == 64 and cw * by["z9"].nz > 64 and by["z9"].nz == by["z8"].nz + 1
    assert (by["z8"].nx, by["z8"].ny) == (by["z9"].nx, by["z9"].ny)
    # 3, 4, 10: the sparse canvas at its two thresholds, with and without z cells; the bitmap at a second width
    for n in ("sparse-z2", "sparse-z1"):
        s = by[n]
        assert s.nx * s.ny == c["SPARSE_MIN_CELLS"] and c["SPARSE_VOXEL_FACTOR"] * s.max_voxels == s.nx * s.ny
        assert s.widths == gc.SHIPPED
    assert by["sparse-z2"].nz == 2 and by["sparse-z1"].nz == 1
    # (the bitmap's rows: 6 words at 256 cells, 8 on the KITTI-shaped grid, the one width k_anchor_lookup_bits had seen)
    assert re.search(r"occ_words\(int nx\) \{ return \(nx \+ 2 \+ 63\) / 64 \+ 1; \}", _source("pp_common.h"))
    kitti = gc.pp.config.Derived(gc.pp.config.kitti_shaped_config(1))
    assert (by["sparse-z1"].nx + 2 + 63) // 64 + 1 == 6 and (kitti.nx + 2 + 63) // 64 + 1 == 8
    # 5: the scalar occupancy load, by nz and by the plane; 6: the 16-byte load across a row end
    assert not gc.mask_vector_load(by["z3"].nx, by["z3"].ny, by["z3"].nz) and (by["z3"].nx * by["z3"].ny) % 4 == 0
    assert not gc.mask_vector_load(by["odd"].nx, by["odd"].ny, by["odd"].nz) and by["odd"].nz == 1
    s = by["straddle"]
    assert gc.mask_vector_load(s.nx, s.ny, s.nz) and s.nx % 4 == 2
    # (cells 4i .. 4i + 3 of some i lie in two rows)
    assert any((4 * i) // s.nx != (4 * i + 3) // s.nx for i in range(s.nx * s.ny // 4))
    # 7: the scans' further trips, inside the LDS image
    assert by["tall"].ny > 64 and by["tall"].nx <= 128 and by["wide"].nx > 128 and by["wide"].ny <= 64
    # 8: the boundary from both sides -- the padded image, not the cell count, decides
    i, o = by["lds-in"], by["lds-out"]
    assert i.ny * (i.nx | 1) == 8128 <= c["AM_MAX_CELLS"] < o.ny * (o.nx | 1) == 8256 and o.nx * o.ny == c["AM_MAX_CELLS"]
    # 9: the column scan's tail
    assert by["col-tail"].ny % 8 == 4
    # odd / straddle: stride-1 blocks at a width the uniform-wave kernels do not take
    assert by["odd"].nx % 2 == 1 and by["odd"].strides == (1, 1, 1) == by["straddle"].strides
    covered = {r for case in gc.CASES for r in case.rows}
    assert covered == set(range(1, 11))                              # (11 is the costmap's: tests/test_costmap_host.py)


@pytest.mark.parametrize("name", gc.NAMES)
def test_the_oracle_result_makes_the_case_mean_something(name):
    case = gc.BY_NAME[name]
    d, w, frames, ref = gc.reference(case)
    assert [f.shape[1] for f in frames] == [3, 3] and all(len(f) <= gc.NMAX for f in frames)
    assert abs(len(frames[0]) - gc.ROWS[0]) < 100 and abs(len(frames[1]) - gc.ROWS[1]) < 100
    z = frames[0][:, 2]
    assert z.min() < d.pc_range[2] and z.max() > d.pc_range[5]        # rows beyond both ends of the z range
    on = []
    for b, fr in enumerate(ref["frames"]):
        co = fr["coordinates"]                                      # (z, y, x)
        P = len(co)
        assert len(np.unique((co[:, 0] * d.ny + co[:, 1]) * d.nx + co[:, 2])) == P
        per_col = np.zeros((d.ny, d.nx), np.int64)
        np.add.at(per_col, (co[:, 1], co[:, 2]), 1)
        assert per_col.max() == d.nz, (name, b)                     # some column holds a pillar in every z cell
        if b == 0:
            assert P < d.max_voxels, (name, P)                      # the max_voxels break would hide columns
            assert P > 100 * d.nz
        if name == "sparse-z2":
            top = np.zeros((d.ny, d.nx), bool)
            top[co[co[:, 0] == 1][:, 1], co[co[:, 0] == 1][:, 2]] = True
            assert (top & (per_col == 1)).any() and (top & (per_col == 2)).any(), b
        on.append(float(fr["anchors_mask"].mean()))
    print(f"{name}: pillars {[len(f['coordinates']) for f in ref['frames']]}, anchors on {on}, "
          f"detections {[0 if r['scores'] is None else len(r['scores']) for r in ref['dets']]}, "
          f"largest |head map| {max(float(np.abs(v).max()) for v in ref['preds'].values()):.3g}")
    assert any(0.05 <= f <= 0.95 for f in on), on
    assert any(r["scores"] is not None and len(r["scores"]) >= 1 for r in ref["dets"])
    # _assert_dets holds the decoded boxes to an ABSOLUTE 1e-4.  A head value is a float32 sum of several hundred terms whose
    # partial sums reach `scale`, so two correct evaluations differ by some units in the last place of scale (8 taken here);
    # a decoded size is anchor * exp(logit) and moves by its own length times the logit's error.  The bar can only be met
    # while box * 8 ulp(scale) stays under it: weights under which the oracle keeps a box hundreds of metres long (it
    # happens: random weights, exp of a logit of 5) make a case no float32 implementation other than the oracle passes.
    scale = max(1.0, max(float(np.abs(v).max()) for v in ref["preds"].values()))
    box = max(float(np.abs(r[k]).max()) for r in ref["dets"] if r["scores"] is not None for k in ("box3d_lidar", "box3d_camera"))
    assert box * 8 * 2.0 ** -23 * scale <= 1e-4, (name, box, scale)
