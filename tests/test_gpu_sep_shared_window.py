"""Shared window columns of the stride-1 separable kernels (k_sep_u<..., SH = 1>, k_sep_p<256, 1>).

On an output map whose width is a multiple of 8 a lane takes its left / right window column from the lane quad before /
after it with a DPP row shift and loads a halo column only at the two ends of a row of 16 lanes (8 pixels).  The grids
here are the smallest on which that exchange can go wrong (nx x ny of block1; block2 / block3 are half / a quarter):

  32 x 12   maps 32x12, 16x6, 8x3 (1152 / 288 / 72 pixels at B = 3): a wave's 32 pixels are one image row, two rows,
            four rows -- in block3 every DPP row has both image edges; block2 and block3 end inside a 128-pixel tile and
            inside a wave (a half-filled wave)
  64 x 8    maps 64x8, 32x4, 16x2: block1's halo crosses a wave boundary in the middle of an image row, so it has to be
            the column the lane loaded, not a DPP move
  24 x 12   block1 24 wide (shared path; image rows start at DPP rows 0, 3, 6, ...; 864 pixels = 6.75 tiles), block2 12
            and block3 6 wide: those two take the unchanged kernels in the same engine

Full-width layers (64 / 128 / 256 channels), three frames with clouds of different sizes.  At three frames the planner
would pick the split-K kernel (k_sep_k4); PP_SEP_K4=0 turns it off.  The switch is read once per process, so every case
runs in a child process of its own (this file as a script), which leaves the head maps, the oracle's and the layer tags
in an .npz; the tags show that k_sep_u / k_sep_p really ran (k_sep_p has no lower size limit: B = 3 is enough).

Checks: the head maps against the oracle at the suite's tolerance, and -- 32 x 12 and 64 x 8 -- bit for bit against
tests/golden/sep_shared_window_parent.npz, the same maps (seeded weights and clouds) recorded with the kernels of the
commit before the shared path, e5e8045 ("Live ingest: one kernel body per phase, one C call path, one feeder"):
`python tests/test_gpu_sep_shared_window.py --record` on a build of that commit (PP_HIP_LIB selects another library).
"""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sep_shared_window_parent.npz")
KEYS = ("box_preds", "cls_preds", "dir_cls_preds")
B = 3
# nx, ny, points per frame, seed
CASES = {"32x12": (32, 12, (2600, 900, 1700), 31), "64x8": (64, 8, (3000, 1300, 500), 32), "24x12": (24, 12, (2000, 2900, 700), 33)}
IN_GOLDEN = ("32x12", "64x8")


def _config(pp, nx, ny):
    cfg = copy.deepcopy(pp.config.pedestrian_d435i_config(B))
    cfg["eval_input_reader"]["feature_map_size"] = [1, ny, nx]
    s = cfg["model"]["second"]
    s["voxel_generator"].update(point_cloud_range=[0, -0.04 * ny, -3.0, 0.08 * nx, 0.04 * ny, 3.0], max_number_of_voxels=nx * ny)
    s["target_assigner"]["anchor_generators"]["anchor_generator_stride"].update(offsets=[0.08, -0.04 * ny, -1.465])
    return cfg


def _run_case(case):
    """(child process, PP_SEP_K4=0) head maps of the HIP path and of the oracle, layer tags"""
    import pp_amd as pp
    import util_ref
    nx, ny, npts, seed = CASES[case]
    eng = pp.Engine(_config(pp, nx, ny), max_batch=B, max_points_per_frame=4096)
    d = eng.d
    assert (d.nx, d.ny) == (nx, ny)
    w = pp.weights.init_weights(d, seed=seed)
    eng.load_weights(w)
    rng = np.random.default_rng(seed)
    frames = [rng.uniform([0, -0.04 * ny, -3], [0.08 * nx, 0.04 * ny, 3], (n, 3)).astype(np.float32) for n in npts]
    rect, trv, p2 = pp.synth.default_calib()
    ref = util_ref.oracle_detect(d, w, frames, rect, trv, p2)
    ex = ref["example"]
    out = eng.forward_voxels(ex[0], ex[1], ex[2], B)
    res = {"tags": np.array(eng.layer_tags())}
    for k in KEYS:
        res[k] = out[k]
        res["ref_" + k] = np.asarray(ref["preds"][k], np.float32)
    eng.close()
    return res


def _child(case, path):
    env = dict(os.environ)
    env["PP_SEP_K4"] = "0"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case, path], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", list(CASES))
def test_shared_window_layers_match_oracle_and_parent(hip_lib, golden, tmp_path, case):
    got = _child(case, str(tmp_path / "out.npz"))
    tags = [str(t) for t in got["tags"]]
    by_layer = {t.split(":")[1]: t.split(":")[0] for t in tags}
    for j in range(4):
        assert by_layer[f"block1.{j}"] == "k_sep_u<64,1,3,1,0>", tags
    for j in range(1, 6):
        assert by_layer[f"block2.{j}"] == "k_sep_u<128,1,2,1,0>", tags
        assert by_layer[f"block3.{j}"] == "k_sep_p", tags
    for k in KEYS:
        assert got[k].shape == got["ref_" + k].shape
        err = float(np.abs(got[k] - got["ref_" + k]).max())
        print(f"{case} {k}: max |hip - oracle| = {err:.3e}")
        np.testing.assert_allclose(got[k], got["ref_" + k], rtol=0, atol=TOL)
    if case in IN_GOLDEN:
        for k in KEYS:
            assert np.array_equal(got[k], golden[f"{case}_{k}"]), f"{case} {k}: not bit-identical with the parent's kernels"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if sys.argv[1] == "--record":       # on a build of the parent commit: writes the fixture
        os.environ["PP_SEP_K4"] = "0"
        fix = {}
        for c in IN_GOLDEN:
            r = _run_case(c)
            fix.update({f"{c}_{k}": r[k] for k in KEYS})
        np.savez_compressed(GOLDEN, **fix)
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
    else:
        np.savez(sys.argv[2], **_run_case(sys.argv[1]))
