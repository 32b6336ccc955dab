"""The host restatement of the camera-rig ingest (ingest.Mount / CameraRig / rig_depth_ingest_np / rig_ingest_np): mounts
against hand-fed matrices, the reference mount against the single-camera configuration bit for bit, one- and
three-camera rigs against the single-camera functions, the bounds, the frame-map rules and the C-ABI's declarations."""
import ctypes
import os
import re

import numpy as np
import pytest

import depth_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _yaw_matrix(deg, t):
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = t
    return T


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_from_matrix_equals_the_same_matrices_fed_by_hand(pp):
    ing = pp.ingest
    rng = np.random.default_rng(5)
    p = rng.uniform(-6, 6, (257, 3)).astype(np.float32)
    T = _yaw_matrix(40.0, [0.25, -0.4, 1.1])
    for M in (T, T[:3]):
        m = ing.Mount.from_matrix(M)
        assert np.array_equal(m.r, T[:3, :3].T) and np.array_equal(m.r2, np.eye(3)) and np.array_equal(m.lift, T[:3, 3])
        got = ing.transform_ordered64(p, m.lift, m.matrices)
        want = ing.transform_ordered64(p, T[:3, 3], (T[:3, :3].T, np.eye(3)))
        assert np.array_equal(_bits64(got), _bits64(want))
        # ... which is R p + t for a column vector, up to the rounding of the sum's order
        np.testing.assert_allclose(got, (T[:3, :3] @ p.astype(np.float64).T).T + T[:3, 3], rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match=r"\[4, 4\] or \[3, 4\]"):
        ing.Mount.from_matrix(np.eye(3))
    with pytest.raises(ValueError, match="last row"):
        ing.Mount.from_matrix(np.ones((4, 4)))
    with pytest.raises(ValueError, match="finite"):
        ing.Mount(np.full((3, 3), np.nan))


def test_a_vector_lift_of_a_height_is_the_scalar_lift_bit_for_bit(pp):
    ing = pp.ingest
    p = np.random.default_rng(6).uniform(-6, 6, (100, 3)).astype(np.float32)
    assert np.array_equal(_bits64(ing.transform_ordered64(p, 1.0)), _bits64(ing.transform_ordered64(p, [0.0, 0.0, 1.0])))
    with pytest.raises(ValueError, match="lift has 2 entries"):
        ing.transform_ordered64(p, [0.0, 1.0])


def test_realsense_mount_is_the_single_camera_configuration_bit_for_bit(pp):
    from pp_amd import engine
    rig = pp.ingest.CameraRig([pp.ingest.Mount.realsense()] * 2, first=[1, 2], decimate=[4, 3])
    cfgs = engine._rig_configs(rig, 3)
    assert len(cfgs) == 6
    for s in range(6):
        want = engine._ingest_config((1, 2)[s % 2], (4, 3)[s % 2], pp.ingest.SENSOR_HEIGHT)
        assert bytes(cfgs[s]) == bytes(want), s
    assert ctypes.sizeof(cfgs) == 6 * ctypes.sizeof(pp._lib.PPIngestConfig)
    m = pp.ingest.Mount.realsense(lift=0.4)
    r, r2 = pp.ingest._matrices()
    assert np.array_equal(_bits64(m.r), _bits64(r)) and np.array_equal(_bits64(m.r2), _bits64(r2))
    assert m.lift.tolist() == [0.0, 0.0, 0.4]


def _three_cameras(pp):
    ing, s = pp.ingest, pp.synth
    rng = np.random.default_rng(21)
    images, intrinsics = [], []
    for c, (w, h, enc, pad, big) in enumerate([(8, 6, "16UC1", 1, True), (31, 17, "32FC1", 3, False), (70, 5, "16UC1", 0, False)]):
        z = rng.uniform(0.3, 6.5, (h, w))
        z[rng.random((h, w)) < 0.3] = 0.0
        images.append(s.depth_from_z(z, enc, step_pad=pad, bigendian=big, seed=c))
        intrinsics.append(depth_cases.intr(w, h, c))
    mounts = [ing.Mount.realsense(), ing.Mount.from_matrix(_yaw_matrix(40.0, [0.2, -0.3, 0.9])),
              ing.Mount(np.eye(3)[[2, 0, 1]], np.diag([1.0, -1.0, -1.0]), [0.1, 0.2, 1.3])]
    rig = ing.CameraRig(mounts, intrinsics, first=[1, 0, 2], decimate=[4, 1, 3], z_max=[np.inf, 5.0, np.inf])
    return images, rig


def test_one_camera_rig_equals_depth_ingest_np(pp):
    ing = pp.ingest
    cases = depth_cases.cases(pp)
    for name in ("w73_h7", "f32_bigendian_padded", "clip_u16", "all_zero", "depth_scale_quarter_mm"):
        img, k, kw = cases[name]
        for first, decimate in depth_cases.SELECTIONS:
            rig = ing.CameraRig([ing.Mount.realsense()], k, first=first, decimate=decimate, **kw)
            pts, valid, kept = ing.rig_depth_ingest_np([img], rig)
            want, n_valid = ing.depth_ingest_np(img, k, first, decimate, ing.SENSOR_HEIGHT, **kw)
            assert pts.dtype == np.float32 and pts.shape == want.shape, name
            assert np.array_equal(depth_cases.bits(pts), depth_cases.bits(want)), name
            assert valid.tolist() == [n_valid] and kept.tolist() == [len(want)]


def test_three_camera_rig_equals_the_explicit_concatenation(pp):
    ing = pp.ingest
    images, rig = _three_cameras(pp)
    pts, valid, kept = ing.rig_depth_ingest_np(images, rig)
    parts = []
    for c in range(3):
        xyz = ing.depth_to_xyz(images[c], rig.intrinsics[c], z_max=rig.z_max[c])
        sel = xyz[rig.first[c]::rig.decimate[c]]
        m = rig.mounts[c]
        parts.append(ing.transform_ordered64(sel, m.lift, (m.r, m.r2)).astype(np.float32))
        assert valid[c] == len(xyz) and kept[c] == len(sel) > 0
    assert np.array_equal(depth_cases.bits(pts), depth_cases.bits(np.concatenate(parts)))
    # the same cameras as messages
    msgs = [ing.depth_to_pointcloud2(images[c], rig.intrinsics[c], z_max=rig.z_max[c], ordered=bool(c % 2), point_step=(16, 20, 32)[c])
            for c in range(3)]
    mp, fin, mk = ing.rig_ingest_np(msgs, rig)
    assert np.array_equal(depth_cases.bits(mp), depth_cases.bits(pts)) and mk.tolist() == kept.tolist()
    assert fin.tolist() == valid.tolist()
    with pytest.raises(ValueError, match="2 sources for a rig of 3 cameras"):
        ing.rig_depth_ingest_np(images[:2], rig)


def test_bounds_hold(pp):
    ing = pp.ingest
    images, rig = _three_cameras(pp)
    _, _, kept = ing.rig_depth_ingest_np(images, rig)
    sizes = [(i[1], i[2]) for i in images]
    per = [ing.kept_bound(w, h, rig.first[c], rig.decimate[c]) for c, (w, h) in enumerate(sizes)]
    assert ing.rig_kept_bound(sizes, rig) == sum(per) == 12 + 31 * 17 + 116
    assert all(k <= b for k, b in zip(kept, per))
    full = [pp.synth.depth_from_z(np.full((h, w), 2.0)) for w, h in sizes]      # every pixel valid: the bound is reached
    _, _, kept_full = ing.rig_depth_ingest_np(full, rig)
    assert kept_full.tolist() == per
    with pytest.raises(ValueError, match="decimate 0 < 1"):
        ing.CameraRig([ing.Mount.realsense()], decimate=0)
    with pytest.raises(ValueError, match="first -1 < 0"):
        ing.CameraRig([ing.Mount.realsense()] * 2, first=[1, -1])
    with pytest.raises(ValueError, match="1 to 16 cameras"):
        ing.CameraRig([ing.Mount.realsense()] * 17)
    with pytest.raises(ValueError, match="2 values of decimate for 3 cameras"):
        ing.CameraRig([ing.Mount.realsense()] * 3, decimate=[1, 2])
    with pytest.raises(ValueError, match="2 sets of intrinsics for 3 cameras"):
        ing.CameraRig([ing.Mount.realsense()] * 3, [(1, 1, 0, 0), (1, 1, 0, 0)])


def test_frame_map_checks_raise(pp):
    ing = pp.ingest
    assert ing.check_frame_map([0, 0, 1, 2, 2], 3).tolist() == [0, 0, 1, 2, 2]
    assert ing.check_frame_map([0] * 16 + [1], 2).dtype == np.int32
    for fmap, batch, text in [([1, 1], 2, "source 0: source_frame 1, the frame map starts at frame 0"),
                              ([0, 1, 0], 2, "source 2: source_frame 0 < 1"),
                              ([0, 2], 3, "source 1: source_frame 2 skips frame 1"),
                              ([0, 1], 3, "source 1: source_frame 1, the frame map ends at frame batch - 1 = 2"),
                              ([0, 1, 2], 2, "ends at frame batch - 1 = 1"),
                              ([0] * 17, 1, "source 16: frame 0 has more than 16 sources"),
                              ([], 1, "empty")]:
        with pytest.raises(ValueError, match=re.escape(text)):
            ing.check_frame_map(fmap, batch)
    rig = ing.CameraRig([ing.Mount.realsense()] * 2)
    flat, fmap = ing.rig_frame_map([["a", "b"], ["c", "d"], ["e", "f"]], rig)
    assert flat == list("abcdef") and fmap.tolist() == [0, 0, 1, 1, 2, 2]
    with pytest.raises(ValueError, match="frame 1 has 1 sources, the rig has 2 cameras"):
        ing.rig_frame_map([["a", "b"], ["c"]], rig)
    with pytest.raises(ValueError, match="no frames"):
        ing.rig_frame_map([], rig)


def test_rig_calls_are_declared_exported_and_bound(pp, hip_lib):
    with open(os.path.join(ROOT, "include", "pp_hip.h")) as f:
        hdr = f.read()
    for name in ("pp_ingest_rig_depth", "pp_ingest_rig_depth_async", "pp_ingest_rig_pointcloud2",
                 "pp_ingest_rig_pointcloud2_async", "pp_ingest_rig_info"):
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, flags=re.M), name
        assert name in pp._lib.EXPORTS and hasattr(hip_lib, name)
    m = re.search(r"#define\s+PP_RIG_MAX_SOURCES\s+(\d+)", hdr)
    assert m and int(m.group(1)) == pp._lib.PP_RIG_MAX_SOURCES == pp.ingest.RIG_MAX_SOURCES == 16
    # the rig kernels are built: they live in ingest.hip beside the single-camera ones, in no file of their own
    assert "ingest.hip" in pp._lib.SOURCES
    assert "rig_ingest.hip" not in pp._lib.SOURCES and "depth_ingest.hip" not in pp._lib.SOURCES
