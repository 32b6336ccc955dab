"""The depth-image rule on the host (ingest.depth_*): depth_ingest_np against the reference-pinned chain
realsense_to_lidar(pointcloud2_to_xyz(message)) on the message a point-cloud node would publish for the image, bit for
bit, for every case of depth_cases.py; the bound; and every refusal by name."""
import numpy as np
import pytest

import depth_cases


@pytest.fixture(scope="module")
def cases(pp):
    return depth_cases.cases(pp)


def _chain(pp, img, intrinsics, kw, first, decimate, **msg_kw):
    ing = pp.ingest
    msg = ing.depth_to_pointcloud2(img, intrinsics, **kw, **msg_kw)
    return ing.realsense_to_lidar(ing.pointcloud2_to_xyz(*msg), decimate, first, ing.SENSOR_HEIGHT), msg


@pytest.mark.parametrize("first,decimate", depth_cases.SELECTIONS)
def test_depth_ingest_np_equals_the_message_chain(pp, cases, first, decimate):
    ing = pp.ingest
    for name, (img, intrinsics, kw) in cases.items():
        got, n_valid = ing.depth_ingest_np(img, intrinsics, first, decimate, ing.SENSOR_HEIGHT, **kw)
        assert got.dtype == np.float32 and got.ndim == 2 and got.shape[1] == 3, (name, got.shape)
        xyz = ing.depth_to_xyz(img, intrinsics, **kw)
        assert xyz.dtype == np.float32 and len(xyz) == n_valid and np.isfinite(xyz).all(), name
        assert len(got) == max(0, -(-(n_valid - first) // decimate)), (name, len(got), n_valid)
        for ordered, point_step in ((False, 16), (True, 16), (True, 20), (True, 32), (False, 20), (False, 32)):
            want, msg = _chain(pp, img, intrinsics, kw, first, decimate, ordered=ordered, point_step=point_step)
            assert msg[3] == point_step and msg[5][:3] == [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1)]
            if ordered:
                assert (msg[1], msg[2]) == (img[1], img[2]), name
            else:
                assert (msg[1], msg[2]) == (n_valid, 1), name
            assert want.shape == got.shape, (name, ordered, point_step, want.shape, got.shape)
            assert np.array_equal(depth_cases.bits(want), depth_cases.bits(got)), (name, first, decimate, ordered, point_step)


def test_the_cases_hold_what_they_are_named_for(pp, cases):
    ing = pp.ingest
    n = {name: ing.depth_ingest_np(img, k, 0, 1, 1.0, **kw)[1] for name, (img, k, kw) in cases.items()}
    assert n["empty_0x0"] == 0 and n["all_zero"] == 0 and n["w1_h1"] == 1
    assert [n[f"w64_h8_valid_{v}"] for v in (511, 512)] == [511, 512]
    assert [n[f"w64_h9_valid_{v}"] for v in (511, 512, 513)] == [511, 512, 513]
    assert n["all_valid"] == 31 * 50
    assert cases["w256_h130_65_chunks"][0][1] * cases["w256_h130_65_chunks"][0][2] == 65 * 512
    assert n["valid_1_keeps_nothing_at_first_1"] == 1 and n["valid_3_keeps_nothing_at_first_3"] == 3
    assert cases["padded_rows_odd_step"][0][3] % 2 == 1 and cases["f32_odd_step"][0][3] % 2 == 1
    # the clip cuts on both sides, keeps z == z_max and drops z == z_min
    for name, (v_lo, u_lo), (v_hi, u_hi) in (("clip_u16", (3, 5), (17, 9)), ("clip_f32", (2, 7), (20, 11))):
        img, k, kw = cases[name]
        unclipped = ing._depth_planes(img, k, kw.get("depth_scale", 0.001), 0.0, np.inf)
        clipped = ing._depth_planes(img, k, kw.get("depth_scale", 0.001), kw["z_min"], kw["z_max"])
        z, was, now = unclipped[2], unclipped[3], clipped[3]
        assert (was & ~now & (z < np.float32(kw["z_min"]))).any() and (was & ~now & (z > np.float32(kw["z_max"]))).any(), name
        assert z[v_lo, u_lo] == np.float32(kw["z_min"]) and was[v_lo, u_lo] and not now[v_lo, u_lo], name
        assert z[v_hi, u_hi] == np.float32(kw["z_max"]) and now[v_hi, u_hi], name
    # 32FC1: NaN, +-inf, negatives and both zeros are there, and none of them is a point
    img, k, kw = cases["f32_little_endian"]
    raw = np.frombuffer(img[0], "<f4").reshape(img[2], img[1])
    assert np.isnan(raw).any() and np.isposinf(raw).any() and np.isneginf(raw).any() and (raw < 0).any()
    assert (np.signbit(raw) & (raw == 0)).any() and (~np.signbit(raw) & (raw == 0)).any()
    assert n["f32_little_endian"] == int((np.isfinite(raw) & (raw > 0)).sum())
    # 32FC1 does not see depth_scale
    img, k, kw = cases["f32_ignores_depth_scale"]
    assert np.array_equal(ing.depth_to_xyz(img, k, depth_scale=0.00025), ing.depth_to_xyz(img, k, depth_scale=0.001))
    # a pixel on the principal point's column has x == 0 exactly
    img, k, kw = cases["principal_point_on_a_pixel"]
    x, _, _, valid = ing._depth_planes(img, k, 0.001, 0.0, np.inf)
    assert (x[:, 20] == 0).all() and valid[:, 20].any()


@pytest.mark.parametrize("first,decimate", depth_cases.SELECTIONS)
def test_depth_kept_bound(pp, cases, first, decimate):
    ing = pp.ingest
    for name, (img, k, kw) in cases.items():
        kept = len(ing.depth_ingest_np(img, k, first, decimate, 1.0, **kw)[0])
        bound = ing.depth_kept_bound(img[1], img[2], first, decimate)
        assert bound >= kept, (name, bound, kept)
        if name == "all_valid":
            assert bound == kept, (bound, kept)


def test_image_as_tuple_and_intrinsics_of(pp):
    ing = pp.ingest

    class Img:
        data, width, height, step, encoding, is_bigendian = bytes(8), 2, 2, 4, "16UC1", 0

    class Info:
        K = [385.5, 0.0, 321.25, 0.0, 384.75, 239.5, 0.0, 0.0, 1.0]
        D = [0.0] * 5

    assert ing.image_as_tuple(Img()) == (bytes(8), 2, 2, 4, "16UC1", False)
    assert ing.image_as_tuple((bytes(8), 2, 2, 4, "16UC1")) == (bytes(8), 2, 2, 4, "16UC1", False)
    with pytest.raises(ValueError, match="5 or 6 entries"):
        ing.image_as_tuple((bytes(8), 2, 2))
    want = (np.float32(385.5), np.float32(384.75), np.float32(321.25), np.float32(239.5))
    for src in (Info(), (Info.K, Info.D), (Info.K,), np.array(Info.K).reshape(3, 3), (385.5, 384.75, 321.25, 239.5)):
        got = ing.intrinsics_of(src)
        assert got == want and all(type(v) is np.float32 for v in got), src
    # the float64 K is cast once
    assert ing.intrinsics_of(([0.1, 0, 1 / 3, 0, 0.7, 2 / 3, 0, 0, 1],)) == tuple(np.float32(v) for v in (0.1, 0.7, 1 / 3, 2 / 3))

    class Distorted(Info):
        D = [0.0, 0.0, 1e-9, 0.0, 0.0]

    for src in (Distorted(), (Info.K, Distorted.D)):
        with pytest.raises(ValueError, match=r"D .*1e-09.*non-zero distortion"):
            ing.intrinsics_of(src)
    with pytest.raises(ValueError, match="K has 4 entries"):
        ing.intrinsics_of(([1, 2, 3, 4], None))


def test_depth_layout_of_refuses_each_bad_field_by_name(pp):
    ing = pp.ingest
    k = (30.0, 31.0, 3.5, 2.5)
    good = (bytes(8 * 6 + 3), 4, 6, 8, "16UC1", False)
    lay = ing.depth_layout_of(good, k)
    assert tuple(lay) == ing.DEPTH_LAYOUT_KEYS
    assert lay == {"width": 4, "height": 6, "row_step": 8, "encoding": 0, "is_bigendian": 0, "fx": 30.0, "fy": 31.0,
                   "ppx": 3.5, "ppy": 2.5, "depth_scale": float(np.float32(0.001)), "z_min": 0.0, "z_max": float("inf")}
    assert ing.depth_layout_of((bytes(9 * 6), 2, 6, 9, "32FC1", True), k)["encoding"] == 1

    def img(**kw):
        t = dict(zip(("data", "width", "height", "step", "encoding", "is_bigendian"), good))
        t.update(kw)
        return tuple(t.values())

    with pytest.raises(ValueError, match=r"step 7 < width 4 x 2 bytes"):
        ing.depth_layout_of(img(step=7), k)
    with pytest.raises(ValueError, match=r"step 15 < width 4 x 4 bytes"):
        ing.depth_layout_of(img(step=15, encoding="32FC1", data=bytes(200)), k)
    for enc in ("8UC1", "rgb8", "16SC1", ""):
        with pytest.raises(ValueError, match=rf"encoding '{enc}' is not a depth encoding"):
            ing.depth_layout_of(img(encoding=enc), k)
    with pytest.raises(ValueError, match=r"Image data holds 51 bytes, 7 rows of step 8 needed"):
        ing.depth_layout_of(img(height=7), k)
    for name, pos in (("fx", 0), ("fy", 1)):
        for bad in (0.0, -0.0, np.inf, -np.inf, np.nan):
            kk = list(k)
            kk[pos] = bad
            with pytest.raises(ValueError, match=rf"^{name} .* focal length"):
                ing.depth_layout_of(good, tuple(kk))
    for name, pos in (("ppx", 2), ("ppy", 3)):
        kk = list(k)
        kk[pos] = np.nan
        with pytest.raises(ValueError, match=rf"^{name} nan is not finite"):
            ing.depth_layout_of(good, tuple(kk))
    for bad in (0.0, -0.001, np.inf, np.nan):
        with pytest.raises(ValueError, match=r"^depth_scale .* finite positive"):
            ing.depth_layout_of(good, k, depth_scale=bad)
        # ... which 32FC1 does not read
        ing.depth_layout_of(img(encoding="32FC1", width=2), k, depth_scale=bad)
    with pytest.raises(ValueError, match=r"^z_min 2.0 > z_max 1.5"):
        ing.depth_layout_of(good, k, z_min=2.0, z_max=1.5)
    assert ing.depth_layout_of(good, k, z_min=1.5, z_max=1.5)["z_min"] == 1.5
    # the functions built on it refuse the same way
    with pytest.raises(ValueError, match="not a depth encoding"):
        ing.depth_to_xyz(img(encoding="bgr8"), k)
    with pytest.raises(ValueError, match="z_min"):
        ing.depth_ingest_np(good, k, 1, 4, 1.0, z_min=3.0, z_max=1.0)
    with pytest.raises(ValueError, match="point_step 8 < 12"):
        ing.depth_to_pointcloud2(good, k, point_step=8)
