"""Host side of the PointCloud2 feature ingest: ingest_np(msg, features=...) -- the rule the GPU kernels implement -- held
bit for bit to the package's x y z chain realsense_to_lidar(pointcloud2_to_xyz(...)) column-stacked with the numpy feature
expression on the same kept records; the feature table feature_layout_of resolves, and its refusals.  No GPU."""
import numpy as np
import pytest

import pc2_cases
import pc2_feature_cases as fc


@pytest.fixture(scope="module")
def cases(pp):
    return fc.feature_cases(pp)


def test_case_list_covers_what_the_feature_decode_must_read(pp, cases):
    ing = pp.ingest
    tables = {k: ing.feature_layout_of(m, f)[0] for k, (m, f) in cases.items()}
    lay = {k: ing.layout_of(m) for k, (m, _) in cases.items()}
    assert {t[1] for t in tables.values()} == set(range(9))                  # every datatype, and the constant
    offs = {k: (tables[k][0], sorted(lay[k][a] for a in ("x_offset", "y_offset", "z_offset"))) for k in cases if tables[k][1]}
    assert any(o < x[0] for o, x in offs.values()) and any(x[0] < o < x[2] for o, x in offs.values())
    assert any(o > x[2] for o, x in offs.values())
    assert tables["unaligned_13_of_29"][0] == 13 and lay["unaligned_13_of_29"]["point_step"] == 29
    assert any(v["row_step"] > v["width"] * v["point_step"] for v in lay.values())
    assert any(v["is_bigendian"] for v in lay.values())
    assert lay["f64xyz_uint16"]["datatype"] == 8 and tables["f64xyz_uint16"][1] == 4
    assert tables["count3_index2"][:2] == (12 + 2 * 2, 4)
    v = lay["velodyne"]
    assert v["point_step"] == 32 and tables["velodyne"][:2] == (16, 7)
    assert ("ring", 20, 4, 1) in [tuple(f) for f in ing.as_tuple(cases["velodyne"][0])[5]]
    assert lay["one_row_partial_chunk"]["width"] == 1500
    assert all(v["width"] * v["height"] <= 64 * 48 for v in lay.values())
    finite = {k: fc.host_points(pp, *cases[k], 0, 1)[1] for k in ("finite_0", "finite_1")}
    assert finite == {"finite_0": 0, "finite_1": 1}
    # the extreme values sit on kept points
    want = fc.host_points(pp, *cases["int32_extremes"], 0, 1)[0][:, 3]
    assert want[0] == np.float32(-2.0 ** 31 + 0.5) and want[1] == np.float32(2.0 ** 31 - 0.5)
    want = fc.host_points(pp, *cases["uint32_extremes"], 0, 1)[0][:, 3]
    assert want[0] == np.float32((2.0 ** 32 - 1) * 1e-3 + -1e-7)
    want = fc.host_points(pp, *cases["float32_special_identity"], 0, 1)[0][:, 3]
    assert want[:5].tolist() == [np.float32(v) for v in (1e-40, -1e-40, 1.4e-45, fc.F32_MAX, -fc.F32_MAX)]
    assert pc2_cases.bits(want[5:7]).tolist() == [0, 0]              # (-0 * 1 + 0 is +0 in IEEE arithmetic)
    want = fc.host_points(pp, *cases["float32_special_bias"], 0, 1)[0][:, 3]
    assert pc2_cases.bits(want[5:7]).tolist() == [0, 0x80000000]
    want = fc.host_points(pp, *cases["float32_special_scaled"], 0, 1)[0][:, 3]
    assert np.isposinf(want[3]) and np.isneginf(want[4])
    want = fc.host_points(pp, *cases["nonfinite_feature_f32"], 0, 1)[0]
    assert np.isnan(want[0, 3]) and np.isposinf(want[1, 3]) and np.isneginf(want[2, 3]) and np.isfinite(want[:, :3]).all()
    # a bias that makes the float64 sum inexact: the float64 result differs from the exactly rounded one somewhere
    from fractions import Fraction
    msg, (f,) = cases["uint16_bias_inexact"]
    assert any(Fraction(float(r) * f.scale) + Fraction(f.bias) != Fraction(float(r) * f.scale + f.bias) for r in range(1, 50))


@pytest.mark.parametrize("first,decimate", fc.SELECTIONS)
def test_ingest_np_with_features_equals_the_xyz_chain_and_the_numpy_expression(pp, cases, first, decimate):
    ing = pp.ingest
    for name, (msg, feats) in cases.items():
        want, n_finite = fc.host_points(pp, msg, feats, first, decimate)
        with np.errstate(over="ignore"):
            got, n = ing.ingest_np(msg, first, decimate, features=feats)
            xyz_only, n3 = ing.ingest_np(msg, first, decimate)
        assert n == n_finite == n3, name
        fc.assert_same_points(got, want, (name, first, decimate))
        # columns 0 - 2 and the counts are the x y z ingest's
        assert np.array_equal(pc2_cases.bits(got[:, :3]), pc2_cases.bits(xyz_only)), name
        assert len(got) == len(xyz_only) <= ing.kept_bound(msg[1], msg[2], first, decimate), name


def test_pointcloud2_to_points_columns_and_nan_removal(pp, cases):
    ing = pp.ingest
    for name, (msg, feats) in cases.items():
        full = ing.pointcloud2_to_points(msg, feats, remove_nans=False)
        xyz = ing.pointcloud2_to_xyz(*msg, remove_nans=False)
        assert full.shape == (len(xyz), 4) and full.dtype == xyz.dtype, name
        assert np.array_equal(full[:, :3], xyz, equal_nan=True), name
        col = fc.numpy_feature(pp, msg, feats[0])
        assert np.array_equal(full[:, 3].astype(np.float32), col, equal_nan=True), name
        fin = np.isfinite(xyz).all(axis=1)
        kept = ing.pointcloud2_to_points(msg, feats)
        assert np.array_equal(kept, full[fin], equal_nan=True), name
    # a record is dropped for x y z only: non-finite feature values stay
    kept = ing.pointcloud2_to_points(*cases["nonfinite_feature_f32"])
    assert np.isnan(kept[:, 3]).any() and np.isinf(kept[:, 3]).any() and np.isfinite(kept[:, :3]).all()
    # no features: the x y z array
    msg = cases["velodyne"][0]
    assert np.array_equal(ing.pointcloud2_to_points(msg, []), ing.pointcloud2_to_xyz(*msg))


def test_two_features_and_names_given_as_strings(pp, cases):
    ing = pp.ingest
    msg = cases["velodyne"][0]
    feats = [ing.FeatureField("intensity", 1.0 / 255.0), ing.FeatureField("ring", 1.0, 0.5)]
    got, _ = ing.ingest_np(msg, 0, 1, features=feats)
    want, _ = fc.host_points(pp, msg, feats, 0, 1)
    assert got.shape[1] == 5
    fc.assert_same_points(got, want, "two features")
    assert ing.feature_layout_of(msg, ["intensity", "ring"]) == [(16, 7, 1.0, 0.0), (20, 4, 1.0, 0.0)]
    assert ing.feature_layout_of(msg, [ing.FeatureField.constant(2.5)]) == [(0, 0, 1.0, 2.5)]


def test_rig_ingest_np_with_features_is_the_concatenation(pp, cases):
    ing = pp.ingest
    names = ["velodyne", "bigendian_int16", "constant"]
    msgs = [cases[n][0] for n in names]
    per = [cases[n][1] for n in names]
    r, r2 = ing._matrices()
    rig = ing.CameraRig([ing.Mount.realsense(), ing.Mount(np.eye(3), None, 0.0), ing.Mount(r, r2, [0.1, 0.2, 0.3])],
                        first=[0, 1, 2], decimate=[1, 4, 3])
    got, fin, kept = ing.rig_ingest_np(msgs, rig, per)
    parts = [ing.ingest_np(m, rig.first[c], rig.decimate[c], rig.mounts[c].lift, rig.mounts[c].matrices, per[c])
             for c, m in enumerate(msgs)]
    assert got.shape == (sum(len(p) for p, _ in parts), 4)
    fc.assert_same_points(got, np.concatenate([p for p, _ in parts]), "rig")
    assert fin.tolist() == [n for _, n in parts] and kept.tolist() == [len(p) for p, _ in parts]
    # without features nothing changes
    assert ing.rig_ingest_np(msgs, rig)[0].shape[1] == 3
    # one list for every camera
    same = ing.rig_ingest_np(msgs, rig, [ing.FeatureField.constant(1.0)])[0]
    assert same.shape[1] == 4 and (same[:, 3] == 1.0).all()
    with pytest.raises(ValueError, match="2 feature lists for a rig of 3 cameras"):
        ing.rig_ingest_np(msgs, rig, per[:2])


def test_feature_layout_of_refusals_name_the_fields(pp, cases):
    ing = pp.ingest
    msg = cases["count3_index2"][0]
    with pytest.raises(ValueError, match=r"feature 0: the message has no field 'intensity'; its fields are x .*echo \(datatype 4, count 3\)"):
        ing.feature_layout_of(msg, [ing.FeatureField("intensity")])
    with pytest.raises(ValueError, match=r"feature 1: index 3 >= count 3 of field 'echo'.*fields are x "):
        ing.feature_layout_of(msg, [ing.FeatureField("echo"), ing.FeatureField("echo", index=3)])
    with pytest.raises(ValueError, match=r"index 1 >= count 1 of field 'x'"):
        ing.feature_layout_of(msg, [ing.FeatureField("x", index=1)])
    with pytest.raises(ValueError, match="no field 'intensity'"):
        ing.ingest_np(msg, features=[ing.FeatureField("intensity")])
    with pytest.raises(ValueError, match="index -1 < 0"):
        ing.FeatureField("echo", index=-1)
    for bad in (dict(scale=np.nan), dict(scale=np.inf), dict(bias=-np.inf), dict(bias=np.nan)):
        with pytest.raises(ValueError, match="must be finite"):
            ing.FeatureField("echo", **bad)
    with pytest.raises(ValueError, match="must be finite"):
        ing.FeatureField.constant(np.inf)


def test_synth_message_round_trips_a_kitti_shaped_array(pp):
    pts = pp.synth.kitti_cloud(3, 1500)
    msg = pp.synth.pointcloud2_from_points(pts, 1500, 1, feature_fields=[("intensity", 7, 16)], point_step=32,
                                           extra_fields=[("ring", 20, 4, 1)])
    back = pp.ingest.pointcloud2_to_points(msg, [pp.ingest.FeatureField("intensity")])
    assert back.dtype == np.float32 and back.tobytes() == pts.tobytes()
    got, n = pp.ingest.ingest_np(msg, 0, 1, 0.0, (np.eye(3), np.eye(3)), features=[pp.ingest.FeatureField("intensity")])
    assert n == 1500
    assert np.array_equal(got[:, 3], pts[:, 3])
    assert np.array_equal(got[:, :3], pts[:, :3])         # (values: an identity mount adds +0, which turns a -0 into +0)
    with pytest.raises(ValueError, match="do not fit point_step"):
        pp.synth.pointcloud2_from_points(pts, 1500, 1, feature_fields=[("intensity", 7, 30)], point_step=32)
