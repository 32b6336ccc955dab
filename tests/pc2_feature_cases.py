"""Synthetic sensor_msgs/PointCloud2 messages with feature fields beside x y z, shared by test_ingest_features_host.py,
test_gpu_ingest_features.py and test_gpu_rig_ingest_features.py: every datatype, position, byte order and value the
feature decode has to read, each with the FeatureFields it is ingested under.  The selections are pc2_cases.SELECTIONS."""
import copy

import numpy as np

import pc2_cases

SELECTIONS = pc2_cases.SELECTIONS

F32_MAX = 3.4028234663852886e38


def config4(pp, B, base="tiny"):
    """A 4-feature variant of a small shipped config (x y z intensity), as tests/test_gpu_train.py builds its own."""
    cfg = copy.deepcopy(pp.config.tiny_config(B) if base == "tiny" else pp.config.pedestrian_d435i_config(B))
    cfg["model"]["second"]["num_point_features"] = 4
    for reader in ("eval_input_reader", "train_input_reader"):
        if reader in cfg:
            cfg[reader]["num_point_features"] = 4
    return cfg


def _xyz(rng, n, nan_fraction=0.3):
    xyz = rng.uniform(-3.0, 6.0, (n, 3))
    bad = rng.random(n) < nan_fraction
    xyz[bad, rng.integers(0, 3, int(bad.sum()))] = np.nan
    return xyz


def _ints(rng, n, lo, hi, extremes=()):
    v = rng.integers(lo, hi, n, endpoint=True).astype(np.float64)
    v[:len(extremes)] = extremes
    return v


def _sparse_xyz(n, n_finite):
    rng = np.random.default_rng(100 + n_finite)
    xyz = np.full((n, 3), np.nan)
    rows = np.sort(rng.choice(n, n_finite, replace=False))
    xyz[rows] = rng.uniform(-3.0, 6.0, (n_finite, 3))
    return xyz


def feature_cases(pp):
    """name -> (message tuple, [FeatureField]).  The first records of the value cases are made finite so that the
    extreme feature values sit on kept points at selection (0, 1)."""
    s, FF = pp.synth, pp.ingest.FeatureField
    rng = np.random.default_rng(17)
    cases = {}

    def add(name, w, h, col, fields, feats, finite_head=0, nan_fraction=0.3, xyz=None, **kw):
        xyz = _xyz(rng, w * h, nan_fraction) if xyz is None else xyz
        if finite_head:
            xyz[:finite_head] = rng.uniform(-3.0, 6.0, (finite_head, 3))
        pts = np.concatenate([xyz, np.asarray(col, np.float64).reshape(w * h, 1)], axis=1)
        cases[name] = (s.pointcloud2_from_points(pts, w, h, feature_fields=fields, seed=300 + len(cases), **kw), feats)

    n = 64 * 48
    # the eight datatypes; the feature before, between and after x y z; padded rows; scales and biases
    add("int8_before", 64, 48, _ints(rng, n, -128, 127, (-128, 127, 0)), [("i", 1, 0)], [FF("i", 0.5, -3.0)], 3,
        point_step=16, offsets=(4, 8, 12))
    add("uint8_scale_1_255", 64, 48, _ints(rng, n, 0, 255, (0, 255, 1, 254)), [("reflectivity", 2, 12)],
        [FF("reflectivity", 1.0 / 255.0)], 4, point_step=13, row_pad=7)
    add("int16_between", 50, 31, _ints(rng, 50 * 31, -32768, 32767, (-32768, 32767, -1)), [("i", 3, 4)], [FF("i", 1e-3, 0.1)], 3,
        point_step=16, offsets=(0, 6, 10), row_pad=5)
    # (0.1 is no float64 sum of a multiple of 0.001 and itself: the sum is inexact, and so is 0.001 * raw)
    add("uint16_bias_inexact", 64, 48, _ints(rng, n, 0, 65535, (0, 65535, 1, 3)), [("reflectivity", 4, 12)],
        [FF("reflectivity", 0.001, 0.1)], 4, point_step=14)
    add("int32_extremes", 40, 25, _ints(rng, 1000, -2 ** 31, 2 ** 31 - 1, (-2 ** 31, 2 ** 31 - 1, 0, -1, 16777217)),
        [("i", 5, 12)], [FF("i", 1.0, 0.5)], 5, point_step=20)
    add("uint32_extremes", 40, 25, _ints(rng, 1000, 0, 2 ** 32 - 1, (2 ** 32 - 1, 0, 2 ** 31, 16777217)),
        [("i", 6, 16)], [FF("i", 1e-3, -1e-7)], 4, point_step=20)
    add("float32_after", 64, 48, rng.uniform(0.0, 1.0, n).astype(np.float32), [("intensity", 7, 12)], [FF("intensity")],
        point_step=16)
    add("float64_feature", 61, 33, rng.uniform(-1e3, 1e3, 61 * 33), [("intensity", 8, 12)], [FF("intensity", 1.0 / 3.0, 1e-3)],
        point_step=21, row_pad=1)
    # an unaligned offset: 13 in a point_step of 29, x y z unaligned too
    add("unaligned_13_of_29", 37, 45, rng.uniform(0.0, 255.0, 37 * 45).astype(np.float32), [("intensity", 7, 13)],
        [FF("intensity", 1.0 / 255.0)], point_step=29, offsets=(1, 5, 9), row_pad=3)
    add("unaligned_u32_17_of_29", 37, 45, _ints(rng, 37 * 45, 0, 2 ** 32 - 1), [("i", 6, 17)], [FF("i", 2.0 ** -32)],
        point_step=29, offsets=(1, 5, 9))
    # big-endian
    add("bigendian_int16", 64, 48, _ints(rng, n, -32768, 32767, (-32768, 32767, 258)), [("i", 3, 12)], [FF("i", 0.25, 1.0)], 3,
        point_step=16, bigendian=True)
    add("bigendian_float32", 50, 31, rng.uniform(0.0, 1.0, 50 * 31).astype(np.float32), [("intensity", 7, 3)], [FF("intensity")],
        point_step=20, offsets=(7, 11, 15), bigendian=True, row_pad=2)
    add("bigendian_f64xyz_float64", 40, 30, rng.uniform(-5.0, 5.0, 1200), [("intensity", 8, 25)], [FF("intensity", 3.0, -0.7)],
        point_step=33, datatype=8, offsets=(1, 9, 17), bigendian=True)
    add("bigendian_uint32", 40, 25, _ints(rng, 1000, 0, 2 ** 32 - 1, (2 ** 32 - 1, 1, 2 ** 24)), [("i", 6, 12)], [FF("i", 1e-6)], 3,
        point_step=16, bigendian=True)
    # FLOAT64 x y z with a UINT16 feature
    add("f64xyz_uint16", 64, 48, _ints(rng, n, 0, 65535, (0, 65535)), [("reflectivity", 4, 24)], [FF("reflectivity", 1.0 / 65535.0)],
        2, point_step=26, datatype=8, offsets=(0, 8, 16))
    # a count = 3 field read at index 2
    add("count3_index2", 64, 48, _ints(rng, n, 0, 65535), [("echo", 4, 12, 3, 2)], [FF("echo", 0.01, index=2)], point_step=18)
    add("count3_float32_index1_bigendian", 31, 17, rng.uniform(0.0, 1.0, 31 * 17).astype(np.float32), [("echo", 7, 12, 3, 1)],
        [FF("echo", index=1)], point_step=24, bigendian=True)
    # the Velodyne driver's layout: point_step 32, intensity FLOAT32 at 16, ring UINT16 at 20
    add("velodyne", 64, 48, rng.uniform(0.0, 255.0, n).astype(np.float32), [("intensity", 7, 16)], [FF("intensity")],
        point_step=32, extra_fields=[("ring", 20, 4, 1)], nan_fraction=0.05)
    # a constant feature: nothing is read (the d435i's own layout: x y z rgb)
    add("constant", 64, 48, np.zeros(n), [("rgb", 7, 16)], [FF.constant(0.3)], point_step=20, row_pad=12)
    # a partial last chunk
    add("one_row_partial_chunk", 1500, 1, rng.uniform(0.0, 1.0, 1500).astype(np.float32), [("intensity", 7, 12)], [FF("intensity")],
        point_step=16)
    # sparsities
    add("finite_0", 100, 7, _ints(rng, 700, 0, 255), [("reflectivity", 2, 12)], [FF("reflectivity", 1.0 / 255.0)],
        xyz=_sparse_xyz(700, 0), point_step=13)
    add("finite_1", 100, 7, rng.uniform(0.0, 1.0, 700).astype(np.float32), [("intensity", 7, 12)], [FF("intensity")],
        xyz=_sparse_xyz(700, 1), point_step=16)
    # float32 values whose handling is easy to get wrong, on finite points: denormals, the largest float32 (scaled by 2 it
    # leaves float32: inf), signed zeros
    sp = rng.uniform(0.0, 1.0, 128)
    sp[:8] = [1e-40, -1e-40, 1.4e-45, F32_MAX, -F32_MAX, 0.0, -0.0, 1.0 + 2.0 ** -23]
    sp = sp.astype(np.float32)
    add("float32_special_identity", 16, 8, sp, [("intensity", 7, 12)], [FF("intensity")], 8, point_step=16)
    add("float32_special_scaled", 16, 8, sp, [("intensity", 7, 12)], [FF("intensity", 2.0, 0.0)], 8, point_step=16)
    add("float32_special_bias", 16, 8, sp, [("intensity", 7, 12)], [FF("intensity", 1.0, -0.0)], 8, point_step=16)
    # NaN / +-inf feature values on finite points: carried through
    nf = rng.uniform(0.0, 1.0, 40 * 25)
    kind = rng.random(1000)
    nf[kind < 0.1] = np.nan
    nf[(kind >= 0.1) & (kind < 0.2)] = np.inf
    nf[(kind >= 0.2) & (kind < 0.3)] = -np.inf
    nf[:3] = [np.nan, np.inf, -np.inf]
    add("nonfinite_feature_f32", 40, 25, nf, [("intensity", 7, 12)], [FF("intensity", 0.5, 1.0)], 3, point_step=16)
    add("nonfinite_feature_f64", 40, 25, nf, [("intensity", 8, 12)], [FF("intensity", -2.0, 0.25)], 3, point_step=20, bigendian=True)
    return cases


def numpy_feature(pp, msg, feat):
    """The issue's numpy expression for one column, over every record of the message."""
    data, width, height, point_step, row_step, fields, big = pp.ingest.as_tuple(msg)
    n = width * height
    if feat.name is None:
        return np.full(n, np.float32(feat.bias), np.float32)
    dt = pp.ingest._parse(data, width, height, point_step, row_step, fields, big)[0]
    rows = np.frombuffer(data, np.uint8)[:height * row_step].reshape(height, row_step)[:, :width * point_step]
    rec = np.ascontiguousarray(rows).reshape(-1).view(dt)
    raw = rec[feat.name]
    raw = raw[:, feat.index] if raw.ndim == 2 else raw
    with np.errstate(all="ignore"):
        return (raw.astype(np.float64) * feat.scale + feat.bias).astype(np.float32)


def host_points(pp, msg, feats, first=1, decimate=4):
    """The yardstick: the package's x y z host chain column-stacked with the numpy feature expression on the same kept
    records.  Returns (points float32 [kept, 3 + nf], finite records)."""
    xyz_all = pp.ingest.pointcloud2_to_xyz(*msg, remove_nans=False)
    fin = np.isfinite(xyz_all).all(axis=1)
    with np.errstate(over="ignore"):
        xyz = pp.ingest.realsense_to_lidar(pp.ingest.pointcloud2_to_xyz(*msg), decimate=decimate, first=first)
    kept = np.flatnonzero(fin)[first::decimate]
    cols = [numpy_feature(pp, msg, f)[kept] for f in feats]
    return np.column_stack([xyz] + cols).astype(np.float32).reshape(len(kept), 3 + len(feats)), int(fin.sum())


def assert_same_points(got, want, what):
    """Bit-identical as uint32, except where the expected value is NaN: there the class is compared."""
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, int((np.isnan(got) != nan).sum()))
    same = (pc2_cases.bits(got) == pc2_cases.bits(want)) | nan
    bad = ~same.all(axis=1) if same.ndim == 2 else ~same
    assert same.all(), (what, int((~same).sum()), got[bad][:3], want[bad][:3])


def lidar_frames(pp, B, n=1500, frame0=0):
    """B `synth.kitti_cloud` arrays [n, 4] scaled into the tiny config's grid (x 0 .. 1.6, y +-0.64, z -3 .. 1), float32,
    no negative zero (an identity mount adds +0, which would turn it into +0)."""
    out = []
    for b in range(B):
        p = pp.synth.kitti_cloud(frame0 + b, n).astype(np.float64)
        p[:, 0] *= 1.6 / 76.0
        p[:, 1] *= 0.64 / 60.0
        p = p.astype(np.float32) + np.float32(0.0)
        assert not np.signbit(p[p == 0]).any()
        out.append(np.ascontiguousarray(p))
    return out


def identity_mount(pp):
    return pp.ingest.Mount(np.eye(3), np.eye(3), 0.0)


def lidar_message(pp, pts, kind="velodyne", seed=977):
    """An [n, 4] array as the message a lidar driver publishes, one row of n records, and the FeatureFields that read the
    intensity back.  velodyne: point_step 32, FLOAT32 intensity at 16, UINT16 ring at 20 -- the intensity comes back bit
    for bit.  reflectivity: point_step 16, UINT8 round(255 * intensity) at 12, read back as raw / 255."""
    FF = pp.ingest.FeatureField
    n = len(pts)
    if kind == "velodyne":
        msg = pp.synth.pointcloud2_from_points(pts, n, 1, feature_fields=[("intensity", 7, 16)], point_step=32,
                                               extra_fields=[("ring", 20, 4, 1)], seed=seed)
        return msg, [FF("intensity")]
    q = np.array(pts, np.float64)
    q[:, 3] = np.round(q[:, 3] * 255.0)
    msg = pp.synth.pointcloud2_from_points(q, n, 1, feature_fields=[("reflectivity", 2, 12)], point_step=16, seed=seed)
    return msg, [FF("reflectivity", 1.0 / 255.0)]
