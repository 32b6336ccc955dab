"""Synthetic sensor_msgs/PointCloud2 messages shared by test_ingest_host.py and test_gpu_ingest.py: every layout the
live ingest has to read, and the (first, decimate) pairs it is checked at."""
import numpy as np

SELECTIONS = [(0, 1), (1, 4), (3, 7)]


def _sparse(pp, n_finite, n=700, **kw):
    """n records of which exactly n_finite are finite, spread over the message."""
    rng = np.random.default_rng(100 + n_finite)
    xyz = np.full((n, 3), np.nan)
    rows = np.sort(rng.choice(n, n_finite, replace=False))
    xyz[rows] = rng.uniform(-3.0, 6.0, (n_finite, 3))
    return pp.synth.pointcloud2_from_xyz(xyz, n // 7, 7, seed=200 + n_finite, **kw)


def layout_cases(pp):
    """name -> message tuple (data, width, height, point_step, row_step, fields, is_bigendian)."""
    s = pp.synth
    rng = np.random.default_rng(5)
    cases = {
        "d435i_ps20_padded_rows": s.pointcloud2_message(1, 64, 48, point_step=20, row_pad=12),
        "ps32": s.pointcloud2_message(2, 64, 48, point_step=32),
        "ps32_padded_rows_odd": s.pointcloud2_message(3, 50, 31, point_step=32, row_pad=5),
        "float64": s.pointcloud2_message(4, 64, 48, point_step=32, datatype=8, offsets=(0, 8, 16)),
        "float64_reordered": s.pointcloud2_message(5, 40, 30, point_step=40, datatype=8, offsets=(24, 4, 12), row_pad=8),
        "bigendian_f32": s.pointcloud2_message(6, 64, 48, point_step=16, bigendian=True),
        "bigendian_f64_unaligned": s.pointcloud2_message(7, 37, 45, point_step=29, row_pad=3, datatype=8, bigendian=True,
                                                         offsets=(1, 9, 17)),
        "unaligned_f32": s.pointcloud2_message(8, 61, 33, point_step=21, offsets=(9, 1, 5), row_pad=1),
        "one_row_partial_chunk": s.pointcloud2_message(9, 1500, 1, point_step=20),
        "all_nan": s.pointcloud2_message(10, 32, 24, nan_fraction=1.1),
        "no_nan": s.pointcloud2_message(11, 48, 40, point_step=12, nan_fraction=0.0),
        "finite_0": _sparse(pp, 0),
        "finite_1": _sparse(pp, 1),
        "finite_2": _sparse(pp, 2, point_step=32),
        "finite_5": _sparse(pp, 5, datatype=8, point_step=24, offsets=(0, 8, 16)),
        "no_records": s.pointcloud2_from_xyz(np.zeros((0, 3)), 0, 0),
        # one record short of a chunk of 512, exactly one, one more (511 x 1, 64 x 8, 27 x 19 = 513)
        "chunk_minus_1": s.pointcloud2_message(12, 511, 1, point_step=20),
        "chunk_exact": s.pointcloud2_message(13, 64, 8, point_step=20),
        "chunk_plus_1": s.pointcloud2_message(14, 27, 19, point_step=20),
    }
    # +-inf entries beside NaN ones: a record with an infinite coordinate is dropped like a NaN one
    xyz = rng.uniform(-3.0, 6.0, (40 * 25, 3))
    bad = rng.random(len(xyz))
    xyz[bad < 0.1, 0] = np.inf
    xyz[(bad >= 0.1) & (bad < 0.2), 2] = -np.inf
    xyz[(bad >= 0.2) & (bad < 0.3), 1] = np.nan
    cases["inf_entries"] = s.pointcloud2_from_xyz(xyz, 40, 25, point_step=20, seed=31)
    # values whose rounding is easy to get wrong: signed zeros, float32 denormals, the largest float32, tiny and huge mixes
    sp = rng.uniform(-3.0, 6.0, (16 * 8, 3))
    sp[0] = [0.0, 0.0, 0.0]
    sp[1] = [-0.0, -0.0, -0.0]
    sp[2] = [1e-40, -1e-40, 3e-45]
    sp[3] = [3.4028234e38, -3.4028234e38, 1.0]
    sp[4] = [1e-30, 1.0, 1e30]
    sp[5] = [16777217.0, 1.0 + 2.0 ** -23, -1.0]
    cases["special_values_f32"] = s.pointcloud2_from_xyz(sp, 16, 8, point_step=20, seed=32)
    sp64 = sp.copy()
    sp64[2] = [1e-310, -1e-310, 5e-324]
    sp64[3] = [1e300, -1e300, 1.0]
    sp64[6] = [1.0 + 2.0 ** -40, 0.1, 1.0 / 3.0]
    cases["special_values_f64"] = s.pointcloud2_from_xyz(sp64, 16, 8, point_step=24, datatype=8, offsets=(0, 8, 16), seed=33)
    return cases


def host_ingest(pp, msg, first=1, decimate=4):
    """The yardstick: the package's host path, (points float32 [n, 3], finite records)."""
    xyz = pp.ingest.pointcloud2_to_xyz(*msg)
    return pp.ingest.realsense_to_lidar(xyz, decimate=decimate, first=first), len(xyz)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
