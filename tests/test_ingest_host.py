"""Host side of the live PointCloud2 ingest: the rule the GPU kernels implement (ingest.select_np +
ingest.transform_ordered64), held bit for bit to the package's host path realsense_to_lidar(pointcloud2_to_xyz(...)),
and the layout / bound helpers with their refusals.  No GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT
import pc2_cases


@pytest.fixture(scope="module")
def cases(pp):
    return pc2_cases.layout_cases(pp)


def test_case_list_covers_what_the_ingest_must_read(pp, cases):
    lay = {k: pp.ingest.layout_of(m) for k, m in cases.items()}
    assert lay["d435i_ps20_padded_rows"]["point_step"] == 20
    assert lay["d435i_ps20_padded_rows"]["row_step"] > 64 * 20
    assert lay["ps32"]["point_step"] == 32
    assert any(v["datatype"] == 8 for v in lay.values()) and any(v["is_bigendian"] for v in lay.values())
    assert any(v["datatype"] == 8 and v["is_bigendian"] for v in lay.values())
    assert any(v["x_offset"] % 4 for v in lay.values())
    finite = {k: pc2_cases.host_ingest(pp, m)[1] for k, m in cases.items()}
    assert finite["all_nan"] == 0 and lay["all_nan"]["width"] * lay["all_nan"]["height"] > 0
    assert [finite[f"finite_{k}"] for k in (0, 1, 2, 5)] == [0, 1, 2, 5]
    xyz = pp.ingest.pointcloud2_to_xyz(*cases["inf_entries"], remove_nans=False)
    assert np.isposinf(xyz).any() and np.isneginf(xyz).any() and np.isnan(xyz).any()


@pytest.mark.parametrize("first,decimate", pc2_cases.SELECTIONS)
def test_rank_rule_and_ordered_transform_equal_the_host_path_bit_for_bit(pp, cases, first, decimate):
    ing = pp.ingest
    for name, msg in cases.items():
        with np.errstate(over="ignore"):
            want, n_finite = pc2_cases.host_ingest(pp, msg, first, decimate)
            xyz = ing.pointcloud2_to_xyz(*msg, remove_nans=False)
            fin = np.isfinite(xyz).all(axis=1)
            keep = ing.select_np(fin, first, decimate)
            got = ing.transform_ordered64(xyz[keep]).astype(np.float32)
            got2, n2 = ing.ingest_np(msg, first, decimate)
        assert int(fin.sum()) == n_finite == n2, name
        assert got.shape == want.shape and want.dtype == np.float32, (name, got.shape, want.shape)
        assert np.array_equal(pc2_cases.bits(got), pc2_cases.bits(want)), name
        assert np.array_equal(pc2_cases.bits(got2), pc2_cases.bits(want)), name
        assert len(keep) <= ing.kept_bound(msg[1], msg[2], first, decimate), name
        # the output row of a kept record is (rank - first) / decimate
        rank = np.cumsum(fin) - fin
        assert np.array_equal((rank[keep] - first) // decimate, np.arange(len(keep))), name


def test_ordered_transform_equals_numpy_dot_in_float64(pp, cases):
    ing = pp.ingest
    for name, msg in cases.items():
        xyz = ing.pointcloud2_to_xyz(*msg)
        a = ing.transform_ordered64(xyz)
        b = ing.realsense_to_lidar64(xyz, decimate=1, first=0)
        assert a.dtype == np.float64 and a.shape == b.shape
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), name
    # a lift other than the sensor height, and matrices handed in
    xyz = ing.pointcloud2_to_xyz(*cases["ps32"])
    assert np.array_equal(ing.transform_ordered64(xyz, lift=0.25, matrices=ing._matrices()),
                          ing.realsense_to_lidar64(xyz, 1, 0, lift=0.25))


def test_layout_of_values(pp, cases):
    ing = pp.ingest
    msg = cases["float64_reordered"]
    lay = ing.layout_of(msg)
    assert lay == {"width": 40, "height": 30, "point_step": 40, "row_step": 40 * 40 + 8, "x_offset": 24, "y_offset": 4,
                   "z_offset": 12, "datatype": 8, "is_bigendian": 0}
    assert tuple(lay) == ing.LAYOUT_KEYS
    assert ing.layout_of(cases["bigendian_f32"])["is_bigendian"] == 1
    assert ing.layout_of(msg[:6]) == lay                      # is_bigendian is optional in the tuple
    # a ROS-like message object: attributes, fields as objects
    data, w, h, ps, rs, fields, be = msg
    ros = types.SimpleNamespace(data=data, width=w, height=h, point_step=ps, row_step=rs, is_bigendian=be,
                                fields=[types.SimpleNamespace(name=n, offset=o, datatype=t, count=c) for n, o, t, c in fields])
    assert ing.layout_of(ros) == lay
    assert np.array_equal(ing.ingest_np(ros)[0], ing.ingest_np(msg)[0])
    # integer fields and mixed field types are described, not judged: the C-ABI refuses them
    ints = (bytes(4 * 12), 4, 1, 12, 48, [("x", 0, 5, 1), ("y", 4, 5, 1), ("z", 8, 5, 1)], False)
    assert ing.layout_of(ints)["datatype"] == 5
    mixed = (bytes(4 * 16), 4, 1, 16, 64, [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 8, 1)], False)
    assert ing.layout_of(mixed)["datatype"] == 7 | 7 << 8 | 8 << 16


def test_layout_of_refuses_what_pointcloud2_to_xyz_refuses(pp):
    ing = pp.ingest
    f = [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1)]
    good = (bytes(2 * 3 * 12), 3, 2, 12, 36, f, False)
    assert ing.layout_of(good)["width"] == 3
    bad = {
        "without x/y/z": (good[0], 3, 2, 12, 36, f[:2], False),
        "unknown datatype": (good[0], 3, 2, 12, 36, f[:2] + [("z", 8, 9, 1)], False),
        "does not fit point_step": (good[0], 3, 2, 12, 36, f[:2] + [("z", 9, 7, 1)], False),
        "row_step 35 < width 3 x point_step 12": (good[0], 3, 2, 12, 35, f, False),
        "data holds 71 bytes": (good[0][:-1], 3, 2, 12, 36, f, False),
    }
    for text, msg in bad.items():
        with pytest.raises(ValueError, match=re.escape(text)) as a:
            ing.layout_of(msg)
        with pytest.raises(ValueError, match=re.escape(text)) as b:
            ing.pointcloud2_to_xyz(*msg)
        assert str(a.value) == str(b.value)
    with pytest.raises(ValueError, match="6 or 7 entries"):
        ing.layout_of(good[:5])


def test_kept_bound_and_select_np(pp):
    ing = pp.ingest
    assert ing.kept_bound(640, 480) == 76800 == len(range(640 * 480)[1::4])
    for n in (0, 1, 2, 3, 4, 5, 9, 100):
        for first, dec in pc2_cases.SELECTIONS + [(7, 2), (0, 3)]:
            assert ing.kept_bound(n, 1, first, dec) == len(range(n)[first::dec]), (n, first, dec)
            fin = np.ones(n, bool)
            assert np.array_equal(ing.select_np(fin, first, dec), np.arange(n)[first::dec])
    assert ing.kept_bound(0, 480) == 0 and ing.kept_bound(1, 1, 1, 4) == 0
    fin = np.array([0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1], bool)
    assert ing.select_np(fin, 1, 2).tolist() == np.flatnonzero(fin)[1::2].tolist() == [2, 6, 9]
    for fn in (lambda: ing.kept_bound(4, 4, 1, 0), lambda: ing.select_np(fin, 1, 0)):
        with pytest.raises(ValueError, match="decimate 0 < 1"):
            fn()
    for fn in (lambda: ing.kept_bound(4, 4, -1, 4), lambda: ing.select_np(fin, -1, 4)):
        with pytest.raises(ValueError, match="first -1 < 0"):
            fn()


def test_new_structs_match_the_header(pp):
    assert ctypes.sizeof(pp._lib.PPPc2Layout) == 10 * 4
    assert ctypes.sizeof(pp._lib.PPIngestConfig) == 2 * 4 + (9 + 9 + 3) * 8
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    lay = hdr.split("typedef struct pp_pc2_layout {", 1)[1].split("} pp_pc2_layout;", 1)[0]
    lay = re.sub(r"/\*.*?\*/", "", lay, flags=re.S)
    names = [n.strip() for decl in re.findall(r"int32_t\s+([^;]+);", lay) for n in decl.split(",")]
    assert names == [n for n, _ in pp._lib.PPPc2Layout._fields_]
    assert names[:-1] == list(pp.ingest.LAYOUT_KEYS)
    cfg = hdr.split("typedef struct pp_ingest_config {", 1)[1].split("} pp_ingest_config;", 1)[0]
    cfg = re.sub(r"/\*.*?\*/", "", cfg, flags=re.S)
    assert re.findall(r"(\w+)(?:\[(\d+)\])?\s*[,;]", cfg) == [("first", ""), ("decimate", ""), ("r", "9"), ("r2", "9"), ("lift", "3")]
    assert [n for n, _ in pp._lib.PPIngestConfig._fields_] == ["first", "decimate", "r", "r2", "lift"]
    assert "pp_ingest_pointcloud2" in pp._lib.EXPORTS and "ingest.hip" in pp._lib.SOURCES


def test_engine_packs_messages_as_the_cabi_takes_them(pp, cases):
    from pp_amd import engine
    names = ["d435i_ps20_padded_rows", "no_records", "bigendian_f64_unaligned"]
    tuples = [pp.ingest.as_tuple(cases[n]) for n in names]
    offs, layouts, bufs = engine._pack_messages(tuples)
    assert offs.dtype == np.int64 and offs[0] == 0
    for b, t in enumerate(tuples):
        assert offs[b + 1] - offs[b] == t[2] * t[4] == bufs[b].size
        assert layouts[b].row_step == t[4] and layouts[b].is_bigendian == int(t[6]) and layouts[b].reserved == 0
    cfg = engine._ingest_config(1, 4, 1.0)
    r, r2 = pp.ingest._matrices()
    assert np.array_equal(np.array(cfg.r[:]).reshape(3, 3), r) and np.array_equal(np.array(cfg.r2[:]).reshape(3, 3), r2)
    assert cfg.lift[:] == [0.0, 0.0, 1.0] and (cfg.first, cfg.decimate) == (1, 4)
