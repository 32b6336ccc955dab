"""sweeps.py, the host restatement of the multi-sweep accumulation (the GPU stage is held to it bit for bit in
tests/test_gpu_sweeps.py).  The reference has no such path, so the restatement is held to hand-made cases with known
coordinates and to an independent homogeneous-matrix formulation written here."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I34 = np.hstack([np.eye(3), np.zeros((3, 1))])


@pytest.fixture(scope="module")
def S(pp):
    return pp.sweeps


def _frame(n, F, seed):
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((n, F)) * 3.0).astype(np.float32)
    if F > 3:
        f[:, 3:] = rng.random((n, F - 3), dtype=np.float32)
    return f


def _acc(S, F=4, nmax=512, streams=1, **kw):
    base = dict(history=2, max_age=10.0)
    base.update(kw)
    return S.SweepAccumulator(S.SweepConfig(**base), streams, F, nmax)


# ---- hand cases ----
def test_identity_pose_copies_the_history(S):
    a = _acc(S, F=4)
    f0, f1, f2 = (_frame(n, 4, i) for i, n in enumerate((5, 7, 3)))
    out, info = a.accumulate([f0], [I34], [1.0])
    assert out[0].tobytes() == f0.tobytes() and info["count"].tolist() == [5] and info["used"].tolist() == [0]
    out, info = a.accumulate([f1], [I34], [2.0])
    assert out[0].tobytes() == np.concatenate([f1, f0]).tobytes() and info["used"].tolist() == [1]
    out, info = a.accumulate([f2], [I34], [3.0])
    assert out[0].tobytes() == np.concatenate([f2, f1, f0]).tobytes()            # newest first
    assert info["count"].tolist() == [15] and info["used"].tolist() == [2] and info["truncated"].tolist() == [0]
    f3 = _frame(2, 4, 9)
    out, info = a.accumulate([f3], [I34], [4.0])                                 # history 2: f0 has left the ring
    assert out[0].tobytes() == np.concatenate([f3, f2, f1]).tobytes()


def test_translation_and_quarter_turn_have_known_coordinates(S):
    a = _acc(S, F=3)
    p = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 0.0]], np.float32)
    a.accumulate([p], [S.pose_from_xyyaw(10.0, 20.0, 0.0)], [0.0])
    # the sensor has moved on by (+1, -2): a stored point appears at p - (1, -2, 0)
    out, _ = a.accumulate([np.zeros((0, 3), np.float32)], [S.pose_from_xyyaw(11.0, 18.0, 0.0)], [1.0])
    assert out[0].tolist() == [[0.0, 4.0, 3.0], [-5.0, 2.5, 0.0]]
    # a quarter turn to the left on the spot, exact entries: what lay ahead (+x) now lies to the right (-y)
    b = _acc(S, F=3)
    b.accumulate([p], [I34], [0.0])
    turn = np.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    out, _ = b.accumulate([np.zeros((0, 3), np.float32)], [turn], [1.0])
    assert out[0].tolist() == [[2.0, -1.0, 3.0], [0.5, 4.0, 0.0]]
    M, u = S.relative_transform(turn, I34)
    assert M.tolist() == [[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]] and u.tolist() == [0.0, 0.0, 0.0]


def test_equals_a_homogeneous_matrix_formulation(S):
    rng = np.random.default_rng(3)
    a = _acc(S, F=4, time_feature=3)
    poses = [S.pose_from_xyyaw(*rng.normal(size=3)) for _ in range(3)]
    frames = [_frame(40, 4, 10 + i) for i in range(3)]
    for i in range(3):
        out, _ = a.accumulate([frames[i]], [poses[i]], [0.5 * i])
    T = [np.vstack([p, [0, 0, 0, 1.0]]) for p in poses]
    want = [frames[2][:, :3].astype(np.float64)]
    for j in (1, 0):
        rel = np.linalg.inv(T[2]) @ T[j]
        want.append(frames[j][:, :3].astype(np.float64) @ rel[:3, :3].T + rel[:3, 3])
    # (another summation order and a LAPACK inverse: agreement to float32 rounding, not bit for bit)
    np.testing.assert_allclose(out[0][:, :3], np.concatenate(want), rtol=0, atol=1e-5)
    assert out[0][:40, 3].tolist() == [0.0] * 40
    assert out[0][40:80, 3].tolist() == [0.5] * 40 and out[0][80:, 3].tolist() == [1.0] * 40
    assert S.pose_from_matrix(T[1]).tobytes() == poses[1].tobytes()
    with pytest.raises(ValueError, match="last row"):
        S.pose_from_matrix(np.ones((4, 4)))


def test_max_age_drops_the_oldest_sweep(S):
    a = _acc(S, F=3, max_age=1.5)
    f = [_frame(4, 3, i) for i in range(3)]
    a.accumulate([f[0]], [I34], [0.0])
    a.accumulate([f[1]], [I34], [1.0])
    out, info = a.accumulate([f[2]], [I34], [2.0])                  # ages 1.0 and 2.0: the second is too old
    assert out[0].tobytes() == np.concatenate([f[2], f[1]]).tobytes() and info["used"].tolist() == [1]
    b = _acc(S, F=3, max_age=1.0)                                   # the bound is inclusive
    b.accumulate([f[0]], [I34], [0.0])
    assert b.accumulate([f[1]], [I34], [1.0])[1]["used"].tolist() == [1]


def test_truncation_inside_a_sweep_and_at_a_boundary(S):
    f = [_frame(6, 3, i) for i in range(3)]
    a = _acc(S, F=3, nmax=15)
    a.accumulate([f[0]], [I34], [0.0])
    a.accumulate([f[1]], [I34], [1.0])
    out, info = a.accumulate([f[2]], [I34], [2.0])                  # 18 rows into 15: the cut falls inside the older sweep
    assert out[0].tobytes() == np.concatenate([f[2], f[1], f[0][:3]]).tobytes()
    assert info["count"].tolist() == [15] and info["truncated"].tolist() == [3] and info["used"].tolist() == [2]
    b = _acc(S, F=3, nmax=12)
    b.accumulate([f[0]], [I34], [0.0])
    b.accumulate([f[1]], [I34], [1.0])
    out, info = b.accumulate([f[2]], [I34], [2.0])                  # exactly at the boundary between the two sweeps
    assert out[0].tobytes() == np.concatenate([f[2], f[1]]).tobytes()
    assert info["count"].tolist() == [12] and info["truncated"].tolist() == [6] and info["used"].tolist() == [2]


def test_history_decimate_and_capacity_cut(S):
    f0, f1 = _frame(10, 3, 0), _frame(2, 3, 1)
    a = _acc(S, F=3, history_decimate=3)
    _, info = a.accumulate([f0], [I34], [0.0])
    assert info["push_truncated"].tolist() == [0]
    out, _ = a.accumulate([f1], [I34], [1.0])
    assert out[0].tobytes() == np.concatenate([f1, f0[[0, 3, 6, 9]]]).tobytes()
    b = _acc(S, F=3, history_decimate=3, capacity=3)
    _, info = b.accumulate([f0], [I34], [0.0])
    assert info["push_truncated"].tolist() == [1]
    out, _ = b.accumulate([f1], [I34], [1.0])
    assert out[0].tobytes() == np.concatenate([f1, f0[[0, 3, 6]]]).tobytes()
    assert b.cfg.capacity == 3 and a.cfg.capacity == 512            # None: max_points_per_frame


def test_reset_of_one_stream_and_shorter_calls(S):
    a = _acc(S, F=3, streams=2)
    f = [_frame(3, 3, i) for i in range(6)]
    a.accumulate([f[0], f[1]], [I34, I34], [0.0, 0.0])
    a.reset(0)
    out, info = a.accumulate([f[2], f[3]], [I34, I34], [0.0, 1.0])  # stream 0 starts over (its stamp may repeat)
    assert out[0].tobytes() == f[2].tobytes() and out[1].tobytes() == np.concatenate([f[3], f[1]]).tobytes()
    assert info["used"].tolist() == [0, 1]
    out, _ = a.accumulate([f[4]], [I34], [1.0])                     # one frame: stream 1 is not touched
    assert out[0].tobytes() == np.concatenate([f[4], f[2]]).tobytes()
    out, _ = a.accumulate([f[5], f[5]], [I34, I34], [2.0, 2.0])
    assert out[1].tobytes() == np.concatenate([f[5], f[3], f[1]]).tobytes()


def test_time_feature_values(S):
    a = _acc(S, F=5, time_feature=4)
    f0, f1 = _frame(3, 5, 0), _frame(2, 5, 1)
    a.accumulate([f0], [I34], [10.0])
    out, _ = a.accumulate([f1], [I34], [10.1])
    lag = np.float32(10.1 - 10.0)
    assert out[0][:, 4].tolist() == [0.0, 0.0] + [float(lag)] * 3
    assert out[0][:, :4].tobytes() == np.concatenate([f1, f0])[:, :4].tobytes()   # the other columns bitwise
    b = _acc(S, F=5)                                                              # -1: nothing is overwritten
    b.accumulate([f0], [I34], [10.0])
    assert b.accumulate([f1], [I34], [10.1])[0][0].tobytes() == np.concatenate([f1, f0]).tobytes()
    # the stored frame is the ORIGINAL one: its own time column comes back as the lag, not as 0
    out, _ = a.accumulate([f1], [I34], [10.2])
    assert out[0][2:4, :4].tobytes() == f1[:, :4].tobytes()


def test_accumulate_np_is_the_accumulator(S):
    f = [_frame(5, 3, i) for i in range(3)]
    calls = [([f[i]], [S.pose_from_xyyaw(0.1 * i, 0.0, 0.05 * i)], [0.1 * i]) for i in range(3)]
    got = S.accumulate_np({"history": 2, "max_age": 1.0}, calls, 3, 512)
    a = _acc(S, F=3, max_age=1.0)
    for c, (out, info) in zip(calls, got):
        want, winfo = a.accumulate(*c)
        assert out[0].tobytes() == want[0].tobytes() and all(np.array_equal(info[k], winfo[k]) for k in info)


# ---- refusals ----
def test_refusals_name_the_stream_or_field(pp, S):
    a = _acc(S, F=3, streams=2)
    f = _frame(3, 3, 0)
    a.accumulate([f, f], [I34, I34], [1.0, 1.0])
    with pytest.raises(ValueError, match="stream 1 does not increase"):
        a.accumulate([f, f], [I34, I34], [2.0, 1.0])
    out, _ = a.accumulate([f, f], [I34, I34], [2.0, 2.0])           # the refused call left no trace
    assert out[0].shape[0] == 6
    bad = I34.copy()
    bad[0, 0] = 1.001
    with pytest.raises(ValueError, match="stream 0 is not orthonormal"):
        a.accumulate([f, f], [bad, I34], [3.0, 3.0])
    nearly = I34.copy()
    nearly[0, 0] = 1.0 + 1e-7                                       # inside the 1e-6 bound
    S.check_call([nearly], [0.0], 1, [np.nan])
    with pytest.raises(ValueError, match="stream 1 is not finite"):
        a.accumulate([f, f], [I34, I34 * np.nan], [3.0, 3.0])
    with pytest.raises(ValueError, match="stamp of stream 0 is not finite"):
        a.accumulate([f, f], [I34, I34], [np.inf, 3.0])
    with pytest.raises(ValueError, match="time_feature"):
        S.SweepAccumulator(S.SweepConfig(time_feature=3), 1, 3, 512)
    with pytest.raises(ValueError, match="time_feature"):
        S.SweepConfig(time_feature=1)
    with pytest.raises(ValueError, match="hystory"):
        S.SweepConfig.from_any({"hystory": 2})
    for field, value in (("history", 0), ("history", 9), ("capacity", 0), ("history_decimate", 0), ("max_age", 0.0),
                         ("max_age", float("nan")), ("history", 1.5)):
        with pytest.raises(ValueError, match=field):
            S.SweepConfig(**{field: value})


# ---- structure ----
NEW = ["pp_set_sweeps", "pp_get_sweeps", "pp_sweeps_accumulate", "pp_sweeps_accumulate_async", "pp_sweeps_info",
       "pp_sweeps_reset"]


def test_struct_size_header_exports_and_sources(pp, S):
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    body = re.search(r"typedef struct pp_sweep_config \{(.*?)\} pp_sweep_config;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(double|int32_t)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in pp._lib.PPSweepConfig._fields_]
    assert sum(8 if t == "double" else 4 for t, _ in fields) == ctypes.sizeof(pp._lib.PPSweepConfig) == 24
    csrc = os.path.join(os.path.dirname(pp._lib.__file__), "csrc")
    assert "static_assert(sizeof(pp_sweep_config) == 24" in open(os.path.join(csrc, "api_sweeps.hip")).read()
    assert re.search(r"#define PP_SWEEP_MAX 8\b", hdr) and pp._lib.PP_SWEEP_MAX == S.PP_SWEEP_MAX == 8
    assert "#define PP_ABI_VERSION 4" in hdr
    later = hdr[hdr.index("later additions within 4"):hdr.index("#define PP_ABI_VERSION")]
    for name in ["PP_SWEEP_MAX", "pp_sweep_config"] + NEW:
        assert re.search(r"\b%s\b" % name, later), name
        if name.startswith("pp_s") and name != "pp_sweep_config":
            assert name in pp._lib.EXPORTS
    src = pp._lib.SOURCES
    assert "api_sweeps.hip" in src and "sweeps.hip" in src
    for s in ("api_sweeps.hip", "sweeps.hip"):
        assert os.path.exists(os.path.join(csrc, s))
    assert "sweeps" in pp.__all__
    for name in ("SweepConfig", "SweepAccumulator", "accumulate_np", "pose_from_xyyaw", "pose_from_matrix"):
        assert hasattr(S, name)
    for name in ("set_sweeps", "sweeps", "accumulate_sweeps", "accumulate_sweeps_async", "sweeps_info", "sweeps_reset"):
        assert callable(getattr(pp.Engine, name))


def test_exported_from_the_library(hip_lib):
    for name in NEW:
        assert hasattr(hip_lib, name), name


def test_config_key_round_trips(pp, S):
    cfg = pp.config.tiny_config(1)
    assert pp.config.Derived(cfg).sweeps is None
    cfg["model"]["second"]["sweeps"] = False
    assert pp.config.Derived(cfg).sweeps is None
    cfg["model"]["second"]["sweeps"] = True
    assert pp.config.Derived(cfg).sweeps == S.SweepConfig().to_dict()
    cfg["model"]["second"]["sweeps"] = {"history": 3, "history_decimate": 2}
    d = pp.config.Derived(cfg)
    assert d.sweeps == dict(S.SweepConfig().to_dict(), history=3, history_decimate=2)
    assert S.SweepConfig.from_any(d.sweeps).to_dict() == d.sweeps
    assert "sweeps" not in d.nms_dict() and "sweeps" not in d.model_dict()
    cfg["model"]["second"]["sweeps"] = {"time_feature": 3}          # tiny_config has 3 point features
    with pytest.raises(ValueError, match="model.second.sweeps.*time_feature"):
        pp.config.Derived(cfg)
    cfg["model"]["second"]["sweeps"] = {"histori": 3}
    with pytest.raises(ValueError, match="histori"):
        pp.config.Derived(cfg)
    cfg["model"]["second"]["sweeps"] = 3
    with pytest.raises(ValueError, match="sweeps"):
        pp.config.Derived(cfg)
