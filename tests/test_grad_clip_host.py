"""Gradient clipping, host side: the restated TensorFlow rules (optim.clip_gradients_np, the GPU tests' reference) on
hand-computed cases, GradClip's validation and configuration key, the C-ABI additions and what they refuse before
anything is launched."""
import ctypes
import re

import numpy as np
import pytest

F = np.float32


def _clip(pp, g, mode, c, **kw):
    return pp.optim.clip_gradients_np(np.asarray(g, F), None, None, pp.optim.GradClip(mode, c, **kw))


def test_3_4_0_tensor(pp):
    g = [3.0, 4.0, 0.0]
    # norm 5, c = 1: (g * 1) / max(5, 1); global: scale = 1 * min(1 / 5, 1 / 1)
    out, st = _clip(pp, g, "norm", 1.0)
    assert st["global_norm"] == 5.0 and st["norms"].tolist() == [5.0] and not st["nonfinite"] and not st["skipped"]
    assert out.dtype == F and np.array_equal(out, np.asarray([F(3) / F(5), F(4) / F(5), 0], F))
    assert st["scales"][0] == F(1) / F(5)
    out, st = _clip(pp, g, "global_norm", 1.0)
    s = F(1) / F(5)
    assert st["scale"] == float(s) and np.array_equal(out, np.asarray([F(3) * s, F(4) * s, 0], F))
    # c = 10: under the bar.  norm: (g * 10) / 10 is g again; global: 10 * min(0.2, 0.1f) rounds to exactly 1
    out, st = _clip(pp, g, "norm", 10.0)
    assert np.array_equal(out, np.asarray(g, F)) and st["scales"][0] == 1.0
    out, st = _clip(pp, g, "global_norm", 10.0)
    assert st["scale"] == float(F(10) * (F(1) / F(10))) == 1.0 and np.array_equal(out, np.asarray(g, F))
    out, st = _clip(pp, g, "value", 3.5)
    assert np.array_equal(out, np.asarray([3.0, 3.5, 0.0], F))
    out, st = _clip(pp, g, None, None)
    assert np.array_equal(out, np.asarray(g, F)) and st["global_norm"] == 5.0 and st["scale"] == 1.0


def test_all_zero_tensor(pp):
    z = np.zeros(5, F)
    out, st = _clip(pp, z, "norm", 0.3)               # (0 * c) / max(0, c)
    assert np.array_equal(out, z) and st["norms"][0] == 0.0 and st["scales"][0] == 1.0
    out, st = _clip(pp, z, "global_norm", 0.3)        # 1 / 0 = inf, so scale = c * (1 / c)
    assert st["scale"] == float(F(0.3) * (F(1) / F(0.3))) and np.array_equal(out, z)
    assert not st["nonfinite"]


def test_value_keeps_a_nan_and_the_flag_sees_it(pp):
    g = np.asarray([-2.0, np.nan, 0.25, np.inf, -np.inf], F)
    out, st = _clip(pp, g, "value", 0.5, skip_nonfinite=True)
    assert np.array_equal(out[[0, 2, 3, 4]], np.asarray([-0.5, 0.25, 0.5, -0.5], F)) and np.isnan(out[1])
    assert st["nonfinite"] and st["skipped"]
    _, st = _clip(pp, g, "global_norm", 0.5)
    assert st["nonfinite"] and not st["skipped"] and np.isnan(st["scale"])
    out, st = _clip(pp, np.asarray([1.0, np.nan], F), "norm", 0.5)       # a NaN norm stays one
    assert np.isnan(out).all() and np.isnan(st["scales"][0])


def test_guard_skips_a_norm_beyond_float32(pp):
    g = np.full(4, 3e38, F)              # the float64 sum is finite, the float32 norm is not
    _, st = _clip(pp, g, "global_norm", 1.0, skip_nonfinite=True)
    assert not st["nonfinite"] and st["skipped"] and np.isinf(st["global_norm"]) and np.isnan(st["scale"])
    _, st = _clip(pp, g, "global_norm", 1.0)
    assert not st["nonfinite"] and not st["skipped"]


def test_groups_and_segments(pp):
    flat = np.asarray([np.nan, 3, 4, np.nan, 0.3, np.nan, 0.4, 7], F)       # entries 0, 3, 5, 7 are outside
    segs, groups = [(1, 2), (4, 1), (6, 1), (7, 0)], [0, 1, 1, 2]
    out, st = pp.optim.clip_gradients_np(flat, segs, groups, pp.optim.GradClip("norm", 1.0))
    n1 = F(np.sqrt(np.float64(F(0.3)) ** 2 + np.float64(F(0.4)) ** 2))
    assert st["norms"].tolist() == [5.0, float(n1), 0.0] and not st["nonfinite"]
    assert st["global_norm"] == float(F(np.sqrt(25.0 + np.float64(F(0.3)) ** 2 + np.float64(F(0.4)) ** 2)))
    assert np.array_equal(out[1:3], np.asarray([F(3) / F(5), F(4) / F(5)], F))
    assert out[4] == F(0.3) and out[6] == F(0.4) and out[7] == 7          # (x * 1) / 1; the empty segment
    assert np.isnan(out[[0, 3, 5]]).all()


def test_gradclip_validation(pp):
    G = pp.optim.GradClip
    assert G().mode is None and not G().skip_nonfinite and G().needs_norm
    assert not G("value", 0.1).needs_norm and G("value", 0.1, skip_nonfinite=True).needs_norm
    assert G("norm", 1).clip == 1.0 and G("global_norm", np.float32(2)).clip == 2.0
    for bad in (("l2", 1.0), ("Value", 1.0), (3, 1.0)):
        with pytest.raises(ValueError):
            G(*bad)
    for mode in ("value", "norm", "global_norm"):
        for clip in (0, -1.0, float("nan"), float("inf"), None, "1"):
            with pytest.raises(ValueError):
                G(mode, clip)


def test_from_config(pp):
    G = pp.optim.GradClip
    assert G.from_config({}) is None and G.from_config({"optimizer": {}}) is None and G.from_config(None) is None
    c = G.from_config({"gradient_clipping": {"mode": "global_norm", "clip": 5, "skip_nonfinite": True}})
    assert (c.mode, c.clip, c.skip_nonfinite) == ("global_norm", 5.0, True)
    c = G.from_config({"gradient_clipping": {"skip_nonfinite": True}})
    assert (c.mode, c.clip, c.skip_nonfinite) == (None, None, True)
    assert G.from_config({"gradient_clipping": {"mode": "none"}}).mode is None
    for bad in ({"mode": "norm"}, {"mode": "norm", "clip": 0}, {"mode": "nope", "clip": 1}, {"mode": "value", "clip": 1, "x": 2}, 3):
        with pytest.raises(ValueError):
            G.from_config({"gradient_clipping": bad})
    # the shipped configuration carries no such key: nothing turns clipping on by itself
    cfg = pp.config.pedestrian_d435i_config(2)
    assert G.from_config(cfg.get("train_config") or {}) is None


def test_abi_symbols_and_sources(pp, hip_lib):
    from pp_amd import _lib
    assert "grad_clip.hip" in _lib.SOURCES
    for name in ("pp_grad_clip_workspace_bytes", "pp_grad_norm_device", "pp_adamw_step_clipped_device"):
        assert name in _lib.EXPORTS and hasattr(hip_lib, name)
    assert (_lib.PP_CLIP_NONE, _lib.PP_CLIP_VALUE, _lib.PP_CLIP_NORM, _lib.PP_CLIP_GLOBAL_NORM) == (0, 1, 2, 3)
    assert ctypes.sizeof(_lib.PPGradClipConfig) == 12
    with open(_lib._INCLUDE) as f:
        head = f.read()
    later = head[head.index("later additions within 4"):head.index("#define PP_ABI_VERSION")]
    for name in ("pp_grad_clip_mode", "pp_grad_clip_config", "pp_grad_clip_workspace_bytes", "pp_grad_norm_device",
                 "pp_adamw_step_clipped_device"):
        assert name in later and len(re.findall(r"\b%s\b" % name, head)) >= 2, name
    assert hip_lib.pp_abi_version() == 4
    def wb(n, nseg, ngroups):
        out = ctypes.c_int64(-1)
        st = hip_lib.pp_grad_clip_workspace_bytes(n, nseg, ngroups, ctypes.byref(out))
        assert (st == 0) == (out.value >= 0) and st in (0, 1)
        return out.value
    assert hip_lib.pp_grad_clip_workspace_bytes(4, 1, 1, None) == 1
    assert wb(0, 0, 1) >= 24 and wb(1 << 20, 70, 10) > wb(1 << 20, 70, 1) > 0
    assert wb(1 << 33, 1, 1) > wb(1 << 20, 1, 1)          # 64-bit sizes
    assert wb(-1, 0, 1) == -1 and wb(4, -1, 1) == -1 and wb(4, 1, 0) == -1


def test_argument_errors_are_refused_before_any_launch(pp, hip_lib):
    """Everything the kernels index with is checked on the host: PP_ERR_ARG, pp_last_error names the reason.  The
    pointers are never followed (no device is touched)."""
    from pp_amd import _lib
    n = 4096
    buf = ctypes.c_void_p(0x1000)       # never dereferenced: every call below is refused first
    ws = ctypes.c_void_p(0x2000)

    def step(segs, groups, n_groups, mode, clip, skip=0, workspace=ws):
        seg = np.ascontiguousarray(segs, np.int64).reshape(-1, 2)
        grp = None if groups is None else np.ascontiguousarray(groups, np.int32)
        cfg = _lib.PPGradClipConfig(mode, clip, skip)
        return hip_lib.pp_adamw_step_clipped_device(
            0, None, buf, buf, buf, buf, n, seg.ctypes.data_as(ctypes.c_void_p), len(seg),
            grp.ctypes.data_as(ctypes.c_void_p) if grp is not None else None, n_groups, ctypes.byref(cfg), workspace,
            1e-3, 0.9, 0.999, 1e-8, 1e-4)

    def norm(segs, groups, n_groups, workspace=ws, n=n):
        seg = np.ascontiguousarray(segs, np.int64).reshape(-1, 2)
        grp = None if groups is None else np.ascontiguousarray(groups, np.int32)
        return hip_lib.pp_grad_norm_device(0, None, buf, n, seg.ctypes.data_as(ctypes.c_void_p), len(seg),
                                           grp.ctypes.data_as(ctypes.c_void_p) if grp is not None else None, n_groups,
                                           workspace)
    ok = [(0, 100), (200, 50)]
    for mode in (1, 2, 3):
        for clip in (0.0, -1.0, float("nan"), float("inf")):
            assert step(ok, None, 1, mode, clip) == 1, (mode, clip)
    assert step(ok, None, 1, 4, 1.0) == 1 and step(ok, None, 1, -1, 1.0) == 1            # unknown mode
    for segs in ([(-1, 10)], [(0, n + 1)], [(n, 1)], [(10, -1)], [(1 << 62, 1 << 62)]):
        assert step(segs, None, 1, 3, 1.0) == 1, segs
        assert step(segs, None, 1, 1, 1.0) == 1, segs                                   # also where no reduction runs
        assert norm(segs, None, 1) == 1, segs
    for groups, n_groups in (([0, 2], 2), ([-1, 0], 2), ([0, 1], 1), (None, 2), ([0, 0], 0)):
        assert step(ok, groups, n_groups, 2, 1.0) == 1, (groups, n_groups)
        assert norm(ok, groups, n_groups) == 1, (groups, n_groups)
    assert step(ok, None, 1, 3, 1.0, workspace=None) == 1                               # a reduction needs a workspace
    assert step(ok, None, 1, 0, 0.0, workspace=None) == 1                               # ... monitor mode, too
    assert step(ok, None, 1, 1, 1.0, skip=1, workspace=None) == 1                       # ... and the guard
    assert norm(ok, None, 1, workspace=None) == 1
    assert norm(ok, None, 1, workspace=ctypes.c_void_p(0x2004)) == 1                    # misaligned
    assert norm([(0, 1 << 20)] * 3, None, 1, n=1 << 20) == 1                            # overlapping segments
    assert b"overlap" in hip_lib.pp_last_error(None)
