"""Gradient clipping and the non-finite step guard on the GPU (csrc/grad_clip.hip, pp_grad_norm_device,
pp_adamw_step_clipped_device, optim.GradClip, Trainer(grad_clip=...)).

Synthetic buffers: ~400 k floats of N(0, 1) * 10^U(-3, 1), 70 segments (sizes 1, 3, 1 023, 1 024, 1 025, 4 099, one
empty, one of ~300 k floats, odd offsets, gaps), the gaps of every buffer NaN-filled.  The norms are held to 1 float32
ulp of sqrt(sum(g.astype(float64) ** 2)): the terms are exact in float64, the summation error is at most n * 2^-53
relative (n < 2^19: below 2^-34, far under float32's 2^-25), and one rounding to float32 follows.  Everything else is
bit-for-bit: the reported scales against the table's formulas in numpy float32, and the clipped update against the
existing pp_adamw_step_segments_device run on the host-built g'."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F = np.float32
N = 400_000
LR = (1.1e-3, 0.9e-3, 0.7e-3)
HYPER = (0.9, 0.999, 1e-8, 1e-2)      # beta1, beta2, epsilon, weight decay


def _table():
    """70 segments at odd offsets with gaps, and 10 groups: segment i in group i % 9, the empty segment alone in 9."""
    rng = np.random.default_rng(5)
    sizes = [1, 3, 1023, 1024, 1025, 4099, 0, 300_001] + [int(x) for x in rng.integers(2, 1500, 62)]
    order = rng.permutation(len(sizes))
    segs, groups, off = [], [], 3
    for k, i in enumerate(order):
        off += int(rng.integers(1, 8))
        if sizes[i] > 1 and off % 4 == 0:
            off += 1                                        # not 16-byte aligned
        segs.append((off, sizes[i]))
        groups.append(9 if sizes[i] == 0 else k % 9)
        off += sizes[i]
    assert off < N and len(segs) == 70
    return np.asarray(segs, np.int64), np.asarray(groups, np.int32)


def _mask(segs):
    m = np.zeros(N, bool)
    for off, size in segs:
        m[off:off + size] = True
    return m


class Buffers:
    """Host originals (NaN in the gaps) and the reference sums, computed once for the whole module."""

    def __init__(self):
        rng = np.random.default_rng(11)
        self.segs, self.groups = _table()
        self.n_groups = 10
        self.mask = _mask(self.segs)
        self.g = (rng.normal(size=N) * 10.0 ** rng.uniform(-3, 1, N)).astype(F)
        self.w = (rng.normal(size=N) * 0.1).astype(F)
        self.m = (rng.normal(size=N) * 1e-2).astype(F)
        self.v = (rng.uniform(0, 1e-3, N)).astype(F)
        for a in (self.g, self.w, self.m, self.v):
            a[~self.mask] = np.nan
        sums = np.zeros(self.n_groups)
        for (off, size), k in zip(self.segs, self.groups):
            sums[k] += np.sum(self.g[off:off + size].astype(np.float64) ** 2)
        self.ref_norms = np.sqrt(sums)                      # float64
        self.ref_global = np.sqrt(np.sum(self.g[self.mask].astype(np.float64) ** 2))


@pytest.fixture(scope="module")
def buf():
    return Buffers()


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _np_p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


class Clipper:
    """The stateless C-ABI on torch buffers, with a workspace sized by pp_grad_clip_workspace_bytes."""

    def __init__(self, lib, segs, groups, n_groups):
        self.lib, self.segs, self.groups, self.n_groups = lib, segs, groups, n_groups
        nbytes = ctypes.c_int64(0)
        assert lib.pp_grad_clip_workspace_bytes(N, len(segs), n_groups, ctypes.byref(nbytes)) == 0 and nbytes.value > 0
        self.ws = torch.full((nbytes.value // 4,), -1, dtype=torch.int32, device="cuda")      # need not be cleared

    def stats(self):
        from pp_amd import optim
        torch.cuda.synchronize()
        return optim.AdamW.decode_stats(self.ws[:4 + 2 * self.n_groups].cpu().numpy())

    def norm(self, g):
        st = self.lib.pp_grad_norm_device(0, None, _p(g), N, _np_p(self.segs), len(self.segs), _np_p(self.groups),
                                          self.n_groups, _p(self.ws))
        assert st == 0, self.lib.pp_last_error(None)
        return self.stats()

    def step(self, w, g, m, v, mode, clip, skip, lr_t, workspace=True):
        from pp_amd import _lib
        cfg = _lib.PPGradClipConfig(mode, clip, skip)
        st = self.lib.pp_adamw_step_clipped_device(
            0, None, _p(w), _p(g), _p(m), _p(v), N, _np_p(self.segs), len(self.segs), _np_p(self.groups), self.n_groups,
            ctypes.byref(cfg), _p(self.ws) if workspace else None, lr_t, *HYPER)
        assert st == 0, self.lib.pp_last_error(None)

    def plain(self, w, g, m, v, lr_t):
        st = self.lib.pp_adamw_step_segments_device(0, None, _p(w), _p(g), _p(m), _p(v), _np_p(self.segs), len(self.segs),
                                                    lr_t, *HYPER)
        assert st == 0, self.lib.pp_last_error(None)


def _ulp_close(got, want64):
    want = F(want64)
    return abs(np.float64(got) - np.float64(want)) <= np.spacing(want)


def test_norms(hip_lib, buf):
    g = _dev(buf.g)
    c = Clipper(hip_lib, buf.segs, buf.groups, buf.n_groups)
    st = c.norm(g)
    assert np.isfinite(st["norms"]).all() and np.isfinite(st["global_norm"])      # the NaN gaps are never read
    worst = 0.0
    for k in range(buf.n_groups):
        worst = max(worst, abs(float(st["norms"][k]) - buf.ref_norms[k]) / max(float(np.spacing(F(buf.ref_norms[k]))), 1e-45))
        assert _ulp_close(st["norms"][k], buf.ref_norms[k]), (k, st["norms"][k], buf.ref_norms[k])
    print(f"worst group norm error {worst:.3f} ulp; global {st['global_norm']!r} vs {buf.ref_global!r}")
    assert st["norms"][9] == 0.0                                  # the group of the empty segment
    assert _ulp_close(st["global_norm"], buf.ref_global)
    assert not st["nonfinite"] and not st["skipped"] and st["scale"] == 1.0 and (st["scales"] == 1.0).all()
    first = _bits(c.ws).copy()
    c.ws.fill_(-1)
    c.norm(g)
    assert np.array_equal(_bits(c.ws), first)                     # statistics, group sums and partials alike
    # one group over the same segments: the global norm of the table
    one = Clipper(hip_lib, buf.segs, None, 1)
    s1 = one.norm(g)
    assert _ulp_close(s1["global_norm"], buf.ref_global) and s1["norms"][0] == F(s1["global_norm"])
    assert np.array_equal(_bits(g), _bits(buf.g))


def _expected_scales(mode, c, norms, gnorm):
    """The table's formulas in numpy float32, from the norms the device reported."""
    c = F(c)
    with np.errstate(all="ignore"):
        if mode == 3:
            s = c * np.minimum(F(1) / F(gnorm), F(1) / c)
            return s, np.full(len(norms), s, F)
        if mode == 2:
            return F(1), (c / np.maximum(norms, c)).astype(F)
    return F(1), np.ones(len(norms), F)


def _host_clipped(buf, mode, c, norms, scale):
    c = F(c)
    out = buf.g.copy()
    for (off, size), k in zip(buf.segs, buf.groups):
        g = buf.g[off:off + size]
        if mode == 1:
            out[off:off + size] = np.minimum(np.maximum(g, -c), c)
        elif mode == 2:
            out[off:off + size] = (g * c) / np.maximum(norms[k], c)
        elif mode == 3:
            out[off:off + size] = g * F(scale)
    return out


CASES = ["global-clips", "global-above", "norm-mixed", "value-median", "monitor"]


@pytest.mark.parametrize("case", CASES)
def test_update_every_mode(hip_lib, buf, case):
    grouped = case == "norm-mixed"
    c = Clipper(hip_lib, buf.segs, buf.groups if grouped else None, buf.n_groups if grouped else 1)
    g = _dev(buf.g)
    measured = c.norm(g)
    mode, clip = {"global-clips": (3, F(measured["global_norm"]) * F(0.5)),
                  "global-above": (3, F(measured["global_norm"]) * F(2)),
                  "norm-mixed": (2, np.median(measured["norms"][:9])),
                  "value-median": (1, np.median(np.abs(buf.g[buf.mask]))),
                  "monitor": (0, 0.0)}[case]
    clip = float(F(clip))
    c.ws.fill_(-1)
    a = [_dev(x) for x in (buf.w, buf.m, buf.v)]          # the new call on g
    b = [_dev(x) for x in (buf.w, buf.m, buf.v)]          # the existing kernel on the host-built g'
    for lr_t in LR:                                        # three steps: the moments carry
        c.step(a[0], g, a[1], a[2], mode, clip, 0, lr_t, workspace=(mode != 1))
        if mode == 1:
            norms, scale = None, F(1)
            assert (_bits(c.ws) == 0xffffffff).all()       # "value" without the guard: no reduction ran
        else:
            st = c.stats()
            norms = st["norms"]
            assert np.array_equal(_bits(norms), _bits(measured["norms"])) and st["global_norm"] == measured["global_norm"]
            scale, scales = _expected_scales(mode, clip, norms, st["global_norm"])
            assert _bits(F(st["scale"])) == _bits(F(scale)), (st["scale"], scale)
            assert np.array_equal(_bits(st["scales"]), _bits(scales))
            assert not st["nonfinite"] and not st["skipped"]
            if case == "global-clips":
                assert 0.49 < st["scale"] < 0.51
            if case == "global-above":
                assert 0.999999 <= st["scale"] <= 1.000001
            if case == "norm-mixed":
                clipped = int((norms[:9] > F(clip)).sum())
                assert 0 < clipped < 9, clipped              # some tensors clip and some do not
        gp = buf.g if mode == 0 else _host_clipped(buf, mode, clip, norms, scale)
        c.plain(b[0], _dev(gp), b[1], b[2], lr_t)
        torch.cuda.synchronize()
        for x, y, name in zip(a, b, "wmv"):
            assert np.array_equal(_bits(x), _bits(y)), (case, name, lr_t)
    for x, orig in zip(a, (buf.w, buf.m, buf.v)):
        got = x.cpu().numpy()
        assert np.array_equal(_bits(got[~buf.mask]), _bits(orig[~buf.mask]))      # the gaps: NaN poison untouched
        assert np.isfinite(got[buf.mask]).all() and not np.array_equal(got[buf.mask], orig[buf.mask])
    assert np.array_equal(_bits(g), _bits(buf.g))                                 # the gradient buffer is not rewritten


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_guard(hip_lib, buf, bad):
    c = Clipper(hip_lib, buf.segs, buf.groups, buf.n_groups)
    big = buf.segs[np.argmax(buf.segs[:, 1])]
    hg = buf.g.copy()
    hg[big[0] + 123_457] = bad                   # a value in a trainable entry of the host copy, then uploaded
    g = _dev(hg)
    for mode, clip in ((0, 0.0), (1, 0.5), (2, 0.5), (3, 0.5)):
        a = [_dev(x) for x in (buf.w, buf.m, buf.v)]
        c.ws.fill_(-1)
        c.step(a[0], g, a[1], a[2], mode, clip, 1, LR[0])
        st = c.stats()
        assert st["nonfinite"] and st["skipped"], mode
        for x, orig in zip(a, (buf.w, buf.m, buf.v)):
            assert np.array_equal(_bits(x), _bits(orig)), mode
    # guard off, monitor mode: what the existing kernel makes of the same buffer
    a = [_dev(x) for x in (buf.w, buf.m, buf.v)]
    b = [_dev(x) for x in (buf.w, buf.m, buf.v)]
    c.step(a[0], g, a[1], a[2], 0, 0.0, 0, LR[0])
    st = c.stats()
    assert st["nonfinite"] and not st["skipped"]
    c.plain(b[0], g, b[1], b[2], LR[0])
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    assert not np.array_equal(_bits(a[0]), _bits(buf.w))
    # guard off, global_norm: a NaN scale, as TensorFlow gives
    c.step(a[0], g, a[1], a[2], 3, 0.5, 0, LR[1])
    st = c.stats()
    assert np.isnan(st["scale"]) and st["nonfinite"] and not st["skipped"]


def test_guard_ignores_the_gaps(hip_lib, buf):
    c = Clipper(hip_lib, buf.segs, buf.groups, buf.n_groups)
    hg = buf.g.copy()
    assert np.isnan(hg[~buf.mask]).all()         # a NaN in the gaps only
    hg[np.flatnonzero(~buf.mask)[::2]] = np.inf
    a = [_dev(x) for x in (buf.w, buf.m, buf.v)]
    c.step(a[0], _dev(hg), a[1], a[2], 3, 1.0, 1, LR[0])
    st = c.stats()
    assert not st["nonfinite"] and not st["skipped"] and np.isfinite(st["global_norm"])
    assert not np.array_equal(_bits(a[0]), _bits(buf.w))


def test_guard_skips_a_norm_beyond_float32(hip_lib, buf):
    """Finite gradients whose norm exceeds FLT_MAX: the float64 sum is finite (nonfinite stays 0), the float32 norm is
    Inf and global_norm's scale NaN -- the guard skips the step; without it the NaN scale goes through, as in TensorFlow."""
    c = Clipper(hip_lib, buf.segs, None, 1)
    big = buf.segs[np.argmax(buf.segs[:, 1])]
    hg = buf.g.copy()
    hg[big[0] + 5:big[0] + 9] = F(3e38)
    g = _dev(hg)
    a = [_dev(x) for x in (buf.w, buf.m, buf.v)]
    c.step(a[0], g, a[1], a[2], 3, 1.0, 1, LR[0])
    st = c.stats()
    assert not st["nonfinite"] and st["skipped"] and np.isinf(st["global_norm"]) and np.isnan(st["scale"])
    for x, orig in zip(a, (buf.w, buf.m, buf.v)):
        assert np.array_equal(_bits(x), _bits(orig))
    c.step(a[0], g, a[1], a[2], 3, 1.0, 0, LR[0])
    st = c.stats()
    assert not st["nonfinite"] and not st["skipped"] and np.isnan(st["scale"])
    assert np.isnan(a[0].cpu().numpy()[buf.mask]).all()


# ---- Trainer ----------------------------------------------------------------------------------------------------------
def _small_cfg(pp, name, B=2):
    cfg = pp.config.tiny_config(B)
    if name == "deep":
        cfg["model"]["second"]["rpn"].update(layer_nums=[3, 5, 5])
    return cfg


def _frames(seed, ns=(900, 400)):
    rng = np.random.default_rng(seed)
    return [rng.uniform([0, -0.64, -3], [1.6, 0.64, 3], (n, 3)).astype(np.float32) for n in ns]


def _targets(d, B, seed, npos=40):
    rng = np.random.default_rng(seed)
    A = d.num_anchors
    labels = rng.choice([-1, 0, 0, 0, 0], size=(B, A)).astype(np.int32)
    reg = np.zeros((B, A, 7), np.float32)
    for b in range(B):
        pos = rng.choice(A, npos if b == 0 else npos // 3, replace=False)
        labels[b, pos] = 1
        reg[b, pos] = rng.normal(0, 0.4, (len(pos), 7)).astype(np.float32)
    return labels, reg


def _problem(pp, name="tiny", B=2):
    cfg = _small_cfg(pp, name, B)
    d = pp.config.Derived(cfg)
    labels, reg = _targets(d, B, 11)
    return cfg, d, _frames(4), labels, reg, pp.weights.init_weights(d, seed=21)


def _host_norm(grads):
    return np.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in grads.values()))


def _state(tr):
    return [_bits(t).copy() for t in (tr.params, tr.optimizer.m, tr.optimizer.v)]


def test_trainer_global_norm_matches_scaled_plain_trainer(pp, hip_lib):
    GradClip = pp.optim.GradClip
    cfg, d, frames, labels, reg, w = _problem(pp)
    kw = dict(max_batch=2, max_points_per_frame=4096)
    mon = pp.Trainer(cfg, w, grad_clip=GradClip(), **kw)                 # monitor mode: an unclipped run's norm
    mon.forward_backward(frames, labels, reg)
    assert mon.grad_stats() is None
    mon.apply_gradients()
    st = mon.grad_stats()
    assert st["scale"] == 1.0 and not st["nonfinite"] and not st["skipped"] and mon.steps_skipped == 0
    assert _ulp_close(st["global_norm"], _host_norm(mon.gradients()))
    clip = float(F(st["global_norm"]) * F(0.5))
    plain0 = pp.Trainer(cfg, w, **kw)                                    # ... and monitoring changes nothing
    plain0.forward_backward(frames, labels, reg)
    plain0.apply_gradients()
    for x, y in zip(_state(mon), _state(plain0)):
        assert np.array_equal(x, y)
    mon.close()
    plain0.close()
    A = pp.Trainer(cfg, w, grad_clip=GradClip("global_norm", clip), **kw)
    B = pp.Trainer(cfg, w, **kw)
    for k in range(2):
        A.forward_backward(frames, labels, reg)
        B.forward_backward(frames, labels, reg)
        assert np.array_equal(_bits(A.grads), _bits(B.grads))
        raw = A.gradients()
        A.apply_gradients()
        st = A.grad_stats()
        assert _ulp_close(st["global_norm"], _host_norm(raw))
        want, _ = _expected_scales(3, clip, st["norms"], st["global_norm"])
        assert _bits(F(st["scale"])) == _bits(F(want)) and st["scale"] < 1.0
        for name, g in A.gradients().items():                            # still the raw gradients
            assert np.array_equal(g, raw[name])
        B.grads.mul_(float(F(st["scale"])))        # one float32 rounding per entry, as the kernel's g * scale
        torch.cuda.synchronize()                   # (torch's stream, not the engine's)
        B.apply_gradients()
        for x, y, name in zip(_state(A), _state(B), "wmv"):
            assert np.array_equal(x, y), (k, name)
    assert A.optimizer.iterations == B.optimizer.iterations == 2 and A.steps_skipped == 0
    out = A.step(frames, labels, reg)
    assert out["step_skipped"] is False and out["grad_norm"] == A.grad_stats()["global_norm"] > 0
    A.close()
    B.close()


def test_trainer_frozen_norm_covers_the_trainable_tensors(pp, hip_lib):
    from pp_amd import trainer
    GradClip = pp.optim.GradClip
    cfg, d, frames, labels, reg, w = _problem(pp, "deep")
    tr = pp.Trainer(cfg, w, max_batch=2, max_points_per_frame=4096, frozen="reference", grad_clip=GradClip("norm", 1e-3))
    units = set(tr.frozen)
    assert units
    mask = np.zeros(tr.params.numel(), bool)
    for name, off, size, is_state in tr.layout:
        if not is_state and trainer.unit_of(name) in units:
            mask[off:off + size] = True
    before = _state(tr)
    tr.forward_backward(frames, labels, reg)
    grads = tr.gradients()
    assert not any(trainer.unit_of(k) in units for k in grads)
    tr.apply_gradients()
    st = tr.grad_stats()
    assert _ulp_close(st["global_norm"], _host_norm(grads))
    assert tr.grad_groups == list(grads) and len(st["norms"]) == len(grads)
    for k, name in enumerate(tr.grad_groups):                             # per-tensor norms
        assert _ulp_close(st["norms"][k], np.sqrt(np.sum(grads[name].astype(np.float64) ** 2))), name
    assert (st["scales"] < 1).any()
    for x, y in zip(_state(tr), before):
        assert np.array_equal(x[mask], y[mask])                           # frozen parameters and moments: untouched
        assert not np.array_equal(x[~mask], y[~mask])
    tr.set_trainable(True)                                                # the groups are rebuilt: everything counts
    tr.forward_backward(frames, labels, reg)
    grads = tr.gradients()
    assert any(trainer.unit_of(k) in units for k in grads)
    mid = _state(tr)
    tr.apply_gradients()
    st = tr.grad_stats()
    assert tr.grad_groups == list(grads) and len(st["norms"]) == len(grads)
    assert _ulp_close(st["global_norm"], _host_norm(grads))
    for x, y in zip(_state(tr), mid):
        assert not np.array_equal(x[mask], y[mask])
    tr.close()


def test_trainer_guard_skips_the_poisoned_step(pp, hip_lib):
    GradClip = pp.optim.GradClip
    cfg, d, frames, labels, reg, w = _problem(pp)
    kw = dict(max_batch=2, max_points_per_frame=4096, grad_clip=GradClip("global_norm", 0.05, skip_nonfinite=True))
    tr = pp.Trainer(cfg, w, **kw)
    clean = pp.Trainer(cfg, w, **kw)                 # never sees the poisoned step
    state0 = tr.state.clone()
    before = _state(tr)
    tr.forward_backward(frames, labels, reg)
    tr.grads[tr.grads.numel() // 2] = float("nan")   # a value in the buffer
    torch.cuda.synchronize()
    tr.apply_gradients()
    st = tr.grad_stats()
    assert st["nonfinite"] and st["skipped"]
    for x, y in zip(_state(tr), before):
        assert np.array_equal(x, y)
    assert tr.optimizer.iterations == 0 and tr.steps_skipped == 1
    # the BatchNorm moving statistics moved in the forward pass; give both trainers the same ones for the clean step
    tr.state.copy_(state0)
    a = tr.step(frames, labels, reg)
    b = clean.step(frames, labels, reg)
    assert a == b and a["step_skipped"] is False and np.isfinite(a["grad_norm"])
    for x, y in zip(_state(tr), _state(clean)):
        assert np.array_equal(x, y)
    assert tr.optimizer.iterations == clean.optimizer.iterations == 1 and tr.steps_skipped == 1
    tr.close()
    clean.close()


def test_off_is_off(pp, hip_lib, monkeypatch):
    cfg, d, frames, labels, reg, w = _problem(pp)
    calls = []
    for name in ("pp_adamw_step_clipped_device", "pp_grad_norm_device"):
        real = getattr(hip_lib, name)
        monkeypatch.setattr(hip_lib, name, lambda *a, _n=name, _f=real: (calls.append(_n), _f(*a))[1])
    tr = pp.Trainer(cfg, w, max_batch=2, max_points_per_frame=4096)
    keys = set(tr.forward_backward(frames, labels, reg))
    out = tr.step(frames, labels, reg)
    assert set(out) == keys and "grad_norm" not in out and "step_skipped" not in out
    tr.set_frozen(["pfn"])
    assert set(tr.step(frames, labels, reg)) == keys
    assert calls == [] and tr.grad_clip is None and tr.steps_skipped == 0
    with pytest.raises(RuntimeError):
        tr.grad_stats()
    tr.close()
    with pytest.raises(ValueError):                  # True reads the configuration key and insists on it
        pp.Trainer(cfg, w, max_batch=2, max_points_per_frame=4096, grad_clip=True)
    cfg2 = dict(cfg)
    cfg2["train_config"] = dict(cfg.get("train_config") or {}, gradient_clipping={"mode": "value", "clip": 0.01})
    try:
        tr = pp.Trainer(cfg2, w, max_batch=2, max_points_per_frame=4096, grad_clip=True, learning_rate=1e-4, weight_decay=1e-4)
    except ValueError:
        pytest.fail("grad_clip=True with the key present must build")
    out = tr.step(frames, labels, reg)
    assert tr.grad_clip.mode == "value" and out["grad_norm"] is None and out["step_skipped"] is False
    assert calls == ["pp_adamw_step_clipped_device"]
    tr.close()


def test_set_grad_clip_on_a_live_trainer(pp, hip_lib):
    """off -> global_norm -> norm -> off on one trainer, a step each: every step matches, to the bit, a fresh trainer
    built with that setting from the same weights, moments and step count; the statistics buffer follows the group
    count, and off is the unclipped calls again."""
    GradClip = pp.optim.GradClip
    cfg, d, frames, labels, reg, w = _problem(pp)
    kw = dict(max_batch=2, max_points_per_frame=4096)
    live = pp.Trainer(cfg, w, **kw)
    with pytest.raises(ValueError):
        live.set_grad_clip("global_norm")
    for clip in (None, GradClip("global_norm", 0.05, skip_nonfinite=True), GradClip("norm", 1e-3), None):
        live.set_grad_clip(clip)
        fresh = pp.Trainer(cfg, live.weights(), grad_clip=clip, **kw)
        fresh.optimizer.m.copy_(live.optimizer.m)
        fresh.optimizer.v.copy_(live.optimizer.v)
        fresh.optimizer.iterations = live.optimizer.iterations
        a, b = live.step(frames, labels, reg), fresh.step(frames, labels, reg)
        assert a == b and ("grad_norm" in a) == (clip is not None)
        for x, y in zip(_state(live), _state(fresh)):
            assert np.array_equal(x, y)
        if clip is None:
            assert live.optimizer.clip is None and live.optimizer.segments is None
            with pytest.raises(RuntimeError):
                live.grad_stats()
        else:
            st, sf = live.grad_stats(), fresh.grad_stats()
            assert st["global_norm"] == sf["global_norm"] == a["grad_norm"] > 0
            assert len(st["norms"]) == (len(live.grad_groups) if clip.mode == "norm" else 1)
            assert np.array_equal(_bits(st["scales"]), _bits(sf["scales"]))
        fresh.close()
    assert live.steps_skipped == 0 and live.optimizer.iterations == 4
    live.close()
