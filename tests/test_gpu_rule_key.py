"""The post-process rule as a whole is part of a captured pass's key (csrc/pp_engine.h: PostRule, DetectKey; detect_key in
csrc/pp_api.hip): one long-lived engine walks through every rule field and must never replay a pass captured under
another rule.  Everything compared is bytes: the passes are deterministic, so there is no tolerance.

Every upload flips the input buffer, which is part of the key as well: the two `detect` calls of a stop capture one pass
per buffer, and the third pass at each stop (the resident frames again) is the replay of the slot just captured.  The walk
takes more slots than the cache of 8 has, so the later stops also evict, and stops 4 and 8 replay (or re-capture) stop 1's.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 2


def _p2():
    return np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2], [0, 0, 1, 0.003], [0, 0, 0, 1]], np.float64)


def _engine(pp, **second):
    cfg = pp.config.pedestrian_d435i_config(B)
    cfg["model"]["second"].update(second)
    eng = pp.Engine(cfg, max_batch=B, max_points_per_frame=8192)
    eng.load_weights(pp.weights.init_weights(eng.d, seed=7))
    return eng


def _set_rule(eng, mode, sigma=None, per_class=False, project=False):
    if sigma is not None:
        eng.set_soft_nms(method="gaussian", sigma=sigma)
    eng.set_nms_mode(mode)
    eng.set_class_nms("per_class" if per_class else "joint")
    eng.set_projection(_p2() if project else None)


def _result(eng, out):
    dets, n = out
    kept = [dets[b][:int(n[b])].tobytes() for b in range(B)]
    return n.copy(), kept, (eng.bboxes(B).tobytes() if eng.projection else None)


def _passes(eng, frames, rect, trv, what):
    """detect twice (the second call meets the other input buffer), then the resident frames once more: a replay."""
    first = _result(eng, eng.detect(frames, rect, trv))
    again = _result(eng, eng.detect(frames, rect, trv))
    eng.detect_async()
    eng.sync()
    replay = _result(eng, eng.detections())
    for other in (again, replay):
        assert np.array_equal(first[0], other[0]), what
        assert first[1] == other[1], what
        assert first[2] == other[2], what
    return first


def test_every_rule_field_selects_its_own_pass(pp, hip_lib):
    rect, trv, _ = pp.synth.default_calib()
    rect, trv = np.stack([rect] * B), np.stack([trv] * B)
    frames = [pp.synth.d435i_cloud(900 + 10 * i, 4096) for i in range(B)]
    # the rule an engine has from its creation, per distinct rule of the walk
    fresh = {}
    # (the config refuses use_multi_class_nms with this configuration's single class: that engine is switched, like its
    # projection, before its first pass)
    for name, second, per_class in (("standup", {}, False),
                                    ("soft 0.1", dict(use_soft_nms=True, soft_nms={"method": "gaussian", "sigma": 0.1}), False),
                                    ("rotated", dict(use_rotate_nms=True), False),
                                    ("per class + projection", {}, True)):
        e = _engine(pp, **second)
        try:
            if per_class:
                e.set_class_nms("per_class")
                e.set_projection(_p2())
            fresh[name] = _passes(e, frames, rect, trv, f"fresh engine, {name}")
        finally:
            e.close()
    walk = [("standup", dict(mode="standup"), "standup"),
            ("soft 0.5", dict(mode="soft", sigma=0.5), None),
            ("soft 0.1", dict(mode="soft", sigma=0.1), "soft 0.1"),
            ("standup again", dict(mode="standup"), "standup"),
            ("rotated", dict(mode="rotated"), "rotated"),
            ("per class", dict(mode="standup", per_class=True), "per class + projection"),
            ("per class + projection", dict(mode="standup", per_class=True, project=True), "per class + projection"),
            ("standup at the end", dict(mode="standup"), "standup")]
    eng = _engine(pp)
    try:
        seen = []
        for stop, (name, rule, ref) in enumerate(walk, 1):
            _set_rule(eng, **rule)
            got = _passes(eng, frames, rect, trv, f"stop {stop}, {name}")
            seen.append(got)
            print(f"stop {stop} ({name}): kept {got[0].tolist()}, boxes {'yes' if got[2] is not None else 'no'}")
            if ref is not None:
                want = fresh[ref]
                assert np.array_equal(got[0], want[0]) and got[1] == want[1], f"stop {stop}, {name}: not the fresh engine's rows"
                if got[2] is not None:
                    assert got[2] == want[2], f"stop {stop}, {name}: not the fresh engine's image boxes"
        for stop in (4, 8):
            assert np.array_equal(seen[stop - 1][0], seen[0][0]) and seen[stop - 1][1] == seen[0][1], f"stop {stop} is not stop 1"
        assert seen[5][2] is None and seen[6][2] is not None and seen[7][2] is None
        # the soft parameters alone select another pass (tests/test_gpu_soft_nms.py holds the same clouds to it)
        assert seen[1][1] != seen[2][1]
    finally:
        eng.close()
