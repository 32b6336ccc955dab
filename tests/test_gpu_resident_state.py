"""The resident frames' bookkeeping across every feed transition: one engine is driven through zero-copy and copy feeds,
augmentation, GT sampling, the object-database build, a PointCloud2 ingest and a sampled training step, and each
step's outputs -- points, boxes, counts, detections, losses, gradients -- equal, bit for bit, what a newly created
engine returns for that step alone (the same kernels on the same data: no tolerance)."""
import random

import numpy as np
import pytest

from test_gpu_gt_sample import _ped_db

pytestmark = pytest.mark.gpu

B_ZC, B_COPY = 2, 5          # either side of ZC_MAX_BATCH = 4: the zero-copy feed and the copy feed
NMAX = 4096


class _Problem:
    def __init__(self, pp):
        rng = np.random.default_rng(71)
        self.pp = pp
        self.cfg = pp.config.tiny_config(B_COPY)
        self.weights = pp.weights.init_weights(pp.config.Derived(self.cfg), seed=7)
        self.db = _ped_db(pp)
        self.acfg = pp.augment.AugmentConfig.from_input_reader({})
        self.frames, self.gt, self.cls, self.val, self.cand, self.draws = {}, {}, {}, {}, {}, {}
        for B in (B_ZC, B_COPY):
            fr, gt = [], []
            for b in range(B):
                n = int(rng.integers(200, 400))
                fr.append(np.stack([rng.uniform(0.0, 1.6, n), rng.uniform(-0.64, 0.64, n), rng.uniform(-1.4, 1.4, n)],
                                   1).astype(np.float32))
                g = 1 + b % 2          # small boxes in the grid's corners: the database's objects find room beside them
                gt.append(np.stack([rng.uniform(0.1, 0.3, g), rng.uniform(-0.6, 0.6, g), np.full(g, -0.4), np.full(g, 0.15),
                                    np.full(g, 0.2), np.full(g, 1.6), rng.uniform(-3.1, 3.1, g)], 1).astype(np.float32))
            self.frames[B], self.gt[B] = fr, gt
            self.cls[B] = [np.ones(len(g), np.int32) for g in gt]
            self.val[B] = [np.arange(len(g)) % 2 == 0 for g in gt]
            self.cand[B] = pp.gt_sampler.draw_candidates(self.db, self.cls[B], random.Random(71 + B))
            self.draws[B] = pp.augment.draw(np.random.RandomState(B), gt, self.acfg)
        # the sampled step's draws: a frame's boxes plus the slots of its largest round
        padded = [np.concatenate([np.asarray(g, np.float64), np.zeros((int(x), 7))], 0)
                  for g, x in zip(self.gt[B_ZC], self.cand[B_ZC].counts.max(axis=1))]
        self.step_draws = pp.augment.draw(np.random.RandomState(9), padded, self.acfg)
        self.msgs = [pp.synth.pointcloud2_message(i, 32, 24) for i in range(B_ZC)]
        self.stagings = []

    def engine(self):
        eng = self.pp.Engine(self.cfg, max_batch=B_COPY, max_points_per_frame=NMAX)
        eng.load_weights(self.weights)
        eng.load_gt_database(self.db)
        return eng

    def upload_async(self, eng, B):
        st = eng.staging(self.frames[B])
        self.stagings.append(st)          # page-locked: lives until the passes that read it are through
        eng.upload_async(st)


def _flat(out):
    return [np.ascontiguousarray(a).tobytes() for o in out for a in o]


def _detect(p, eng, B):
    rect, trv, _ = p.pp.synth.default_calib()
    eng.set_calib(np.stack([rect] * B), np.stack([trv] * B), B)
    eng.detect_async()
    eng.sync()
    dets, n = eng.detections()
    im = eng.intermediates()
    return [dets[:B].tobytes(), n[:B].tobytes()] + [im[k][:B].tobytes() for k in ("n_pillars", "coors", "anchors_mask",
                                                                                  "box_preds", "cls_preds")]


def _zero_copy_augment_detect(p, eng):
    p.upload_async(eng, B_ZC)
    out = eng.augment(p.gt[B_ZC], p.cls[B_ZC], p.val[B_ZC], p.draws[B_ZC], p.acfg)
    return _flat(out) + _detect(p, eng, B_ZC)


def _copy_sample_count_detect(p, eng):
    p.upload_async(eng, B_COPY)
    out = eng.gt_sample(p.gt[B_COPY], p.cls[B_COPY], p.val[B_COPY], p.cand[B_COPY])
    counts = eng.count_points_in_gt([np.asarray(o[1], np.float64) for o in out])
    return _flat(out) + [c.tobytes() for c in counts] + _detect(p, eng, B_COPY)


def _zero_copy_build_detect(p, eng):
    p.upload_async(eng, B_ZC)
    objs = eng.build_gt_objects([np.asarray(g, np.float64) for g in p.gt[B_ZC]])
    return [o.tobytes() for f in objs for o in f] + _detect(p, eng, B_ZC)      # the same, untouched zero-copy frames


def _ingest_refuse_upload_augment(p, eng):
    eng.ingest_pointcloud2(p.msgs)
    eng._offsets = np.zeros(B_ZC + 1, np.int64)      # past the binding's own check: the library refuses
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*upload frames first"):
        eng.augment(p.gt[B_ZC], p.cls[B_ZC], p.val[B_ZC], p.draws[B_ZC], p.acfg)
    eng.upload(p.frames[B_COPY])
    return _flat(eng.augment(p.gt[B_COPY], p.cls[B_COPY], p.val[B_COPY], p.draws[B_COPY], p.acfg))


def _sampled_step_then_sample(p, eng):
    import torch
    layout, n_params, n_state = eng.train_layout()
    host = [np.zeros(n_params, np.float32), np.zeros(n_state, np.float32)]
    for name, off, size, is_state in layout:
        host[is_state][off:off + size] = np.asarray(p.weights[name], np.float32).reshape(-1)
    params, state = (torch.from_numpy(h).cuda() for h in host)
    grads = torch.zeros_like(params)
    torch.cuda.synchronize()
    B = B_ZC
    p.upload_async(eng, B)
    boxes, classes, counts = eng.pack_gt(p.gt[B], p.cls[B])
    eng.train_step_sample_async(params.data_ptr(), grads.data_ptr(), state.data_ptr(), boxes, classes, counts, p.val[B],
                                p.cand[B], p.db.config, p.step_draws, p.acfg)
    losses = eng.train_step_wait()
    with pytest.raises(RuntimeError, match="PP_ERR_STATE.*sampled inside a training step"):
        eng.gt_sample(p.gt[B], p.cls[B], p.val[B], p.cand[B])
    eng.upload(p.frames[B])
    out = eng.gt_sample(p.gt[B], p.cls[B], p.val[B], p.cand[B])
    return [repr(losses).encode(), grads.cpu().numpy().tobytes(), state.cpu().numpy().tobytes()] + _flat(out)


def test_every_feed_transition_equals_a_fresh_engine(pp, hip_lib):
    p = _Problem(pp)
    steps = [_zero_copy_augment_detect, _copy_sample_count_detect, _zero_copy_build_detect, _ingest_refuse_upload_augment,
             _sampled_step_then_sample]
    eng = p.engine()
    for step in steps:
        got = step(p, eng)
        fresh = p.engine()
        want = step(p, fresh)
        fresh.close()
        assert len(got) == len(want), step.__name__
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, f"{step.__name__}: output {i} differs from a fresh engine's"
    eng.close()
    for st in p.stagings:
        st.close()
