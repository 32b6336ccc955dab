"""Golden vectors for the GT-database sampling (pp_amd.gt_sampler, csrc/gt_sample.hip), produced by RUNNING the
reference's own DataBaseSamplerV2, BatchSampler and sample_all (load_data.py:1344-1467, :1690-1921) on a small synthetic
database written to a temporary directory in the reference's file layout (build container only, through ref_shim).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_gtsample.py   ->  tests/golden/ref_gt_sample.npz

Recorded (data only): the database as given and after construction (shuffled indices, translated boxes), every cursor
call since construction (class, num, returned indices), and per kept case the inputs, the candidates, the survivors of
the box test with their point counts (the arguments / results of the reference's points_in_rbbox calls), the `low`
coins (the recorded getrandbits values, short-circuit), and sample_all's outputs.  A case is one frame; a frame without
boxes calls sample_all once per round until something is accepted, as the loader's loop does.
What is NOT recorded from the reference: the per-slot `status`, `point_counts`, `accepted` and `round_used` arrays of
a case are what gt_sampler.sample_all_np returned for it.  The reference has no such outputs; they are tied to it by
the assertions below, per round: the survivors of the restatement's box test are exactly the boxes the reference passed
to points_in_rbbox, in order, with the same point counts, and the restatement's pasted cloud, appended boxes and class
names equal sample_all's return -- a wrong status would change one of those.
Margins, asserted: no frame point within 1e-5 m of a face of ANY database box; no collision decision of a kept case
changes when a candidate moves by +-1e-6 m.
"""
import os
import pickle
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

ld, _ = ref_shim.load_reference()
import pp_amd  # noqa: E402

aug, gts = pp_amd.augment, pp_amd.gt_sampler
SEED = 31
READER = dict(gts._DEFAULTS)

_log = {"cursor": [], "rbbox": [], "bits": []}
_orig_sample = ld.BatchSampler._sample
_orig_rbbox = ld.points_in_rbbox
_orig_bits = random.getrandbits


def _rec_sample(self, num):
    r = _orig_sample(self, num)
    _log["cursor"].append((self._name, int(num), np.array(r)))
    return r


def _rec_rbbox(points, rbbox, *a, **k):
    r = _orig_rbbox(points, rbbox, *a, **k)
    _log["rbbox"].append((np.array(rbbox[0], np.float64), int(r.sum(0)[0])))
    return r


def _rec_bits(k):
    v = _orig_bits(k)
    _log["bits"].append(int(v))
    return v


ld.BatchSampler._sample = _rec_sample
ld.points_in_rbbox = _rec_rbbox


def make_database(rng):
    infos, points = {"Pedestrian": [], "Cyclist": []}, {"Pedestrian": [], "Cyclist": []}
    for name, n in (("Pedestrian", 42), ("Cyclist", 8)):
        for i in range(n):
            w, l, h = (0.6, 0.8, 1.7) if name == "Pedestrian" else (0.6, 1.6, 1.6)
            box = np.array([rng.uniform(0.4, 6.0), rng.uniform(-1.2, 1.2), rng.uniform(-0.9, -0.5),
                            w * rng.uniform(0.85, 1.15), l * rng.uniform(0.85, 1.15), h * rng.uniform(0.9, 1.1),
                            rng.uniform(-np.pi, np.pi)])
            npts = int(rng.integers(12, 48))
            diff = 0
            if name == "Pedestrian" and i in (5, 17):
                diff = -1                       # removed at construction
            if name == "Pedestrian" and i in (3, 11, 23, 30):
                npts = 0                        # an object without points
            if name == "Cyclist" and i == 2:
                npts = 3                        # below the Cyclist minimum of 5
            u = rng.uniform(-0.45, 0.45, (npts, 3))
            c, s = np.cos(box[6]), np.sin(box[6])
            lx, ly = u[:, 0] * box[3], u[:, 1] * box[4]
            p = np.stack([lx * c + ly * s, -lx * s + ly * c, (u[:, 2] + 0.5) * box[5]], 1).astype(np.float32)
            infos[name].append({"name": name, "path": f"gt_database/{name}_{i}.bin", "box3d_lidar": box,
                                "difficulty": diff, "num_points_in_gt": npts, "group_id": i})
            points[name].append(p)
    return infos, points


def write_database(tmp, infos, points):
    os.makedirs(os.path.join(tmp, "gt_database"))
    with open(os.path.join(tmp, "dbinfos.pkl"), "wb") as f:
        pickle.dump(infos, f)
    for name, objs in infos.items():
        for o, p in zip(objs, points[name]):
            with open(os.path.join(tmp, o["path"][:-3] + "pkl"), "wb") as f:
                pickle.dump(p, f)


def make_frame(rng, n, all_boxes, hole_x=None):
    p = np.stack([rng.uniform(0.05, 6.35, n), rng.uniform(-2.5, 2.5, n), rng.uniform(-1.4, 1.4, n)], 1).astype(np.float32)
    if hole_x is not None:
        p = p[p[:, 0] > hole_x]
    pn, pd = aug.box_planes(all_boxes)
    sg = aug.face_sign(p.astype(np.float64), pn, pd)
    far = (np.abs(sg) / np.linalg.norm(pn, axis=-1)[None]).min(axis=(1, 2)) > 1e-5
    return p[far]


def lows_from_bits(bits, n):
    """The n coins the recorded getrandbits values make (three per coin, short-circuit on the first 0)."""
    out, i = [], 0
    for _ in range(n):
        v = True
        for _k in range(3):
            b = bits[i]
            i += 1
            if not b:
                v = False
                break
        out.append(v)
    assert i == len(bits), (i, len(bits))
    return out


def robust(frame_boxes, cand_boxes):
    """No collision decision among (frame boxes + candidates) changes when a candidate moves by +-1e-6 m."""
    fc = aug.box_corners_2d(*(frame_boxes[:, k] for k in (0, 1, 3, 4, 6)))
    cc = aug.box_corners_2d(*(cand_boxes[:, k] for k in (0, 1, 3, 4, 6)))
    every = np.concatenate([fc, cc], 0)
    base = aug.collide(cc[:, None], every[None])
    for dx, dy in ((1e-6, 0), (-1e-6, 0), (0, 1e-6), (0, -1e-6), (1e-6, 1e-6), (-1e-6, -1e-6)):
        moved = cc + np.array([dx, dy])
        a = aug.collide(moved[:, None], every[None])
        b = aug.collide(cc[:, None], np.concatenate([fc, moved], 0)[None])
        n = len(cc)
        a[np.arange(n), len(fc) + np.arange(n)] = base[np.arange(n), len(fc) + np.arange(n)]
        b[np.arange(n), len(fc) + np.arange(n)] = base[np.arange(n), len(fc) + np.arange(n)]
        if (a != base).any() or (b != base).any():
            return False
    return True


def main():
    rng = np.random.default_rng(2025)
    infos, points = make_database(rng)
    out = {}
    for name in infos:
        out[f"db_in__{name}__boxes"] = np.array([o["box3d_lidar"] for o in infos[name]])
        out[f"db_in__{name}__difficulty"] = np.array([o["difficulty"] for o in infos[name]])
        out[f"db_in__{name}__num_points"] = np.array([o["num_points_in_gt"] for o in infos[name]])
        out[f"db_in__{name}__points"] = np.concatenate(points[name], 0)
        out[f"db_in__{name}__offsets"] = np.concatenate([[0], np.cumsum([len(p) for p in points[name]])])
    tmp = tempfile.mkdtemp()
    write_database(tmp, infos, points)
    np.random.seed(SEED)
    random.seed(SEED)
    sampler = ld.DataBaseSamplerV2(os.path.join(tmp, "dbinfos.pkl"), READER)
    for name, bs in sampler._sampler_dict.items():
        out[f"db__{name}__indices"] = np.array(bs._indices)
        out[f"db__{name}__boxes"] = np.array([o["box3d_lidar"] for o in bs._sampled_list], np.float64)
    # the twin, built from the same inputs and seeds: its flat arrays are what the cases index
    cfg2 = gts.SamplerConfig.from_input_reader({"sample_classes": ["Pedestrian", "Cyclist"], "sample_max_nums": [5, 3]})
    db = gts.GtDatabase(infos, points, cfg2, np.random.RandomState(SEED), random.Random(SEED), 3)
    for name in infos:
        assert np.array_equal(db.samplers[name].boxes, out[f"db__{name}__boxes"]), name
        assert np.array_equal(db.samplers[name].indices, out[f"db__{name}__indices"]), name
    all_boxes = np.concatenate([out["db__Pedestrian__boxes"], out["db__Cyclist__boxes"]], 0)
    frames = {"full": make_frame(rng, 3000, all_boxes), "hole": make_frame(rng, 3000, all_boxes, hole_x=2.9)}
    for k, v in frames.items():
        out[f"frame__{k}"] = v

    def call(frame, gt_boxes, gt_names, classes, nums, max_pc, min_pc):
        """One frame: sample_all per round as the loader's loop calls it.  Returns the recorded rounds."""
        rounds = []
        while True:
            _log["rbbox"].clear()
            _log["bits"].clear()
            c0 = len(_log["cursor"])
            random.getrandbits = _rec_bits
            try:
                ret = ld.sample_all(sampler, tmp, gt_boxes, gt_names, 3, True, classes, nums, max_pc, min_pc,
                                    points=frame.copy())
            finally:
                random.getrandbits = _orig_bits
            cur = _log["cursor"][c0:]
            surv = list(_log["rbbox"])
            rounds.append({"cursor": cur, "surv_boxes": np.array([s[0] for s in surv]).reshape(-1, 7),
                           "surv_counts": np.array([s[1] for s in surv], np.int64),
                           "low": np.array(lows_from_bits(list(_log["bits"]), len(surv)), bool), "ret": ret})
            if len(gt_boxes) or ret is not None or len(rounds) == gts.PP_GTS_MAX_ROUNDS:
                return rounds

    def box32(x, y, r=0.0, z=-0.7, w=0.6, l=0.8, h=1.7):
        return np.array([x, y, z, w, l, h, r], np.float32).astype(np.float64)

    PED, CYC = ["Pedestrian"], ["Pedestrian", "Cyclist"]
    plans = [  # name, frame, boxes, names, classes, nums, max_pc, min_pc, wanted property
        ("shipped", "full", [box32(1.5, -2.0, 0.3), box32(4.5, 2.0, -1.1)], ["Pedestrian"] * 2, PED, [8], 500, 1, None),
        ("no_boxes", "full", [], [], PED, [8], 500, 1, None),
        ("two_classes", "full", [box32(3.0, 2.1, 0.2)], ["Pedestrian"], CYC, [5, 3], 500, 1, "second_avoids_first"),
        ("later_candidate", "full", [box32(5.9, -2.2)], ["Pedestrian"], PED, [8], 500, 1, "later"),
        ("near_low", "hole", [box32(5.5, 2.2)], ["Pedestrian"], PED, [8], 500, 1, "near_low"),
        ("max_points", "full", [box32(5.9, 2.2)], ["Pedestrian"], PED, [8], 18, 1, "max"),
        ("empty_object", "full", [box32(0.5, 2.2)], ["Pedestrian"], PED, [8], 500, 1, "empty"),
        ("enough_boxes", "full", [box32(0.8 + 0.7 * i, 2.1) for i in range(8)], ["Pedestrian"] * 8, PED, [8], 500, 1, "none"),
        ("cyclist_only", "full", [box32(0.8 + 0.7 * i, 2.1) for i in range(5)], ["Pedestrian"] * 5, CYC, [5, 3], 500, 1, None),
    ]
    cases = []
    for name, fkey, boxes, names, classes, nums, max_pc, min_pc, want in plans:
        gt = np.array(boxes, np.float64).reshape(-1, 7)
        gt_names = np.array(names)
        cfg = gts.SamplerConfig.from_input_reader({"sample_classes": classes, "sample_max_nums": nums,
                                                   "sampler_max_point_collision": max_pc,
                                                   "sampler_min_point_collision": min_pc})
        for attempt in range(60):
            rounds = call(frames[fkey], gt, gt_names, classes, nums, max_pc, min_pc)
            # the candidate rows of this frame, from the recorded cursor calls
            cands = np.zeros(gts.PP_GTS_MAX_CAND, gts.CAND_DTYPE)
            counts = np.zeros(gts.PP_GTS_MAX_ROUNDS, np.int32)
            s = 0
            for r, rd in enumerate(rounds):
                s0 = s
                for cname, num, idx in rd["cursor"]:
                    cands["object"][s:s + len(idx)] = db.base[cname] + idx
                    cands["group"][s:s + len(idx)] = classes.index(cname)
                    s += len(idx)
                cands["low"][s0:s0 + len(rd["low"])] = rd["low"]
                counts[r] = s - s0
            ids = np.array([db.class_ids[n] for n in names], np.int32)
            o_pts, o_boxes, o_cls, o_valid, info = gts.sample_all_np(frames[fkey], gt, ids, None, db, cands, counts, cfg,
                                                                     return_info=True)
            ok = all(robust(gt, db.boxes[cands["object"][sum(counts[:r]):sum(counts[:r + 1])]])
                     for r in range(len(rounds)) if counts[r])
            st = info["status"]
            has = {
                None: True, "none": counts.sum() == 0,
                "max": (st == gts.TOO_MANY_POINTS).any(), "empty": (st == gts.EMPTY_OBJECT).any(),
                "near_low": any(st[k] == gts.ACCEPTED and info["point_counts"][k] == 0 for k in range(s)),
            }
            n_all = int(counts[0])
            if want in ("later", "second_avoids_first"):
                cb = db.boxes[cands["object"][:n_all]]
                cc = aug.box_corners_2d(*(cb[:, k] for k in (0, 1, 3, 4, 6)))
                fc = aug.box_corners_2d(*(gt[:, k] for k in (0, 1, 3, 4, 6)))
                hf = aug.collide(cc[:, None], fc[None]).any(1)
                m = aug.collide(cc[:, None], cc[None])
                m[np.arange(n_all), np.arange(n_all)] = False
                grp = cands["group"][:n_all]
                surv = st[:n_all] != gts.BOX_COLLISION
                has["later"] = any(st[k] == gts.BOX_COLLISION and not hf[k] and not m[k, :k].any() and m[k, k + 1:].any()
                                   for k in range(n_all))
                has["second_avoids_first"] = any(
                    grp[k] == 1 and st[k] == gts.BOX_COLLISION and not hf[k] and not (m[k] & (grp == 1)).any()
                    and (m[k] & (grp == 0) & surv).any() for k in range(n_all))
            if ok and has[want]:
                break
        else:
            raise AssertionError(f"case {name}: no attempt showed {want!r}")
        # what the reference returned, against the restatement (the test repeats this from the stored data)
        last = rounds[-1]
        ret = last["ret"]
        for r, rd in enumerate(rounds):
            surv_slots = [k for k in range(sum(counts[:r]), sum(counts[:r + 1])) if st[k] != gts.BOX_COLLISION]
            assert np.array_equal(db.boxes[cands["object"][surv_slots]], rd["surv_boxes"]), (name, r)
            assert np.array_equal(info["point_counts"][surv_slots], rd["surv_counts"]), (name, r)
        if ret is None:
            assert len(info["accepted"]) == 0, name
            pasted, ret_boxes = np.zeros((0, 3), np.float32), np.zeros((0, 7))
        else:
            pasted, ret_boxes = ret["points"], ret["gt_boxes"]
            assert pasted.dtype == np.float32 and ret["gt_masks"].all()
            assert [db.class_ids[n] for n in ret["gt_names"]] == db.classes[info["accepted"]].tolist(), name
        assert np.array_equal(o_pts, np.concatenate([pasted, frames[fkey]], 0)), name
        assert np.array_equal(o_boxes, np.concatenate([gt, ret_boxes.reshape(-1, 7)], 0)), name
        pre = f"case__{name}__"
        out[pre + "frame"] = np.array(fkey)
        out[pre + "gt_boxes"], out[pre + "gt_classes"] = gt, ids
        out[pre + "cfg"] = np.array([max_pc, min_pc])
        out[pre + "sample_classes"], out[pre + "sample_max_nums"] = np.array(classes), np.array(nums)
        out[pre + "cands"], out[pre + "cand_counts"] = cands, counts
        out[pre + "pasted"], out[pre + "ret_boxes"] = pasted, ret_boxes.reshape(-1, 7)
        out[pre + "ret_classes"] = db.classes[info["accepted"]]
        out[pre + "accepted"] = info["accepted"]
        out[pre + "status"], out[pre + "point_counts"] = st, info["point_counts"]
        out[pre + "round_used"] = np.array(info["round_used"])
        out[pre + "surv_boxes"] = np.concatenate([rd["surv_boxes"] for rd in rounds], 0)
        out[pre + "surv_counts"] = np.concatenate([rd["surv_counts"] for rd in rounds], 0)
        cases.append(name)
        print(name, "attempt", attempt, "counts", counts.tolist(), "status", st[:counts.sum()].tolist(),
              "points", info["point_counts"][:counts.sum()].tolist(), "round", info["round_used"])
    # the cursor log since construction: (class, num, returned indices)
    log = _log["cursor"]
    out["cursor__class"] = np.array([c for c, _, _ in log])
    out["cursor__num"] = np.array([n for _, n, _ in log])
    out["cursor__offsets"] = np.concatenate([[0], np.cumsum([len(i) for _, _, i in log])])
    out["cursor__indices"] = np.concatenate([i for _, _, i in log])
    # the tail + reshuffle occurred: the twin, replaying the calls, must have reset its cursor at least once
    twin = gts.GtDatabase(infos, points, cfg2, np.random.RandomState(SEED), random.Random(SEED), 3)
    resets = 0
    for c, num, idx in log:
        before = twin.samplers[c].idx
        got = twin.samplers[c].sample(num)
        assert np.array_equal(got, idx), (c, num)
        resets += twin.samplers[c].idx == 0 and before + num >= len(twin.samplers[c].boxes)
    assert resets >= 1, "the cursor never wrapped"
    out["seed"] = np.array(SEED)
    out["reader_keys"] = np.array(sorted(k for k in READER if k.startswith("sampler_noise")))
    out["reader_values"] = np.array([np.atleast_1d(READER[k]).astype(np.float64).tolist() + [0.0] * (2 - np.size(READER[k]))
                                     for k in sorted(k for k in READER if k.startswith("sampler_noise"))])
    path = os.path.join(ROOT, "tests", "golden", "ref_gt_sample.npz")
    np.savez_compressed(path, names=np.array(cases), **out)
    print("cursor calls", len(log), "resets", int(resets), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
