"""The ledger of tests/backbone_ledger.py on the GPU (`-m gpu`): every template instantiation launch_layer can dispatch,
and every runtime branch inside one that the layer tag does not show, run once and held against the oracle.

Per case: an engine with seeded init_weights, the oracle's padded voxels of the seeded clouds through forward_voxels, then
  * Engine.layer_tags() == the planner probe's answers for the DEVICE's compute-unit count (device_info), modulo the SH
    argument the tags leave out -- so the claimed kernel really ran, on a part with another CU count too -- and, on a
    256-CU part, the ledger's rows themselves;
  * box_preds, cls_preds, dir_cls_preds against util_ref's oracle at the suite's bar, atol = 1e-4, rtol = 0 (TOL of
    test_gpu_parity.py);
  * the cases with float32 rows a second time after set_gemm_precision("f32") on the same engine (PREC = 0, k_gemm_ws /
    k_gemm_layer for the transposed convolutions), the same bar, and the split-float16 / float32 difference printed;
  * the cases with a class-plane row through `detect` as well: the compact class-logit plane is read by the post-process
    only, so the number of detections, their scores and labels are held against the reference's predict().
The cases under a process-start switch (PP_SEP_KERNEL=ws) run in ONE child process per switch set (this file as a
script, a fresh subprocess), which leaves every case's head maps, tags and the probe's answers under the switch in an
.npz; the child, and every case inside it and inside the in-process tests, runs under a time limit of its own.

Measured on the MI355X (256 CUs): largest |head map - oracle| over the three maps, with float16 pieces and -- the cases
with float32 rows -- after set_gemm_precision("f32"), and the largest difference between the two runs.  These are
measurements; the bar is the suite's 1e-4 and does not move.  Every tag equals the probe's answer, every row's kernel ran.

  case          B   largest |head|  split      float32    |split - float32|
  k4             3    1.20        8.34e-07   5.96e-07   7.15e-07
  k4occ          2    3.67        2.26e-06      -          -
  occ128s1       5    6.23        3.81e-06   3.10e-06   4.77e-06
  occ64s1        2    4.24        3.10e-06      -          -
  occ32s1        2    3.66        2.38e-06   2.38e-06   1.91e-06
  occ128s2       4    4.34        3.10e-06      -          -
  occ64s2        4    3.53        3.70e-06      -          -
  occ32s2        4    4.76        2.38e-06      -          -
  rounds        90    1.93        2.03e-06      -          -
  generic        3    1.44        9.54e-07   9.54e-07   7.15e-07
  unfused        9    1.23        1.49e-06      -          -
  twins         16    1.78        1.91e-06      -          -
  wsmall         3    2.43        1.07e-06   9.54e-07   8.34e-07
  ws-k4          3    1.20        7.60e-07      -          -
  ws-occ128s1    5    6.23        3.81e-06      -          -
  ws-occ64s1     2    4.24        3.58e-06      -          -
  ws-occ32s1     2    3.66        2.38e-06      -          -
  ws-occ64s2     4    3.53        2.86e-06      -          -
  ws-occ32s2     4    4.76        2.38e-06      -          -
  ws-wsmall      3    2.43        1.07e-06      -          -

  k4, occ32s1, twins through `detect`: 30, 100 and 359 detections, counts, scores and labels as the reference's predict().
  The whole file: 21 tests in 18.9 s (11.6 s of them the first test: library and device start-up), the child under
  PP_SEP_KERNEL=ws with its seven engines included.

What the cases found: no kernel computed a wrong value, no instantiation faulted; the two never-run suspects
(k_sep_k4<64,2,8>: k4's block3.0; k_sep_k4 with the cell-map lookup: k4occ's block1.0) included.
"""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):          # (as a script, the child, nothing else puts them there)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import backbone_ledger as bl  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4                        # test_gpu_parity.TOL (asserted equal below)
HEADS = ("box_preds", "cls_preds", "dir_cls_preds")
NMAX = 16384                      # max_points_per_frame of the engines
STEP_LIMIT = 120                  # seconds for one case's GPU work (a hung kernel ends the process, with a traceback)
CHILD_LIMIT = 600


def _heads(out):
    return {k: np.asarray(out[k], np.float32) for k in HEADS}


def _run(pp, case):
    """One case on the device: {"cus", "tags_split", "plan_split", "split_<head>", [the same for f32], ["dets", "n"]}."""
    d, w, frames, ex = bl.example(case)
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True, file=sys.__stderr__)
    try:
        eng = pp.Engine(bl.config(case), max_batch=case.max_batch, max_points_per_frame=NMAX)
        try:
            eng.load_weights(w)
            cus = eng.device_info()["compute_units"]
            res = {"cus": np.int32(cus)}
            precs = ("split", "f32") if case.name in bl.F32_CASES else ("split",)
            for prec in precs:
                if prec == "f32":
                    eng.set_gemm_precision("f32")
                out = eng.forward_voxels(ex[0], ex[1], ex[2], case.batch)
                res["tags_" + prec] = np.array(eng.layer_tags())
                plan = bl.plan(case, prec, cus)
                res["plan_" + prec] = np.array([f"{bl.tag_of(plan[n])}:{n}" for n, _ in bl.layer_table(case, prec)])
                res["full_" + prec] = np.array([f"{plan[n]}:{n}" for n, _ in bl.layer_table(case, prec)])
                for k, v in _heads(out).items():
                    res[f"{prec}_{k}"] = v
                if prec == "split" and case.name in bl.CLS_PLANE_CASES:
                    rect, trv, _ = pp.synth.default_calib()
                    dets, n = eng.detect(frames, np.stack([rect] * case.batch), np.stack([trv] * case.batch))
                    res["det_n"], res["det_score"], res["det_label"] = n.copy(), dets["score"].copy(), dets["label"].copy()
                    assert eng.layer_tags() == [str(t) for t in res["tags_split"]], "detect and forward_voxels plan alike"
        finally:
            eng.close()
    finally:
        faulthandler.cancel_dump_traceback_later()
    return res


def _check(case, res):
    ref = bl.reference(case, dets=case.name in bl.CLS_PLANE_CASES)
    cus = int(res["cus"])
    worst = {}
    for prec in ("split", "f32"):
        if "tags_" + prec not in res:
            continue
        tags = [str(t) for t in res["tags_" + prec]]
        assert tags == [str(t) for t in res["plan_" + prec]], (case.name, prec, cus)
        full = dict(reversed(str(t).split(":")) for t in res["full_" + prec])
        for r in bl.ROWS:
            if r.case == case.name and r.prec == prec:
                if cus == bl.CUS:
                    assert full[r.layer] == r.inst, (r, full)
                assert f"{bl.tag_of(full[r.layer])}:{r.layer}" in tags, (r, tags)
        for k in HEADS:
            got, want = res[f"{prec}_{k}"], np.asarray(ref["preds"][k], np.float32)
            assert got.shape == want.shape, (case.name, prec, k)
            worst[prec] = max(worst.get(prec, 0.0), float(np.abs(got - want).max()))
    line = f"{case.name}: {cus} CUs, B = {case.batch}, largest |head map - oracle| split {worst['split']:.2e}"
    if "f32" in worst:
        diff = max(float(np.abs(res[f"split_{k}"] - res[f"f32_{k}"]).max()) for k in HEADS)
        line += f", f32 {worst['f32']:.2e}, largest |split - f32| {diff:.2e}"
    print(line + f" (bar {TOL:.0e}); largest |oracle head map| {max(float(np.abs(v).max()) for v in ref['preds'].values()):.2f}")
    for prec in worst:
        for k in HEADS:
            np.testing.assert_allclose(res[f"{prec}_{k}"], np.asarray(ref["preds"][k], np.float32), rtol=0, atol=TOL,
                                       err_msg=f"{case.name} {prec} {k}")
    if "det_n" in res:
        kept = 0
        for b, r in enumerate(ref["dets"]):
            k = 0 if r["scores"] is None else len(r["scores"])
            assert int(res["det_n"][b]) == k, (case.name, b, int(res["det_n"][b]), k)
            if k:
                np.testing.assert_allclose(res["det_score"][b, :k], r["scores"], rtol=0, atol=TOL)
                assert np.array_equal(res["det_label"][b, :k], r["label_preds"]), (case.name, b)
            kept += k
        assert kept > 0, "the class plane has to decide something"
        print(f"{case.name}: {kept} detections through the class plane, scores and labels as the reference's predict()")


def test_the_bar_is_the_suites():
    import test_gpu_parity
    assert TOL == test_gpu_parity.TOL


def _names(env):
    return [c.name for c in bl.CASES if c.env == env]


@pytest.mark.parametrize("name", _names(()))
def test_ledger_case_against_the_oracle(pp, hip_lib, name):
    for v in ("PP_SEP_K4", "PP_DECONV_K4", "PP_SEP_KERNEL", "PP_SEP_NT", "PP_GEMM_PREC", "PP_DENSE_CANVAS", "PP_NO_HEAD_FUSION"):
        assert v not in os.environ, v
    case = bl.BY_NAME[name]
    _check(case, _run(pp, case))


@pytest.fixture(scope="module")
def children(hip_lib, tmp_path_factory):
    """{switch set: the child's .npz as a dict}: one child per switch set, started on first use."""
    done = {}

    def get(env):
        if env not in done:
            path = str(tmp_path_factory.mktemp("ledger") / "out.npz")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), str(bl.ENVS.index(env)), path], cwd=ROOT,
                               env=dict(os.environ, **dict(env)), capture_output=True, text=True, timeout=CHILD_LIMIT)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            with np.load(path) as z:
                done[env] = {k: z[k] for k in z.files}
        return done[env]
    return get


@pytest.mark.parametrize("name", [n for env in bl.ENVS if env for n in _names(env)])
def test_ledger_case_under_a_switch_against_the_oracle(children, name):
    case = bl.BY_NAME[name]
    got = children(case.env)
    pre = name + "/"
    _check(case, {k[len(pre):]: v for k, v in got.items() if k.startswith(pre)})


if __name__ == "__main__":          # the child: <index into ENVS> <out.npz>, started with that switch set
    import pp_amd
    env = bl.ENVS[int(sys.argv[1])]
    assert env and all(os.environ.get(k) == v for k, v in env), env
    out = {}
    for c in bl.CASES:
        if c.env == env:
            out.update({f"{c.name}/{k}": v for k, v in _run(pp_amd, c).items()})
    np.savez(sys.argv[2], **out)
