"""The ledger of tests/backbone_ledger.py checked on the host alone (no GPU), through the planner probe
pp_plan_layer_name at 256 compute units (the MI355X):

  * every row's layer, in the layer table built from config.Derived the way pp_create builds it, plans to the row's
    instantiation -- the rows under a process-start switch in a child process started with it;
  * the rows claim exactly the set launch_layer can dispatch.  The set is generated here from the parameter lists of the
    with_value<...> calls, and those lists are read back out of csrc/backbone.hip: an instantiation added to launch_layer
    without a ledger row fails here;
  * both sides of every size heuristic (sep_k4_runs at 64 / 128 / 256 input channels, sep_k8_runs, deconv_k4_runs,
    sep_u_nt's 64 / 128 switch, ws_small_tile) are pinned, so a moved threshold fails here and not as a silently emptied
    GPU case;
  * the shapes are what the ledger says they are (frames of different sizes, a frame boundary inside a wave tile, SH
    widths and their twins, more tiles than resident workgroups in case `rounds`);
  * in the float64 restatement of the oracle, every layer a row names is alive: nonzero in at least a quarter of its
    output elements and in the first and last row and column of the map."""
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

import backbone_ledger as bl

BACKBONE = os.path.join(ROOT, "3d-object-detection-for-autonomous-navigation_amd", "csrc", "backbone.hip")
PLAN_HEADER = os.path.join(os.path.dirname(BACKBONE), "pp_plan.h")
HEADER = os.path.join(ROOT, "include", "pp_hip.h")


# ---- the dispatchable set, from the parameter lists of launch_layer's with_value calls ----
STRIDES = (1, 2)                  # with_value<1, 2>(p.s, ...): k_sep_k4, k_sep_u, k_gemm_ws MODE 0
TILES = (128, 64, 32)             # with_value<128, 64, 32>(p.nt, ...): k_sep_u, k_deconv_k4, k_deconv_u, k_gemm_ws, k_gemm_layer
DECONV_R_CIN = (256, 128, 64)     # with_value<256, 128, 64>(p.cin, ...): k_deconv_r
MODES = (0, 1)                    # with_value<0, 1>(p.mode, ...): k_gemm_layer
PIXEL_TILES = (64, 128)           # launch_ws: k_gemm_ws<..., 64> / <..., 128>


def _sep_u_wpc(nt, s, prec):
    """constexpr sep_u_wpc of backbone.hip: workgroups per CU, the third template argument of k_sep_u"""
    if s == 1:
        return (2 if nt == 128 else 3) if prec else (3 if nt == 128 else 4)
    return (2 if nt == 128 else 3) if prec else (2 if nt == 128 else (3 if nt == 64 else 4))


def dispatchable():
    out = []
    for s in STRIDES:
        out += [f"k_sep_k4<64,{s}>", f"k_sep_k4<64,{s},8>"]                                  # launch_k4<S>: k8 or not
        for nt in TILES:                                                                     # launch_u<NT, S>
            out += [f"k_sep_u<{nt},{s},{_sep_u_wpc(nt, s, 0)},0,0>",                           # PREC 0
                    f"k_sep_u<{nt},{s},{_sep_u_wpc(nt, s, 1)},1,0>",                           # PREC 1
                    f"k_sep_u<{nt},{s},{_sep_u_wpc(nt, s, 1)},1,1>"]                           # PREC 1, OCC 1
            out += [f"k_gemm_ws<{nt},0,{s},{p}>" for p in PIXEL_TILES]                         # launch_ws<NT, 0, S>
    out += ["k_sep_u<64,1,3,1,0,0,1>"]                                                       # launch_u: SH, S == 1 && NT == 64 only
    out += ["k_sep_p<256>", "k_sep_p<256,1>"]                                                # launch_p
    for nt in TILES:
        out += [f"k_deconv_k4<{nt}>", f"k_deconv_u<{nt},3>"]
        out += [f"k_gemm_ws<{nt},1,1,{p}>" for p in PIXEL_TILES]                               # launch_ws<NT, 1, 1>
        out += [f"k_gemm_layer<{nt},{m}>" for m in MODES]
    out += [f"k_deconv_r<{c}>" for c in DECONV_R_CIN]
    return out


def test_the_parameter_lists_are_those_of_launch_layer():
    """The lists above, read back out of the source: launch_layer's switch statement, case by case."""
    with open(BACKBONE) as f:
        src = f.read()
    body = src[src.index("int launch_layer(const LayerDesc& L"):]
    body = body[body.index("switch (p.kernel) {"):]
    cases = {m.group(1): m.group(2) for m in re.finditer(r"case LayerKernel::(\w+):(.*?)break;", body, re.S)}
    assert sorted(cases) == sorted(["SEP_K4", "SEP_P", "SEP_U", "DECONV_K4", "DECONV_R", "DECONV_U", "GEMM_WS", "GEMM_LAYER"])
    lists = {k: [tuple(int(x) for x in m.split(",")) for m in re.findall(r"with_value<([\d, ]+)>", v)] for k, v in cases.items()}
    assert lists == {"SEP_K4": [STRIDES], "SEP_P": [], "SEP_U": [STRIDES, TILES], "DECONV_K4": [TILES], "DECONV_R": [DECONV_R_CIN],
                     "DECONV_U": [TILES], "GEMM_WS": [STRIDES, TILES, TILES], "GEMM_LAYER": [MODES, TILES]}, lists
    # the launchers' own branches: the eight-way split, SH of k_sep_p and of the one k_sep_u instantiation, OCC, the pixel tiles
    assert src.count("(k_sep_k4<64, S, 8>)") == 1 and src.count("(k_sep_k4<64, S>)") == 1
    assert src.count("(k_sep_p<256, 1>)") == 1 and src.count("k_sep_p<256>,") == 1
    assert "if constexpr (S == 1 && NT == 64) {" in src and src.count("(k_sep_u<NT, S, WPB, 1, 0, 0, 1>)") == 1
    assert src.count("(k_sep_u<NT, S, WPB, 1, 1>)") == 1 and src.count("(k_sep_u<NT, S, WPB, 1>)") == 1
    assert src.count("(k_sep_u<NT, S, WPS, 0>)") == 1
    assert src.count("(k_gemm_ws<NT, MODE, S, 64>)") == 1 and src.count("(k_gemm_ws<NT, MODE, S, 128>)") == 1
    assert src.count("(k_deconv_u<NT, WPS>)") == 1 and "constexpr int WPS = 3;" in src
    with open(PLAN_HEADER) as f:          # the workgroups per CU: the planner's header, which backbone.hip includes
        plan_src = f.read()
    assert '#include "pp_plan.h"' in src and "sep_u_wpc(int" not in src
    m = re.search(r"constexpr int sep_u_wpc\(int nt, int s, bool prec\) \{\s*return (.*?);\s*\}", plan_src, re.S)
    assert " ".join(m.group(1).split()) == ("s == 1 ? (prec ? (nt == 128 ? SEP128_WPB : (nt == 64 ? SEP64_WPB : 3)) : (nt == 128 ? 3 : 4)) "
                                            ": (prec ? (nt == 128 ? 2 : 3) : (nt == 128 ? 2 : (nt == 64 ? 3 : 4)))")
    assert "constexpr int SEP128_WPB = 2, SEP64_WPB = 3;" in plan_src


def test_the_ledger_claims_exactly_the_dispatchable_set():
    full = dispatchable()
    assert len(full) == len(set(full)) == 58
    claimed = {r.inst for r in bl.ROWS}
    assert claimed == set(full), (sorted(set(full) - claimed), sorted(claimed - set(full)))
    plain = [r.inst for r in bl.ROWS if r.variant == ""]
    assert sorted(plain) == sorted(full), "one row with an empty variant per instantiation"
    # the runtime branches the tags do not show
    variants = {(r.inst.split("<")[0], r.variant) for r in bl.ROWS if r.variant}
    assert ("k_sep_k4", "cell-map lookup (a.occ)") in variants
    for fam in ("k_deconv_k4", "k_deconv_r", "k_deconv_u"):
        text = " ".join(v for f, v in variants if f == fam)
        for need in ("head_mode 0", "head_mode 1", "head_mode 2", "class plane", "k = 2", "k = 4") + (() if fam == "k_deconv_r" else ("k = 1",)):
            assert need in text, (fam, need)
    for r in bl.ROWS:
        assert r.case in bl.BY_NAME and r.prec in ("split", "f32"), r
        assert r.prec == "split" or not bl.BY_NAME[r.case].env, "the float32 runs share their engine: no child"


@pytest.fixture(scope="module")
def plans(hip_lib):
    """{case: {prec: {layer: instantiation}}} at 256 CUs: this process for the cases without a switch, one child per switch
    set for the others (the switches are read once per process; the child touches no device)."""
    out = {}
    for i, env in enumerate(bl.ENVS):
        if not env:
            out.update(bl.plans_of_env(env))
            continue
        assert not any(k in os.environ for k, _ in env), "the suite runs without the backbone's switches"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "backbone_ledger.py"), str(i)], cwd=ROOT,
                           env=dict(os.environ, **dict(env), PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")])),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    return out


def test_every_row_plans_to_its_instantiation(plans):
    for v in ("PP_SEP_K4", "PP_DECONV_K4", "PP_SEP_KERNEL", "PP_SEP_NT", "PP_GEMM_PREC", "PP_DENSE_CANVAS", "PP_NO_HEAD_FUSION"):
        assert v not in os.environ, v
    for r in bl.ROWS:
        assert plans[r.case][r.prec][r.layer] == r.inst, (r, plans[r.case][r.prec])


def test_the_variants_are_what_the_rows_say():
    for r in bl.ROWS:
        L = dict(bl.layer_table(bl.BY_NAME[r.case], r.prec))[r.layer]
        for k in (1, 2, 4):
            if f"k = {k}" in r.variant:
                assert L["k"] == k, r
        for hm in (0, 1, 2):
            if f"head_mode {hm}" in r.variant:
                assert L["head_mode"] == hm, r
        if "class plane" in r.variant:      # the last transposed convolution of a fused engine (layer_writes_cls_plane)
            assert r.layer == "deconv3" and L["head_mode"] == 2 and r.inst.startswith("k_deconv_"), r
        if "cell-map" in r.variant or r.inst.endswith(",1,1>"):
            assert L["sparse_input"] == 1 and r.layer == "block1.0", r
        if r.variant == "the heads layer":
            assert L["kind"] == "head", r
        if "two column tiles" in r.variant:
            assert L["cout"] == 256, r


def _pixels(L, batch):
    return batch * (L["out_h"] * L["out_w"] if L["kind"] == "sep" else L["in_h"] * L["in_w"])


def test_the_shapes_are_what_the_ledger_says():
    for c in bl.CASES:
        sizes = [len(f) for f in bl.frames(c)]
        assert c.batch >= 2 and len(set(sizes[:2])) == 2 and c.batch <= c.max_batch, c.name
    tables = {c.name: dict(bl.layer_table(c)) for c in bl.CASES}
    # a frame boundary inside a wave tile and a half-filled last tile, in a layer a row names, on every family of kernels
    for fam in ("k_sep_k4", "k_sep_p", "k_sep_u", "k_deconv_k4", "k_deconv_r", "k_deconv_u", "k_gemm_ws", "k_gemm_layer"):
        ok = [r for r in bl.ROWS if r.inst.startswith(fam + "<")
              and _pixels(tables[r.case][r.layer], 1) % 32 != 0 and _pixels(tables[r.case][r.layer], bl.BY_NAME[r.case].batch) % 128 != 0]
        assert ok, fam
    # stride 2: even maps (pp_create refuses the odd ones, see the ledger's docstring)
    for r in bl.ROWS:
        L = tables[r.case][r.layer]
        if L["kind"] == "sep" and L["stride"] == 2:
            assert L["in_w"] % 2 == 0 and L["in_h"] % 2 == 0 and L["out_w"] % 2 == 0, r
    # SH rows on widths that are multiples of 8 with equal maps; their twins on widths that are not
    for r in bl.ROWS:
        L = tables[r.case][r.layer]
        if r.inst in ("k_sep_u<64,1,3,1,0,0,1>", "k_sep_p<256,1>"):
            assert L["out_w"] % 8 == 0 and (L["in_w"], L["in_h"]) == (L["out_w"], L["out_h"]) and L["stride"] == 1, r
        if r.inst in ("k_sep_u<64,1,3,1,0>", "k_sep_p<256>"):
            assert L["out_w"] % 8 != 0 and L["stride"] == 1, r
    # case `rounds`: more 128-pixel tiles (units of k_deconv_r: tiles x taps) than resident workgroups, and no multiple
    slots = {"k_sep_u<64,1,3,1,0,0,1>": bl.CUS * 3, "k_sep_u<128,1,2,1,0>": bl.CUS * 2, "k_sep_u<128,2,2,1,0>": bl.CUS * 2,
             "k_sep_p<256,1>": bl.CUS, "k_deconv_u<128,3>": bl.CUS * 3, "k_deconv_r<128>": bl.CUS * 2, "k_deconv_r<256>": bl.CUS * 2}
    seen = set()
    for r in bl.ROWS:
        if r.case != "rounds":
            continue
        L = tables["rounds"][r.layer]
        tiles = -(-_pixels(L, bl.BY_NAME["rounds"].batch) // 128)
        work = tiles * L["k"] * L["k"] if r.inst.startswith("k_deconv_r") else tiles
        assert L["n_total"] // L["cout"] in (1, 4) and work > slots[r.inst] and work % slots[r.inst] != 0, (r, work)
        seen.add(r.inst)
    assert seen == set(slots)


# ---- both sides of every size heuristic, at 256 compute units ----
def _sep(cin, cout, w, h, stride=1, pieces=1):
    return dict(kind="sep", cin=cin, cout=cout, n_total=cout, stride=stride, in_h=h * stride, in_w=w * stride, out_h=h, out_w=w,
                has_wt16=pieces)


def _deconv(cin, cout, w, h, k=1, pieces=1):
    return dict(kind="deconv", cin=cin, cout=cout, n_total=k * k * cout, k=k, in_h=h, in_w=w, out_h=h * k, out_w=w * k,
                head_mode=1, has_wt16=pieces, has_head_wt16=pieces)


NEIGHBOURS = [
    # sep_k4_runs: 2 * ceil(M / 32) * (n_total / 64) <= 3 / 5 / 6 * CUs at 64 / 128 / 256 input channels
    ("sep_k4_runs cin 64", _sep(64, 64, 128, 96), 1, "k_sep_k4<64,1>"),                    # 12288 pixels: 384 wave tiles
    ("sep_k4_runs cin 64", _sep(64, 64, 110, 112), 1, "k_sep_u<64,1,3,1,0>"),              # 12320: 385
    ("sep_k4_runs cin 128", _sep(128, 64, 128, 160), 1, "k_sep_k4<64,1>"),                 # 20480: 640
    ("sep_k4_runs cin 128", _sep(128, 64, 32, 641), 1, "k_sep_u<64,1,3,1,0,0,1>"),         # 20512: 641
    ("sep_k4_runs cin 256", _sep(256, 64, 128, 192), 1, "k_sep_k4<64,1>"),                 # 24576: 768 (and past sep_k8_runs)
    ("sep_k4_runs cin 256", _sep(256, 64, 32, 769), 1, "k_sep_u<64,1,3,1,0,0,1>"),         # 24608: 769
    # sep_k8_runs: ceil(M / 32) * (n_total / 64) <= CUs
    ("sep_k8_runs", _sep(256, 64, 128, 64), 1, "k_sep_k4<64,1,8>"),                        # 8192: 256
    ("sep_k8_runs", _sep(256, 64, 32, 257), 1, "k_sep_k4<64,1>"),                          # 8224: 257
    ("sep_k8_runs stride 2", _sep(256, 64, 128, 64, stride=2), 1, "k_sep_k4<64,2,8>"),
    ("sep_k8_runs stride 2", _sep(256, 64, 32, 257, stride=2), 1, "k_sep_k4<64,2>"),
    # deconv_k4_runs: 2 * ceil(M / 32) * (n_total / NT) <= 3 * CUs
    ("deconv_k4_runs", _deconv(64, 64, 128, 96), 1, "k_deconv_k4<64>"),                    # 384
    ("deconv_k4_runs", _deconv(64, 64, 110, 112), 1, "k_deconv_u<64,3>"),                  # 385
    ("deconv_k4_runs k 2", _deconv(128, 128, 128, 24, k=2), 1, "k_deconv_k4<128>"),        # 96 wave tiles x 4 taps
    ("deconv_k4_runs k 2", _deconv(128, 128, 4, 776, k=2), 1, "k_deconv_r<128>"),          # 97 x 4
    # sep_u_nt without float16 pieces: 64-channel tiles while 2 * ceil(rows / 32) * (cout / 128) < 20 * CUs
    ("sep_u_nt", _sep(128, 128, 32, 2559, pieces=0), 1, "k_sep_u<64,1,4,0,0>"),            # 2559 waves
    ("sep_u_nt", _sep(128, 128, 128, 640, pieces=0), 1, "k_sep_u<128,1,3,0,0>"),           # 2560
    ("sep_u_nt 256 channels", _sep(128, 256, 2, 20464, pieces=0), 1, "k_sep_u<64,1,4,0,0>"),      # 1279 x 2
    ("sep_u_nt 256 channels", _sep(128, 256, 128, 320, pieces=0), 1, "k_sep_u<128,1,3,0,0>"),     # 1280 x 2
    # ws_small_tile: ceil(M / 128) * (n_total / NT) < 256 -> 64-pixel tiles
    ("ws_small_tile", _deconv(64, 128, 128, 255, pieces=0), 1, "k_gemm_ws<128,1,1,64>"),   # 255 tiles
    ("ws_small_tile", _deconv(64, 128, 4, 8161, pieces=0), 1, "k_gemm_ws<128,1,1,128>"),   # 32644 pixels: 256
    ("ws_small_tile k 2", _deconv(64, 64, 4, 2016, k=2, pieces=0), 1, "k_gemm_ws<64,1,1,64>"),    # 63 tiles x 4
    ("ws_small_tile k 2", _deconv(64, 64, 4, 2017, k=2, pieces=0), 1, "k_gemm_ws<64,1,1,128>"),   # 64 x 4
]


@pytest.mark.parametrize("i", range(0, len(NEIGHBOURS), 2), ids=[NEIGHBOURS[i][0] for i in range(0, len(NEIGHBOURS), 2)])
def test_threshold_neighbours(pp, hip_lib, i):
    for what, layer, batch, want in NEIGHBOURS[i:i + 2]:
        assert pp.planner.plan_layer_name(layer, batch, bl.CUS) == want, (what, layer)


def test_the_probe_weighs_the_compute_units_it_is_given(pp, hip_lib):
    """Half the chip: the crossovers halve.  And the batch multiplies the pixels."""
    L = _sep(64, 64, 128, 48)                    # 6144 pixels: 192 wave tiles
    assert pp.planner.plan_layer_name(L, 1, 128) == "k_sep_k4<64,1>" == pp.planner.plan_layer_name(L, 2, 256)
    assert pp.planner.plan_layer_name(_sep(64, 64, 110, 56), 1, 128) == "k_sep_u<64,1,3,1,0>"      # 6160: 193
    assert pp.planner.plan_layer_name(L, 3, 256) == "k_sep_u<64,1,3,1,0,0,1>"
    assert pp.planner.plan_layer_name(L, 1, 304) == "k_sep_k4<64,1>"
    with pytest.raises(ValueError):
        pp.planner.plan_layer_name(L, 0, 256)
    with pytest.raises(ValueError):
        pp.planner.plan_layer_name(L, 1, 0)


def test_the_probe_is_exported_the_way_the_other_entry_points_are(pp, hip_lib):
    with open(HEADER) as f:
        hdr = f.read()
    assert "#define PP_ABI_VERSION 4" in hdr and hip_lib.pp_abi_version() == 4
    later = hdr[hdr.index("later additions within 4"):hdr.index("#define PP_ABI_VERSION")]
    for name in ("pp_layer_plan_desc", "pp_plan_layer_name"):
        assert name in later, name
    fields = re.search(r"typedef struct pp_layer_plan_desc \{(.*?)\} pp_layer_plan_desc;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip() for line in fields.split(";") if line.strip() for n in line.replace("int32_t", "").split(",")]
    assert names == [n for n, _ in pp._lib.PPLayerPlanDesc._fields_]
    assert "pp_plan_layer_name" in pp._lib.EXPORTS
    assert bl.tag_of("k_sep_u<64,1,3,1,0,0,1>") == "k_sep_u<64,1,3,1,0>" and bl.tag_of("k_sep_p<256,1>") == "k_sep_p" == bl.tag_of("k_sep_p<256>")
    assert bl.tag_of("k_sep_k4<64,1,8>") == "k_sep_k4<64,1,8>"


@pytest.mark.parametrize("name", [c.name for c in bl.CASES if not c.env])
def test_the_oracles_maps_are_alive_in_every_named_layer(name):
    """The cap on the inputs: a case proves nothing about a layer whose output is mostly dead.  (The cases under a switch
    share the oracle of the case they are named after.)"""
    case = bl.BY_NAME[name]
    named = {r.layer for r in bl.ROWS if bl.base(bl.BY_NAME[r.case]).name == name}
    assert named, "a case no row names"
    ref = bl.reference(case)
    act = bl.layer_activity(case, ref["w"], ref["canvas"])
    for layer in sorted(named):
        share, edges = act[layer]
        print(f"{name} {layer}: {share:.2f} of the output elements nonzero, borders {'alive' if edges else 'DEAD'}")
        assert share >= 0.25 and edges, (name, layer, share, edges)
