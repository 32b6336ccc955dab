"""Ledger of the backbone's kernel dispatch: every template instantiation csrc/backbone.hip's launch_layer can pick, and
every runtime variant inside one that the layer tag does not show, with the case that runs it.  Shared by
tests/test_backbone_ledger_host.py (no device: the planner probe pp_plan_layer_name says every row's layer plans to the
row's instantiation; the rows cover the whole dispatchable set; the oracle's activations of every named layer are alive)
and tests/test_gpu_backbone_ledger.py (the cases on the GPU against the oracle, layer tags against the probe).

A case is pedestrian_d435i_config edited the way tests/grid_shape_cases.py edits it: 0.08 m cells, one z cell, x from 0,
y centred.  CASES holds the shapes, ROWS the claims.  Nothing here is drawn at run time except the seeded clouds.

Shapes (what the sizes are chosen for; test_backbone_ledger_host.py asserts the arithmetic):
  * every case has at least two frames with clouds of different sizes; every kernel family has a row whose layer has
    frames of a pixel count that is no multiple of 32 (a frame boundary inside a wave tile) and a total that is no
    multiple of 128 (a half-filled last tile);
  * stride 2 reads even maps only: an odd map under a stride-2 layer gives ceil(n / 2) columns, which no transposed
    convolution (kernel == stride) brings back to the head map, so pp_create refuses every such config
    (PP_ERR_SHAPE) -- the "odd input" stride-2 shape does not exist among accepted configs.  What exists is an odd
    map at stride 1 (21 columns), which takes k_gemm_layer; case `generic` runs it;
  * SH rows: stride-1 maps 24 / 48 / 128 columns wide; their twins (case `twins`) 44 and 22 columns wide;
  * persistent kernels past one round: case `rounds` (B = 90) has more tiles than resident workgroup slots in
    k_sep_u<64,1,3,1,0>+SH, k_sep_u<128,1,2,1,0>, k_sep_u<128,2,2,1,0>, k_sep_p, k_deconv_u<128,3> and more units than
    slots in k_deconv_r<128> / <256>, none a multiple of the slots.
"""
import collections
import copy

import numpy as np

import pp_amd as pp

CELL = 0.08
Z_RANGE = (-3.0, 1.0)
CUS = 256                         # the MI355X; PlanEnv's default

Case = collections.namedtuple(
    "Case", "name nx ny strides up0 layer_nums pfn filters ups batch max_batch max_voxels points seed env")
# strides: layer_strides; up0: upsample_strides[0] (1 or strides[0]; the others follow: every branch ends on the head map)
# points: rows of frame b are points[b % len(points)] + 7 * b (different sizes); env: the process-start switches of the case
# (a non-empty env runs in a child process); seed: of the clouds and of init_weights, chosen so that the oracle's maps are
# alive (see activity)


WS = (("PP_SEP_KERNEL", "ws"),)        # the producer / consumer kernel for every separable layer
#     name        nx   ny  strides   up0 layer_nums pfn  filters          ups              B  maxB max_vox points              seed env
CASES = [
    # small maps, float16 pieces: the split-K kernels (three frames; 576 / 144 / 36 pixels a frame)
    Case("k4", 24, 24, (1, 2, 2), 1, (1, 1, 1), 128, (64, 256, 256), (128, 64, 32), 3, 3, 576, (700, 300, 500), 1, ()),
    # the smallest sparse canvas (32768 cells), first stride 2, 128 input channels: two frames stay under the split-K limit
    Case("k4occ", 256, 128, (2, 2, 2), 1, (1, 1, 1), 128, (64, 64, 64), (64, 64, 64), 2, 2, 8192, (12000, 5000), 1, ()),
    # sparse canvases whose first layer is too large (or too narrow: 32 input channels) for split-K: OCC = 1 per NT, S
    Case("occ128s1", 256, 128, (1, 2, 2), 1, (1, 1, 1), 32, (128, 256, 64), (128, 64, 32), 5, 5, 8192, (12000, 5000, 8000), 1, ()),
    Case("occ64s1", 256, 128, (1, 2, 2), 1, (1, 1, 1), 32, (64, 128, 64), (64, 64, 64), 2, 2, 8192, (12000, 5000), 1, ()),
    Case("occ32s1", 256, 128, (1, 2, 2), 1, (1, 1, 1), 32, (32, 32, 64), (32, 32, 32), 2, 2, 8192, (12000, 5000), 1, ()),
    Case("occ128s2", 256, 128, (2, 2, 2), 2, (1, 1, 1), 32, (128, 64, 64), (128, 128, 128), 4, 4, 8192, (12000, 5000), 1, ()),
    Case("occ64s2", 256, 128, (2, 2, 2), 2, (1, 1, 1), 32, (64, 64, 64), (64, 64, 64), 4, 4, 8192, (12000, 5000), 1, ()),
    Case("occ32s2", 256, 128, (2, 2, 2), 2, (1, 1, 1), 32, (32, 64, 64), (32, 32, 32), 4, 4, 8192, (12000, 5000), 1, ()),
    # the persistent kernels past one round of their resident workgroups (90 frames of 48 x 62 and 24 x 31 pixels)
    Case("rounds", 48, 62, (1, 2, 1), 1, (1, 1, 1), 64, (64, 128, 256), (128, 128, 128), 90, 90, 2976, (900, 400, 650), 1, ()),
    # 21 columns: no kernel with a pixel-pair producer takes the map, the heads run as a layer of their own
    Case("generic", 21, 10, (1, 1, 1), 1, (1, 1, 1), 32, (32, 64, 128), (128, 64, 32), 3, 3, 210, (500, 200, 350), 1, ()),
    # a 256-channel upsample branch: heads not fused (head_mode 0), maps too large for the split-K deconv
    Case("unfused", 40, 36, (1, 2, 2), 1, (1, 1, 1), 64, (64, 128, 128), (128, 128, 256), 9, 9, 1440, (2500, 900, 1500), 1, ()),
    # 44 / 22 columns: the twins of the SH instantiations
    Case("twins", 44, 36, (1, 2, 1), 1, (1, 1, 1), 64, (64, 128, 256), (128, 128, 128), 16, 16, 1584, (2500, 900, 1500), 1, ()),
    # narrow layers at both strides on small maps
    Case("wsmall", 48, 32, (2, 2, 2), 2, (1, 1, 1), 32, (32, 64, 128), (32, 32, 32), 3, 3, 1536, (2500, 900, 1500), 1, ()),
]
# the same shapes with every separable layer on k_gemm_ws (PP_SEP_KERNEL=ws; the canvases are dense there)
CASES += [c._replace(name="ws-" + c.name, env=WS) for c in CASES if c.name in ("k4", "wsmall", "occ128s1", "occ64s1", "occ32s1", "occ64s2", "occ32s2")]
BY_NAME = {c.name: c for c in CASES}
ENVS = sorted({c.env for c in CASES})


Row = collections.namedtuple("Row", "inst variant case prec layer")
# inst: the full instantiation name (pp_plan_layer_name); variant: "" for the instantiation itself, else the runtime branch
# inside it that the row is about; prec: "split" (float16 pieces) or "f32" (after set_gemm_precision("f32") on the same
# engine); layer: the layer of the case that runs it.
ROWS = [
    # ---- k_sep_k4<64, S[, 8]> ----
    Row("k_sep_k4<64,1>", "", "k4", "split", "block1.0"),
    Row("k_sep_k4<64,1,8>", "", "k4", "split", "block2.1"),
    Row("k_sep_k4<64,2>", "", "k4", "split", "block2.0"),
    Row("k_sep_k4<64,2,8>", "", "k4", "split", "block3.0"),               # a stride-2 layer with 256 input channels
    Row("k_sep_k4<64,2>", "cell-map lookup (a.occ)", "k4occ", "split", "block1.0"),
    # ---- k_sep_p<256[, SH]> ----
    Row("k_sep_p<256>", "", "twins", "split", "block3.1"),
    Row("k_sep_p<256,1>", "", "occ128s1", "split", "block2.1"),
    Row("k_sep_p<256,1>", "tiles > slots", "rounds", "split", "block3.0"),
    # ---- k_sep_u<NT, S, WPS, PREC[, OCC][, 0, SH]> ----
    Row("k_sep_u<128,1,2,1,0>", "", "occ64s1", "split", "block2.1"),
    Row("k_sep_u<64,1,3,1,0>", "", "twins", "split", "block1.1"),
    Row("k_sep_u<32,1,3,1,0>", "", "occ32s1", "split", "block1.1"),
    Row("k_sep_u<128,2,2,1,0>", "", "twins", "split", "block2.0"),
    Row("k_sep_u<64,2,3,1,0>", "", "wsmall", "split", "block2.0"),
    Row("k_sep_u<32,2,3,1,0>", "", "wsmall", "split", "block1.0"),
    Row("k_sep_u<64,1,3,1,0,0,1>", "", "k4occ", "split", "block1.1"),
    Row("k_sep_u<128,1,2,1,1>", "", "occ128s1", "split", "block1.0"),
    Row("k_sep_u<64,1,3,1,1>", "", "occ64s1", "split", "block1.0"),
    Row("k_sep_u<32,1,3,1,1>", "", "occ32s1", "split", "block1.0"),
    Row("k_sep_u<128,2,2,1,1>", "", "occ128s2", "split", "block1.0"),
    Row("k_sep_u<64,2,3,1,1>", "", "occ64s2", "split", "block1.0"),
    Row("k_sep_u<32,2,3,1,1>", "", "occ32s2", "split", "block1.0"),
    Row("k_sep_u<128,1,3,0,0>", "", "occ128s1", "f32", "block1.1"),
    Row("k_sep_u<64,1,4,0,0>", "", "k4", "f32", "block1.0"),
    Row("k_sep_u<32,1,4,0,0>", "", "occ32s1", "f32", "block1.1"),
    Row("k_sep_u<128,2,2,0,0>", "", "occ128s1", "f32", "block2.0"),
    Row("k_sep_u<64,2,3,0,0>", "", "k4", "f32", "block2.0"),
    Row("k_sep_u<32,2,4,0,0>", "", "wsmall", "f32", "block1.0"),
    Row("k_sep_u<64,1,3,1,0,0,1>", "tiles > slots", "rounds", "split", "block1.1"),
    Row("k_sep_u<128,1,2,1,0>", "tiles > slots", "rounds", "split", "block2.1"),
    Row("k_sep_u<128,2,2,1,0>", "tiles > slots", "rounds", "split", "block2.0"),
    # ---- k_deconv_k4<NT>: kernel 1 / 2 / 4, head_mode 1 / 2 / 2 + the class plane ----
    Row("k_deconv_k4<128>", "", "k4", "split", "deconv1"),
    Row("k_deconv_k4<64>", "", "k4", "split", "deconv2"),
    Row("k_deconv_k4<32>", "", "k4", "split", "deconv3"),
    Row("k_deconv_k4<128>", "k = 1, head_mode 1", "k4", "split", "deconv1"),
    Row("k_deconv_k4<64>", "k = 2, head_mode 2", "k4", "split", "deconv2"),
    Row("k_deconv_k4<32>", "k = 4, head_mode 2, class plane", "k4", "split", "deconv3"),
    Row("k_deconv_k4<64>", "head_mode 0", "generic", "split", "deconv2"),
    # ---- k_deconv_r<CIN> (kernel > 1 only) ----
    Row("k_deconv_r<256>", "", "twins", "split", "deconv3"),
    Row("k_deconv_r<128>", "", "twins", "split", "deconv2"),
    Row("k_deconv_r<64>", "", "occ128s2", "split", "deconv2"),
    Row("k_deconv_r<128>", "k = 2, head_mode 1", "occ128s2", "split", "deconv1"),
    Row("k_deconv_r<64>", "k = 4, head_mode 2", "occ128s2", "split", "deconv2"),
    Row("k_deconv_r<256>", "k = 2, head_mode 2, class plane", "twins", "split", "deconv3"),
    Row("k_deconv_r<128>", "head_mode 0", "unfused", "split", "deconv2"),
    Row("k_deconv_r<128>", "units > slots", "rounds", "split", "deconv2"),
    Row("k_deconv_r<256>", "units > slots", "rounds", "split", "deconv3"),
    # ---- k_deconv_u<NT, 3> ----
    Row("k_deconv_u<128,3>", "", "occ128s1", "split", "deconv1"),
    Row("k_deconv_u<64,3>", "", "occ64s1", "split", "deconv1"),
    Row("k_deconv_u<32,3>", "", "occ32s1", "split", "deconv1"),
    Row("k_deconv_u<32,3>", "k = 1, head_mode 1", "occ32s1", "split", "deconv1"),
    Row("k_deconv_u<32,3>", "k = 2, head_mode 2", "occ32s1", "split", "deconv2"),
    Row("k_deconv_u<32,3>", "k = 4, head_mode 2, class plane", "occ32s1", "split", "deconv3"),
    Row("k_deconv_u<128,3>", "head_mode 0, two column tiles", "unfused", "split", "deconv3"),
    Row("k_deconv_u<128,3>", "tiles > slots", "rounds", "split", "deconv1"),
    # ---- k_gemm_ws<NT, 1, 1, PXB>: the transposed convolutions without float16 pieces, the heads as a layer ----
    Row("k_gemm_ws<128,1,1,64>", "", "k4", "f32", "deconv1"),
    Row("k_gemm_ws<64,1,1,64>", "", "k4", "f32", "deconv2"),
    Row("k_gemm_ws<32,1,1,64>", "", "k4", "f32", "deconv3"),
    Row("k_gemm_ws<128,1,1,128>", "", "occ128s1", "f32", "deconv1"),
    Row("k_gemm_ws<64,1,1,128>", "", "occ128s1", "f32", "deconv2"),
    Row("k_gemm_ws<32,1,1,128>", "", "occ128s1", "f32", "deconv3"),
    Row("k_gemm_ws<32,1,1,64>", "the heads layer", "unfused", "split", "heads"),
    # ---- k_gemm_ws<NT, 0, S, PXB>: PP_SEP_KERNEL=ws ----
    Row("k_gemm_ws<128,0,1,64>", "", "ws-k4", "split", "block2.1"),
    Row("k_gemm_ws<64,0,1,64>", "", "ws-k4", "split", "block1.0"),
    Row("k_gemm_ws<32,0,1,64>", "", "ws-wsmall", "split", "block1.1"),
    Row("k_gemm_ws<128,0,2,64>", "", "ws-k4", "split", "block2.0"),
    Row("k_gemm_ws<64,0,2,64>", "", "ws-wsmall", "split", "block2.0"),
    Row("k_gemm_ws<32,0,2,64>", "", "ws-wsmall", "split", "block1.0"),
    Row("k_gemm_ws<128,0,1,128>", "", "ws-occ128s1", "split", "block1.1"),
    Row("k_gemm_ws<64,0,1,128>", "", "ws-occ64s1", "split", "block1.1"),
    Row("k_gemm_ws<32,0,1,128>", "", "ws-occ32s1", "split", "block1.1"),
    Row("k_gemm_ws<128,0,2,128>", "", "ws-occ128s1", "split", "block2.0"),
    Row("k_gemm_ws<64,0,2,128>", "", "ws-occ64s2", "split", "block1.0"),
    Row("k_gemm_ws<32,0,2,128>", "", "ws-occ32s2", "split", "block1.0"),
    # ---- k_gemm_layer<NT, MODE>: maps no pixel-pair producer takes ----
    Row("k_gemm_layer<128,0>", "", "generic", "split", "block3.1"),
    Row("k_gemm_layer<64,0>", "", "generic", "split", "block2.1"),
    Row("k_gemm_layer<32,0>", "", "generic", "split", "block1.1"),
    Row("k_gemm_layer<128,1>", "", "generic", "f32", "deconv1"),
    Row("k_gemm_layer<64,1>", "", "generic", "f32", "deconv2"),
    Row("k_gemm_layer<32,1>", "", "generic", "f32", "deconv3"),
    Row("k_gemm_layer<32,1>", "the heads layer", "generic", "split", "heads"),
]
F32_CASES = sorted({r.case for r in ROWS if r.prec == "f32"})            # these engines run a second time in float32
CLS_PLANE_CASES = sorted({r.case for r in ROWS if "class plane" in r.variant})   # these also run `detect`


def base(case):
    """The case whose oracle answers for this one (the switches change kernels, not values)."""
    return BY_NAME[case.name[3:]] if case.name.startswith("ws-") else case


def config(case):
    B = case.max_batch
    cfg = copy.deepcopy(pp.config.pedestrian_d435i_config(B))
    nx, ny = case.nx, case.ny
    s1, s2, s3 = case.strides
    osf = s1 // case.up0
    x0, y0 = 0.0, -ny * CELL / 2
    cfg["eval_input_reader"].update(batch_size=B, feature_map_size=[1, ny // osf, nx // osf])
    s = cfg["model"]["second"]
    s["voxel_generator"].update(point_cloud_range=[x0, y0, Z_RANGE[0], x0 + nx * CELL, y0 + ny * CELL, Z_RANGE[1]],
                                voxel_size=[CELL, CELL, Z_RANGE[1] - Z_RANGE[0]], max_number_of_voxels=case.max_voxels)
    s["voxel_feature_extractor"]["num_filters"] = case.pfn
    s["rpn"].update(layer_nums=list(case.layer_nums), layer_strides=[s1, s2, s3], num_filters=list(case.filters),
                    upsample_strides=[case.up0, case.up0 * s2, case.up0 * s2 * s3], num_upsample_filters=list(case.ups))
    s["target_assigner"]["anchor_generators"]["anchor_generator_stride"].update(
        strides=[CELL * osf, CELL * osf, 0.0], offsets=[x0 + CELL * osf, y0, -1.465])
    return cfg


def frames(case):
    """case.batch seeded clouds, uniform over the range (every border row and column of the maps gets pillars)."""
    rng = np.random.default_rng(case.seed)
    lo = [0.0, -case.ny * CELL / 2, Z_RANGE[0]]
    hi = [case.nx * CELL, case.ny * CELL / 2, Z_RANGE[1]]
    return [rng.uniform(lo, hi, (case.points[b % len(case.points)] + 7 * b, 3)).astype(np.float32) for b in range(case.batch)]


# ---- the layer table, as pp_create builds it (csrc/pp_api.hip, "layer table + map sizes") ----
def _sparse_canvas(case, layer0):
    """decide_sparse_canvas: a large, mostly empty grid whose first layer runs a kernel with the cell-map lookup at
    max_batch (sparse_input_supported: a uniform-wave separable kernel on float16 pieces)."""
    if case.nx * case.ny < 32768 or 4 * case.max_voxels > case.nx * case.ny or dict(case.env).get("PP_DENSE_CANVAS") == "1":
        return False
    name = pp.planner.plan_layer_name(layer0, case.max_batch, CUS)
    return name.startswith(("k_sep_k4", "k_sep_p")) or (name.startswith("k_sep_u") and name.split(",")[3] == "1")


def layer_table(case, prec="split"):
    """[(name, desc)] in launch order; desc is what pp.planner.plan_layer_name takes.  prec: 'split' (weights as float16
    pieces: init_weights stays inside their range) or 'f32' (set_gemm_precision('f32'): no layer has pieces)."""
    d = pp.config.Derived(config(case))
    split = prec == "split"
    h, w, cin = d.ny, d.nx, d.pfn_filters
    out = []
    for b in range(3):
        for j in range(d.layer_nums[b] + 1):
            s = d.layer_strides[b] if j == 0 else 1
            L = dict(kind="sep", cin=cin, cout=d.num_filters[b], n_total=d.num_filters[b], stride=s, k=0, in_h=h, in_w=w,
                     out_h=(h + 2 - 3) // s + 1, out_w=(w + 2 - 3) // s + 1, head_mode=0,
                     has_wt16=int(split and cin % 16 == 0), has_head_wt16=0, sparse_input=0)
            out.append((f"block{b + 1}.{j}", L))
            h, w, cin = L["out_h"], L["out_w"], L["cout"]
        k = d.upsample_strides[b]
        D = dict(kind="deconv", cin=cin, cout=d.num_upsample_filters[b], n_total=k * k * d.num_upsample_filters[b], stride=0,
                 k=k, in_h=h, in_w=w, out_h=h * k, out_w=w * k, head_mode=0, has_wt16=int(split and cin % 16 == 0),
                 has_head_wt16=0, sparse_input=0)
        assert (D["out_h"], D["out_w"]) == (d.head_h, d.head_w), (case.name, b, D, d.head_h, d.head_w)
        out.append((f"deconv{b + 1}", D))
    decs = [L for _, L in out if L["kind"] == "deconv"]
    fuse = all(L["cout"] in (32, 64, 128) and (L["in_h"] * L["in_w"]) % 4 == 0 for L in decs)      # deconv_can_fuse_heads
    if fuse:
        for i, L in enumerate(decs):
            L["head_mode"] = 1 if i == 0 else 2
            L["has_head_wt16"] = int(split and L["cout"] % 32 == 0)
    else:
        CC = sum(d.num_upsample_filters)
        out.append(("heads", dict(kind="head", cin=CC, cout=32, n_total=32, stride=0, k=0, in_h=d.head_h, in_w=d.head_w,
                                  out_h=d.head_h, out_w=d.head_w, head_mode=0, has_wt16=0, has_head_wt16=0, sparse_input=0)))
    if split:
        out[0][1]["sparse_input"] = int(_sparse_canvas(case, out[0][1]))
    return out


def plan(case, prec="split", cus=CUS):
    """{layer name: full instantiation name} of the case at its batch on a part with `cus` compute units."""
    return {n: pp.planner.plan_layer_name(L, case.batch, cus) for n, L in layer_table(case, prec)}


def tag_of(full):
    """The form Engine.layer_tags() shows: without the SH argument of k_sep_u / k_sep_p."""
    if full.startswith("k_sep_p"):
        return "k_sep_p"
    if full.startswith("k_sep_u") and full.endswith(",0,1>"):
        return full[:-len(",0,1>")] + ">"
    return full


# ---- the oracle's maps layer by layer, float64 (oracle/nn_ref.py hands out the head maps only) ----
def layer_activity(case, w, canvas, chunk=8):
    """{layer name: (share of nonzero output elements, do the first and last row and column of the map hold a nonzero
    value)} of the separable layers and the transposed convolutions (after BatchNorm and ReLU) and of the heads (the
    three head maps side by side), from the oracle's canvas.  A plain restatement of the backbone in float64, `chunk`
    frames at a time; the maps are not kept."""
    from oracle import nn_ref
    d = pp.config.Derived(config(case))
    f64 = lambda a: np.asarray(a, np.float64)

    def bn(x, prefix):
        p = {k: f64(v) for k, v in nn_ref._bn_params(w, prefix).items()}
        sc = p["gamma"] / np.sqrt(p["moving_variance"] + nn_ref.BN_EPS)
        return x * sc + (p["beta"] - p["moving_mean"] * sc)

    def sep(x, prefix, s):
        B, H, W, C = x.shape
        xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        dwk = f64(w[prefix + "/depthwise_kernel"])
        acc = np.zeros((B, Ho, Wo, C))
        for i in range(3):
            for j in range(3):
                acc += xp[:, i:i + (Ho - 1) * s + 1:s, j:j + (Wo - 1) * s + 1:s, :] * dwk[i, j, :, 0]
        return np.maximum(bn(acc @ f64(w[prefix + "/pointwise_kernel"])[0, 0], prefix + "/bn"), 0.0)

    tally = {}

    def note(name, m):
        nz = m != 0
        t = tally.setdefault(name, [0, 0, np.zeros(4, bool)])
        t[0] += int(nz.sum())
        t[1] += nz.size
        t[2] |= [nz[:, 0].any(), nz[:, -1].any(), nz[:, :, 0].any(), nz[:, :, -1].any()]

    for b0 in range(0, canvas.shape[0], chunk):
        x = f64(canvas[b0:b0 + chunk])
        ups = []
        for b in range(3):
            for j in range(d.layer_nums[b] + 1):
                x = sep(x, f"rpn/block{b + 1}/{j}", d.layer_strides[b] if j == 0 else 1)
                note(f"block{b + 1}.{j}", x)
            k = f64(w[f"rpn/deconv{b + 1}/kernel"])
            B, H, W, _ = x.shape
            u = np.einsum("bhwc,ijoc->bhiwjo", x, k).reshape(B, H * k.shape[0], W * k.shape[0], k.shape[2])
            u = np.maximum(bn(u, f"rpn/deconv{b + 1}/bn"), 0.0)
            note(f"deconv{b + 1}", u)
            ups.append(u)
        cat = np.concatenate(ups, axis=-1)
        note("heads", np.concatenate([cat @ f64(w[key + "/kernel"])[0, 0] + f64(w[key + "/bias"])
                                      for key in ("rpn/conv_box", "rpn/conv_cls", "rpn/conv_dir_cls") if key + "/kernel" in w], axis=-1))
    return {n: (t[0] / t[1], bool(t[2].all())) for n, t in tally.items()}


_EX, _REF = {}, {}


def example(case):
    """(Derived, weights, frames, the oracle's example: padded voxels, point counts, coordinates, ...) of a case, computed
    once and shared; nobody writes into it."""
    import util_ref
    case = base(case)
    if case.name not in _EX:
        d = pp.config.Derived(config(case))
        fr = frames(case)
        rect, trv, p2 = pp.synth.default_calib()
        _EX[case.name] = (d, pp.weights.init_weights(d, seed=case.seed), fr, util_ref.oracle_example(d, fr, rect, trv, p2)[0])
    return _EX[case.name]


def reference(case, dets=False):
    """The oracle's answer for a case, computed once and shared; nobody writes into it: dict with d (Derived), w (weights),
    frames, example, preds (the head maps), canvas and -- dets=True -- dets (the reference's predict() on them)."""
    import util_ref
    from oracle import ref_numpy as rn
    case = base(case)
    if case.name not in _REF:
        d, w, fr, ex = example(case)
        preds, canvas, _ = util_ref.oracle_forward(d, w, ex)
        _REF[case.name] = dict(d=d, w=w, frames=fr, example=ex, preds=preds, canvas=canvas)
    r = _REF[case.name]
    if dets and "dets" not in r:
        r["dets"] = rn.predict(r["example"], r["preds"], r["d"].nms_dict())
    return r


def plans_of_env(env, cus=CUS):
    """{case name: {prec: {layer: full instantiation name}}} of the cases of one switch set; call it in a process started
    with that set (the switches are read once per process)."""
    import os
    assert all(os.environ.get(k) == v for k, v in env), env
    return {c.name: {prec: plan(c, prec, cus) for prec in ("split", "f32")} for c in CASES if c.env == env}


if __name__ == "__main__":          # python tests/backbone_ledger.py <index into ENVS> [compute units]: the plans as JSON
    import json
    import sys
    print(json.dumps(plans_of_env(ENVS[int(sys.argv[1])], int(sys.argv[2]) if len(sys.argv) > 2 else CUS)))
