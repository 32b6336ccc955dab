// Host-only check of csrc/pp_plan.h: the backbone's kernel planner as a function of its arguments.  In ONE process
// the same layer descriptions are planned under several environments (PlanEnv: compute units + switch table) and the
// full instantiation names compared with fixed strings -- what the library itself cannot show, since its own table is
// parsed once per process.  Calls no HIP entry point, so it runs on a machine without a GPU, and is meant to be built
// with the host sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -I <package>/csrc \
//         tools/plan_host_check.hip -o plan_host_check && ./plan_host_check
//
// Where the expected strings come from: NOT from pp_plan.h.  They were recorded from the library of the commit before
// the planner moved into the header, by calling planner.plan_layer_name(layer, batch, compute_units) in one child
// process per environment with the corresponding variables set (PP_SEP_KERNEL=ws, PP_GEMM_PREC=f32,
// PP_SEP_K4=0 PP_DECONV_K4=0, PP_SEP_NT=64, PP_SEP_K4=6 PP_DECONV_K4=6, and none at 256 and at 64 compute units).
// The layers are pedestrian_d435i_config's (an 80 x 64 grid, 128 PFN channels): the first and a later layer of each
// block, the three transposed convolutions with their fused-head modes, deconv2 and the heads layer as an engine
// without head fusion has them, and the sparse first layer of kitti_shaped_config; each at 1, 4 and 64 frames.
#include <stdio.h>
#include <string.h>

#include "pp_plan.h"

struct Shape {
    const char* name;
    int kind, cin, cout, n_total, stride, k, in_h, in_w, out_h, out_w, head_mode, has_wt16, has_head_wt16, sparse_input;
};
static const Shape kLayers[] = {
    {"block1.0", LAYER_SEP, 128, 64, 64, 1, 0, 64, 80, 64, 80, 0, 1, 0, 0},
    {"block1.1", LAYER_SEP, 64, 64, 64, 1, 0, 64, 80, 64, 80, 0, 1, 0, 0},
    {"block2.0", LAYER_SEP, 64, 128, 128, 2, 0, 64, 80, 32, 40, 0, 1, 0, 0},
    {"block2.1", LAYER_SEP, 128, 128, 128, 1, 0, 32, 40, 32, 40, 0, 1, 0, 0},
    {"block3.0", LAYER_SEP, 128, 256, 256, 2, 0, 32, 40, 16, 20, 0, 1, 0, 0},
    {"block3.1", LAYER_SEP, 256, 256, 256, 1, 0, 16, 20, 16, 20, 0, 1, 0, 0},
    {"deconv1 (head_mode 1)", LAYER_DECONV, 64, 128, 128, 0, 1, 64, 80, 64, 80, 1, 1, 1, 0},
    {"deconv2 (head_mode 2)", LAYER_DECONV, 128, 128, 512, 0, 2, 32, 40, 64, 80, 2, 1, 1, 0},
    {"deconv3 (head_mode 2)", LAYER_DECONV, 256, 128, 2048, 0, 4, 16, 20, 64, 80, 2, 1, 1, 0},
    {"deconv2 (head_mode 0)", LAYER_DECONV, 128, 128, 512, 0, 2, 32, 40, 64, 80, 0, 1, 0, 0},
    {"heads", LAYER_HEAD, 384, 32, 32, 0, 0, 64, 80, 64, 80, 0, 0, 0, 0},
    {"kitti block1.0 (sparse)", LAYER_SEP, 64, 64, 64, 2, 0, 496, 432, 248, 216, 0, 1, 0, 1},
};
constexpr int NL = sizeof(kLayers) / sizeof(kLayers[0]);
static const int kBatches[] = {1, 4, 64};
constexpr int NB = 3;

struct Expect {
    const char* what;
    PlanEnv env;
    const char* name[NL][NB];
};

static PlanEnv make_env(int cus, void (*set)(PpSwitches&)) {
    PlanEnv e;
    e.cus = cus;
    if (set) set(e.sw);
    return e;
}

static const Expect kExpect[] = {
    {"default, 256 CUs", make_env(256, nullptr), {
        {"k_sep_k4<64,1>", "k_sep_k4<64,1>", "k_sep_u<64,1,3,1,0,0,1>"},
        {"k_sep_k4<64,1>", "k_sep_u<64,1,3,1,0,0,1>", "k_sep_u<64,1,3,1,0,0,1>"},
        {"k_sep_k4<64,2>", "k_sep_k4<64,2>", "k_sep_u<128,2,2,1,0>"},
        {"k_sep_k4<64,1>", "k_sep_k4<64,1>", "k_sep_u<128,1,2,1,0>"},
        {"k_sep_k4<64,2>", "k_sep_k4<64,2>", "k_sep_u<128,2,2,1,0>"},
        {"k_sep_k4<64,1,8>", "k_sep_k4<64,1,8>", "k_sep_p<256>"},
        {"k_deconv_k4<128>", "k_deconv_u<128,3>", "k_deconv_u<128,3>"},
        {"k_deconv_k4<128>", "k_deconv_r<128>", "k_deconv_r<128>"},
        {"k_deconv_k4<128>", "k_deconv_r<256>", "k_deconv_r<256>"},
        {"k_deconv_k4<128>", "k_deconv_r<128>", "k_deconv_r<128>"},
        {"k_gemm_ws<32,1,1,64>", "k_gemm_ws<32,1,1,64>", "k_gemm_ws<32,1,1,128>"},
        {"k_sep_u<64,2,3,1,1>", "k_sep_u<64,2,3,1,1>", "k_sep_u<64,2,3,1,1>"}}},
    {"sep_ws (PP_SEP_KERNEL=ws)", make_env(256, [](PpSwitches& s) { s.sep_ws = true; }), {
        {"k_gemm_ws<64,0,1,64>", "k_gemm_ws<64,0,1,64>", "k_gemm_ws<64,0,1,128>"},
        {"k_gemm_ws<64,0,1,64>", "k_gemm_ws<64,0,1,64>", "k_gemm_ws<64,0,1,128>"},
        {"k_gemm_ws<128,0,2,64>", "k_gemm_ws<128,0,2,64>", "k_gemm_ws<128,0,2,128>"},
        {"k_gemm_ws<128,0,1,64>", "k_gemm_ws<128,0,1,64>", "k_gemm_ws<128,0,1,128>"},
        {"k_gemm_ws<128,0,2,64>", "k_gemm_ws<128,0,2,64>", "k_gemm_ws<128,0,2,128>"},
        {"k_gemm_ws<128,0,1,64>", "k_gemm_ws<128,0,1,64>", "k_gemm_ws<128,0,1,128>"},
        {"k_deconv_k4<128>", "k_deconv_u<128,3>", "k_deconv_u<128,3>"},
        {"k_deconv_k4<128>", "k_deconv_r<128>", "k_deconv_r<128>"},
        {"k_deconv_k4<128>", "k_deconv_r<256>", "k_deconv_r<256>"},
        {"k_deconv_k4<128>", "k_deconv_r<128>", "k_deconv_r<128>"},
        {"k_gemm_ws<32,1,1,64>", "k_gemm_ws<32,1,1,64>", "k_gemm_ws<32,1,1,128>"},
        {"k_gemm_ws<64,0,2,128>", "k_gemm_ws<64,0,2,128>", "k_gemm_ws<64,0,2,128>"}}},
    {"gemm_f32 (PP_GEMM_PREC=f32)", make_env(256, [](PpSwitches& s) { s.gemm_f32 = true; }), {
        {"k_sep_u<64,1,4,0,0>", "k_sep_u<64,1,4,0,0>", "k_sep_u<64,1,4,0,0>"},
        {"k_sep_u<64,1,4,0,0>", "k_sep_u<64,1,4,0,0>", "k_sep_u<64,1,4,0,0>"},
        {"k_sep_u<64,2,3,0,0>", "k_sep_u<64,2,3,0,0>", "k_sep_u<128,2,2,0,0>"},
        {"k_sep_u<64,1,4,0,0>", "k_sep_u<64,1,4,0,0>", "k_sep_u<128,1,3,0,0>"},
        {"k_sep_u<64,2,3,0,0>", "k_sep_u<64,2,3,0,0>", "k_sep_u<64,2,3,0,0>"},
        {"k_sep_u<64,1,4,0,0>", "k_sep_u<64,1,4,0,0>", "k_sep_u<64,1,4,0,0>"},
        {"k_gemm_ws<128,1,1,64>", "k_gemm_ws<128,1,1,64>", "k_gemm_ws<128,1,1,128>"},
        {"k_gemm_ws<128,1,1,64>", "k_gemm_ws<128,1,1,64>", "k_gemm_ws<128,1,1,128>"},
        {"k_gemm_ws<128,1,1,64>", "k_gemm_ws<128,1,1,64>", "k_gemm_ws<128,1,1,128>"},
        {"k_gemm_ws<128,1,1,64>", "k_gemm_ws<128,1,1,64>", "k_gemm_ws<128,1,1,128>"},
        {"k_gemm_ws<32,1,1,64>", "k_gemm_ws<32,1,1,64>", "k_gemm_ws<32,1,1,128>"},
        {"k_sep_u<64,2,3,0,0>", "k_sep_u<64,2,3,0,0>", "k_sep_u<64,2,3,0,0>"}}},
    {"sep_k4 = 0, deconv_k4 = 0", make_env(256, [](PpSwitches& s) { s.sep_k4 = 0; s.deconv_k4 = 0; }), {
        {"k_sep_u<64,1,3,1,0,0,1>", "k_sep_u<64,1,3,1,0,0,1>", "k_sep_u<64,1,3,1,0,0,1>"},
        {"k_sep_u<64,1,3,1,0,0,1>", "k_sep_u<64,1,3,1,0,0,1>", "k_sep_u<64,1,3,1,0,0,1>"},
        {"k_sep_u<128,2,2,1,0>", "k_sep_u<128,2,2,1,0>", "k_sep_u<128,2,2,1,0>"},
        {"k_sep_u<128,1,2,1,0>", "k_sep_u<128,1,2,1,0>", "k_sep_u<128,1,2,1,0>"},
        {"k_sep_u<128,2,2,1,0>", "k_sep_u<128,2,2,1,0>", "k_sep_u<128,2,2,1,0>"},
        {"k_sep_p<256>", "k_sep_p<256>", "k_sep_p<256>"},
        {"k_deconv_u<128,3>", "k_deconv_u<128,3>", "k_deconv_u<128,3>"},
        {"k_deconv_r<128>", "k_deconv_r<128>", "k_deconv_r<128>"},
        {"k_deconv_r<256>", "k_deconv_r<256>", "k_deconv_r<256>"},
        {"k_deconv_r<128>", "k_deconv_r<128>", "k_deconv_r<128>"},
        {"k_gemm_ws<32,1,1,64>", "k_gemm_ws<32,1,1,64>", "k_gemm_ws<32,1,1,128>"},
        {"k_sep_u<64,2,3,1,1>", "k_sep_u<64,2,3,1,1>", "k_sep_u<64,2,3,1,1>"}}},
    {"sep_nt = 64", make_env(256, [](PpSwitches& s) { s.sep_nt = 64; }), {
        {"k_sep_k4<64,1>", "k_sep_k4<64,1>", "k_sep_u<64,1,3,1,0,0,1>"},
        {"k_sep_k4<64,1>", "k_sep_u<64,1,3,1,0,0,1>", "k_sep_u<64,1,3,1,0,0,1>"},
        {"k_sep_k4<64,2>", "k_sep_k4<64,2>", "k_sep_u<64,2,3,1,0>"},
        {"k_sep_k4<64,1>", "k_sep_k4<64,1>", "k_sep_u<64,1,3,1,0,0,1>"},
        {"k_sep_k4<64,2>", "k_sep_k4<64,2>", "k_sep_u<64,2,3,1,0>"},
        {"k_sep_k4<64,1,8>", "k_sep_k4<64,1,8>", "k_sep_p<256>"},
        {"k_deconv_k4<128>", "k_deconv_u<128,3>", "k_deconv_u<128,3>"},
        {"k_deconv_k4<128>", "k_deconv_r<128>", "k_deconv_r<128>"},
        {"k_deconv_k4<128>", "k_deconv_r<256>", "k_deconv_r<256>"},
        {"k_deconv_k4<128>", "k_deconv_r<128>", "k_deconv_r<128>"},
        {"k_gemm_ws<32,1,1,64>", "k_gemm_ws<32,1,1,64>", "k_gemm_ws<32,1,1,128>"},
        {"k_sep_u<64,2,3,1,1>", "k_sep_u<64,2,3,1,1>", "k_sep_u<64,2,3,1,1>"}}},
    {"sep_k4 = 6, deconv_k4 = 6", make_env(256, [](PpSwitches& s) { s.sep_k4 = 6; s.deconv_k4 = 6; }), {
        {"k_sep_k4<64,1>", "k_sep_k4<64,1>", "k_sep_u<64,1,3,1,0,0,1>"},
        {"k_sep_k4<64,1>", "k_sep_k4<64,1>", "k_sep_u<64,1,3,1,0,0,1>"},
        {"k_sep_k4<64,2>", "k_sep_k4<64,2>", "k_sep_u<128,2,2,1,0>"},
        {"k_sep_k4<64,1>", "k_sep_k4<64,1>", "k_sep_u<128,1,2,1,0>"},
        {"k_sep_k4<64,2>", "k_sep_k4<64,2>", "k_sep_u<128,2,2,1,0>"},
        {"k_sep_k4<64,1,8>", "k_sep_k4<64,1,8>", "k_sep_p<256>"},
        {"k_deconv_k4<128>", "k_deconv_k4<128>", "k_deconv_u<128,3>"},
        {"k_deconv_k4<128>", "k_deconv_k4<128>", "k_deconv_r<128>"},
        {"k_deconv_k4<128>", "k_deconv_k4<128>", "k_deconv_r<256>"},
        {"k_deconv_k4<128>", "k_deconv_k4<128>", "k_deconv_r<128>"},
        {"k_gemm_ws<32,1,1,64>", "k_gemm_ws<32,1,1,64>", "k_gemm_ws<32,1,1,128>"},
        {"k_sep_u<64,2,3,1,1>", "k_sep_u<64,2,3,1,1>", "k_sep_u<64,2,3,1,1>"}}},
    {"default, 64 CUs", make_env(64, nullptr), {
        {"k_sep_k4<64,1>", "k_sep_u<64,1,3,1,0,0,1>", "k_sep_u<64,1,3,1,0,0,1>"},
        {"k_sep_u<64,1,3,1,0,0,1>", "k_sep_u<64,1,3,1,0,0,1>", "k_sep_u<64,1,3,1,0,0,1>"},
        {"k_sep_k4<64,2>", "k_sep_u<128,2,2,1,0>", "k_sep_u<128,2,2,1,0>"},
        {"k_sep_k4<64,1>", "k_sep_u<128,1,2,1,0>", "k_sep_u<128,1,2,1,0>"},
        {"k_sep_k4<64,2>", "k_sep_k4<64,2>", "k_sep_u<128,2,2,1,0>"},
        {"k_sep_k4<64,1,8>", "k_sep_k4<64,1>", "k_sep_p<256>"},
        {"k_deconv_u<128,3>", "k_deconv_u<128,3>", "k_deconv_u<128,3>"},
        {"k_deconv_r<128>", "k_deconv_r<128>", "k_deconv_r<128>"},
        {"k_deconv_r<256>", "k_deconv_r<256>", "k_deconv_r<256>"},
        {"k_deconv_r<128>", "k_deconv_r<128>", "k_deconv_r<128>"},
        {"k_gemm_ws<32,1,1,64>", "k_gemm_ws<32,1,1,64>", "k_gemm_ws<32,1,1,128>"},
        {"k_sep_u<64,2,3,1,1>", "k_sep_u<64,2,3,1,1>", "k_sep_u<64,2,3,1,1>"}}},
};
constexpr int NE = sizeof(kExpect) / sizeof(kExpect[0]);

static LayerDesc describe(const Shape& s) {
    static float pieces;                 // what the planner asks of the weight pointers is only whether they are NULL
    static int cells;
    LayerDesc L;
    memset(&L, 0, sizeof(L));
    L.kind = s.kind; L.cin = s.cin; L.cout = s.cout; L.n_total = s.n_total; L.stride = s.stride; L.k = s.k;
    L.in_h = s.in_h; L.in_w = s.in_w; L.out_h = s.out_h; L.out_w = s.out_w; L.head_mode = s.head_mode;
    L.d_wt16 = s.has_wt16 ? &pieces : nullptr;
    L.d_head_wt16 = s.has_head_wt16 ? &pieces : nullptr;
    L.d_occ = s.sparse_input ? &cells : nullptr;
    L.name = s.name;
    return L;
}

static std::string name_of(const LayerDesc& L, int batch, const PlanEnv& env) {
    return plan_name(plan_layer(L, layer_rows(L, batch), layer_rows(L, batch), env), true);
}

int main() {
    int bad = 0, differing = 0;
    for (int l = 0; l < NL; ++l) {
        const LayerDesc L = describe(kLayers[l]);
        for (int b = 0; b < NB; ++b) {
            for (int e = 0; e < NE; ++e) {
                const std::string got = name_of(L, kBatches[b], kExpect[e].env);
                if (got != kExpect[e].name[l][b]) {
                    fprintf(stderr, "%s at batch %d under [%s]: planned %s, recorded %s\n", kLayers[l].name, kBatches[b],
                            kExpect[e].what, got.c_str(), kExpect[e].name[l][b]);
                    ++bad;
                }
                // the thing one process could not show before: another environment, another plan, side by side
                if (e > 0 && got != name_of(L, kBatches[b], kExpect[0].env)) ++differing;
            }
        }
    }
    // planning is a function of its arguments: an environment planned again after the others gives what it gave first
    const LayerDesc L0 = describe(kLayers[0]);
    if (name_of(L0, 1, kExpect[1].env) == name_of(L0, 1, kExpect[0].env)) { fprintf(stderr, "sep_ws and the default agree on block1.0\n"); ++bad; }
    if (name_of(L0, 1, kExpect[0].env) != "k_sep_k4<64,1>" || name_of(L0, 1, kExpect[1].env) != "k_gemm_ws<64,0,1,64>") ++bad;
    // the compute units alone: block1.1 at one frame is a split-K layer on 256 CUs and a k_sep_u layer on 64
    const LayerDesc L1 = describe(kLayers[1]);
    if (name_of(L1, 1, kExpect[0].env) == name_of(L1, 1, kExpect[NE - 1].env)) { fprintf(stderr, "256 and 64 CUs agree on block1.1\n"); ++bad; }
    if (differing == 0) { fprintf(stderr, "no environment changed any plan\n"); ++bad; }
    if (bad) { fprintf(stderr, "plan_host_check: %d mismatches\n", bad); return 1; }
    printf("plan_host_check: OK (%d layers x %d batches x %d environments, %d plans differ from the default's)\n", NL, NB, NE, differing);
    return 0;
}
