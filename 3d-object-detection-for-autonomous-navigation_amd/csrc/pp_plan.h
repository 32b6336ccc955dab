// The backbone's kernel planner: which template instantiation of backbone.hip runs one launch of a layer.
//
// plan_layer(L, rows, m_end, env) is a function of its arguments: the layer description, the launch's size, and a
// PlanEnv -- the compute units of the part and the process's switch table (pp_switches.h), which a handle fills once at
// pp_create.  Nothing here reads the environment, holds a static, names an engine, makes a HIP call or contains device
// code, so two environments can be planned side by side in one process: tools/plan_host_check.hip does, on a CPU
// machine.  backbone.hip keeps the kernels, the launch_* helpers and launch_layer's dispatch switch over a LayerPlan.
//
// Of L the planner reads the shape fields, head_mode, and whether d_wt16 / d_head_wt16 / d_occ are NULL ("has float16
// weight pieces / float16 head weights / a sparse input").
#pragma once

#include <stdio.h>

#include <string>

#include "pp_common.h"
#include "pp_switches.h"

// What a plan depends on besides the layer and the launch's size.  A member of pp_engine (pp_create: the device's
// compute units, the process-wide switch table); pp_plan_layer_name builds one from its compute_units argument.
struct PlanEnv {
    int cus = 256;      // compute units: sizes the persistent grids and weighs the small-map crossovers
    PpSwitches sw;
};

// does layer L run on the split-precision MFMA?  (its weights fit the float16 pieces and the precision is not forced:
// PP_GEMM_PREC=f32 selects the float32 MFMA)
inline bool split_operands(const LayerDesc& L, const PpSwitches& sw) { return L.d_wt16 != nullptr && !sw.gemm_f32; }
// channel tile of the GEMM kernels: the widest of 128 / 64 / 32 that divides cout
constexpr int col_tile(int cout) { return cout % 128 == 0 ? 128 : (cout % 64 == 0 ? 64 : 32); }

// workgroups per CU of k_sep_u<NT, S, ., PREC> (one wave per SIMD each): the register budgets of the float32 and
// the split-precision instantiations differ (split-precision k_sep_u<128, 1>: 256 / 168)
constexpr int SEP128_WPB = 2, SEP64_WPB = 3;
constexpr int sep_u_wpc(int nt, int s, bool prec) {
    return s == 1 ? (prec ? (nt == 128 ? SEP128_WPB : (nt == 64 ? SEP64_WPB : 3)) : (nt == 128 ? 3 : 4))
                  : (prec ? (nt == 128 ? 2 : 3) : (nt == 128 ? 2 : (nt == 64 ? 3 : 4)));
}

// may this stride-1 launch share window columns between the lanes of a DPP row?  (SEP_SHARED_WINDOW: the output width
// a multiple of 8 -- a DPP row's 8 pixels then never straddle an image row, a frame or the end of the data -- and the
// input map the size of the output map)
inline bool sep_shared_window(const LayerDesc& L) {
    return L.stride == 1 && L.out_w % 8 == 0 && L.in_w == L.out_w && L.in_h == L.out_h;
}

// does k_sep_p run this separable layer?  (256 output channels, stride 1, dense input, large enough for the persistent
// kernels)
inline bool sep_p_runs(const LayerDesc& L, long long M, const PpSwitches& sw) {
    // (the 128-channel instantiation, where k_sep_u already computes the depthwise once, measured 32 us against 28.5)
    return split_operands(L, sw) && L.stride == 1 && L.d_occ == nullptr && L.cout == 256 && L.n_total == 256 &&
           L.cin % 64 == 0 && L.cin <= 256 && M < (1 << 24);
}

// the split-K kernel runs a layer while the map is too small to fill the chip with 32-pixel wave tiles.
// Measured crossover against k_sep_u (tools/k4_sweep.sh, cfg-A, B = 2..16): 1.5 workgroups per CU for
// cin = 64, 2.5 for cin = 128, 3 for cin = 256 -- the longer the K chain, the later k_sep_u catches up.
// PP_SEP_K4=0 turns it off, PP_SEP_K4=n sets the limit to n workgroups per CU for every layer.
inline bool sep_k4_runs(const LayerDesc& L, long long M, const PlanEnv& env) {
    const int force = env.sw.sep_k4;
    if (force == 0 || !split_operands(L, env.sw) || L.cin % 64 != 0 || L.cin > 256 || L.n_total % 64 != 0) return false;
    const int half_cus = (force > 0) ? 2 * force : (L.cin <= 64 ? 3 : (L.cin <= 128 ? 5 : 6));
    return 2 * ((M + 31) / 32 * (L.n_total / 64)) <= (long long)half_cus * env.cus;
}
// eight-way split: cin = 256 and at most one workgroup per CU (the latency case proper: a frame or two).  Measured
// at B=1 (tools/latency_b1.py): block3.1-.5 8.1 -> 7.2 us; the 128-channel layers gain nothing (block2.x 5.8 -> 5.6,
// block3.0 6.0 -> 7.0: one iteration per wave leaves nothing to pipeline) and keep four waves
inline bool sep_k8_runs(const LayerDesc& L, long long M, int cus) {
    return L.cin % 256 == 0 && (M + 31) / 32 * (L.n_total / 64) <= (long long)cus;
}

// k_deconv_r runs where k_deconv_u would and the shape fits (cout == 128, cin 64 / 128 / 256)
inline bool deconv_r_runs(const LayerDesc& L) {
    // kernel == stride 1 has one tap per tile: nothing is re-read or re-split, and k_deconv_u's two-chunk register
    // prefetch hides the tile changes better (deconv1 at B=64: 35.4 us against 37.1)
    return L.k > 1 && L.cout == 128 && (L.cin == 64 || L.cin == 128 || L.cin == 256);
}

// k_deconv_k4 runs while the layer has at most 1.5 workgroups per CU (measured crossover against k_deconv_u on cfg-A,
// tools/k4_sweep.sh: ahead at B = 1, 2 (160 / 320 workgroups), behind from B = 4); PP_DECONV_K4=0: never,
// =n: up to n per CU
inline bool deconv_k4_runs(const LayerDesc& L, long long M, const PlanEnv& env) {
    const int force = env.sw.deconv_k4;
    if (force == 0 || L.cin % 64 != 0 || L.cin > 256) return false;
    const int nt = col_tile(L.cout);
    const int half_cus = force > 0 ? 2 * force : 3;
    return 2 * ((M + 31) / 32 * (L.n_total / nt)) <= (long long)half_cus * env.cus;
}

// k_gemm_ws: 128-pixel tiles (8-wave workgroups: every SIMD hosts one consumer and one producer wave) are the
// default.  64-pixel tiles (4-wave workgroups) are used only when a launch would otherwise not even
// cover the chip's CUs once (small batches): measured at B=64 they are slower -- a 4-wave
// workgroup's two consumer waves land on two of the four SIMDs, so the matrix pipes are unevenly fed.
inline bool ws_small_tile(long long M, int n_total, int NT) {
    const long long tiles128 = ((M + 127) / 128) * (n_total / NT);
    return tiles128 < 256;
}

// channel-tile width of the uniform-wave kernel: the widest that divides cout, narrowed to 64 when
// the layer would otherwise put fewer than ~2.5 waves on a SIMD (small maps: a wave per 32 pixels x NT
// channels is the scheduling grain; the depthwise is recomputed per channel tile, which the idle
// vector pipe absorbs).  PP_SEP_NT=64 / 128 forces the width of the layers that could run either.
inline int sep_u_nt(const LayerDesc& L, long long rows, const PlanEnv& env) {
    if (L.cout % 64 != 0) return 32;
    if (L.cout % 128 != 0) return 64;
    const long long waves128 = (rows + 31) / 32 * (L.cout / 128);
    if (env.sw.sep_nt == 64 || env.sw.sep_nt == 128) return env.sw.sep_nt;
    // split-precision path: the depthwise (VALU) is the larger half of a chunk, so recomputing it per
    // channel tile costs more than the thinner wave supply (measured: block3 at B=64 36 vs 40 us)
    if (split_operands(L, env.sw)) return 128;
    return (waves128 * 2 < 5ll * env.cus * 4) ? 64 : 128;
}

inline bool use_ws(const LayerDesc& L) {
    // MODE 1 producers own 4 consecutive pixels, MODE 0 producers 2 of one row: the frame's pixel
    // count (hence every batch's) must be divisible accordingly, else the generic kernel runs
    if (L.kind != LAYER_SEP) return (L.in_h * L.in_w) % 4 == 0;
    return (L.stride == 1 || L.stride == 2) && (L.out_w % 2 == 0);
}

// the uniform-wave separable kernels (k_sep_u and the split-K / 256-channel ones chosen among them) run a separable
// layer whose pixel range ends at m_end (k_sep_u's float-reciprocal index math).  They are the default;
// PP_SEP_KERNEL=ws selects the producer/consumer kernel (k_gemm_ws).
inline bool sep_uniform_runs(const LayerDesc& L, long long m_end, const PpSwitches& sw) {
    return L.kind == LAYER_SEP && use_ws(L) && !sw.sep_ws && m_end < (1 << 24);
}

// one workgroup column covers the whole channel range of a deconv's tap (NT == cout): the fused head GEMM fits
inline bool one_column_tile(const LayerDesc& L) {
    return L.cout == 32 || L.cout == 64 || L.cout == 128;
}

// the split-precision uniform-wave deconv kernel runs when its operands exist (cin % 32 == 0: an even
// number of 16-channel chunks) and, with fused heads, when one column tile covers the tap
inline bool deconv_uniform(const LayerDesc& L, const PpSwitches& sw) {
    if (L.kind != LAYER_DECONV || !split_operands(L, sw) || L.cin % 32 != 0) return false;
    if (L.head_mode != 0 && (L.d_head_wt16 == nullptr || !one_column_tile(L))) return false;
    return true;
}

inline long long layer_rows(const LayerDesc& L, int batch) {
    return (L.kind == LAYER_SEP) ? (long long)batch * L.out_h * L.out_w : (long long)batch * L.in_h * L.in_w;
}

// the kernel that runs one launch of a layer, with its template arguments
enum class LayerKernel { SEP_K4, SEP_P, SEP_U, DECONV_K4, DECONV_R, DECONV_U, GEMM_WS, GEMM_LAYER };
struct LayerPlan {
    LayerKernel kernel;
    int nt;      // channel tile NT (k_sep_u, k_deconv_k4 / _u, k_gemm_ws / _layer)
    int cin;     // CIN (k_deconv_r)
    int s;       // stride S (k_sep_k4, k_sep_u, k_gemm_ws)
    int wpc;     // workgroups per CU (k_sep_u)
    int prec;    // PREC, OCC (k_sep_u)
    int occ;
    int k8;      // the eight-way split (k_sep_k4)
    int sh;      // SH, shared window columns (k_sep_p, k_sep_u<64,1,.,1,0>)
    int pxb;     // pixel tile (k_gemm_ws)
    int mode;    // MODE (k_gemm_ws / _layer): 0 separable, 1 deconv or heads
};

// rows: the output rows of this launch (what the size heuristics weigh); m_end: the end of its pixel range (frame0 > 0:
// a sub-range of a larger batch, see launch_layer)
inline LayerPlan plan_layer(const LayerDesc& L, long long rows, long long m_end, const PlanEnv& env) {
    LayerPlan p = {};
    p.nt = (L.kind == LAYER_HEAD) ? 32 : col_tile(L.cout);
    p.mode = (L.kind == LAYER_SEP) ? 0 : 1;
    p.s = (L.kind == LAYER_SEP) ? L.stride : 1;
    if (sep_uniform_runs(L, m_end, env.sw)) {
        if (sep_k4_runs(L, rows, env)) {   // small map
            p.kernel = LayerKernel::SEP_K4;
            p.k8 = sep_k8_runs(L, rows, env.cus);
        } else if (sep_p_runs(L, rows, env.sw)) {   // depthwise once for 256 channels
            p.kernel = LayerKernel::SEP_P;
            p.sh = sep_shared_window(L);
        } else {
            p.kernel = LayerKernel::SEP_U;
            p.nt = sep_u_nt(L, rows, env);
            p.prec = split_operands(L, env.sw);
            p.occ = p.prec && L.d_occ != nullptr;
            p.wpc = sep_u_wpc(p.nt, p.s, p.prec);
            p.sh = p.prec && !p.occ && p.nt == 64 && p.s == 1 && sep_shared_window(L);   // (see launch_u)
        }
    } else if (deconv_uniform(L, env.sw)) {
        if (deconv_k4_runs(L, rows, env)) {   // small map: split-K
            p.kernel = LayerKernel::DECONV_K4;
        } else if (deconv_r_runs(L)) {   // input resident in registers
            p.kernel = LayerKernel::DECONV_R;
            p.cin = L.cin;
        } else {
            p.kernel = LayerKernel::DECONV_U;
        }
    } else if (use_ws(L)) {
        p.kernel = LayerKernel::GEMM_WS;
        p.pxb = ws_small_tile(rows, L.n_total, p.nt) ? 64 : 128;
    } else {
        p.kernel = LayerKernel::GEMM_LAYER;
    }
    return p;
}

// name of a plan's template instantiation.  full: with the SH argument of k_sep_p / k_sep_u, which the profiler tags
// leave out
inline std::string plan_name(const LayerPlan& p, bool full) {
    char buf[64];
    switch (p.kernel) {
    case LayerKernel::SEP_K4:
        if (p.k8) snprintf(buf, sizeof(buf), "k_sep_k4<64,%d,8>", p.s);
        else snprintf(buf, sizeof(buf), "k_sep_k4<64,%d>", p.s);
        break;
    case LayerKernel::SEP_P:
        if (!full) snprintf(buf, sizeof(buf), "k_sep_p");
        else if (p.sh) snprintf(buf, sizeof(buf), "k_sep_p<256,1>");
        else snprintf(buf, sizeof(buf), "k_sep_p<256>");
        break;
    case LayerKernel::SEP_U:
        if (full && p.sh) snprintf(buf, sizeof(buf), "k_sep_u<%d,%d,%d,%d,%d,0,1>", p.nt, p.s, p.wpc, p.prec, p.occ);
        else snprintf(buf, sizeof(buf), "k_sep_u<%d,%d,%d,%d,%d>", p.nt, p.s, p.wpc, p.prec, p.occ);
        break;
    case LayerKernel::DECONV_K4: snprintf(buf, sizeof(buf), "k_deconv_k4<%d>", p.nt); break;
    case LayerKernel::DECONV_R: snprintf(buf, sizeof(buf), "k_deconv_r<%d>", p.cin); break;
    case LayerKernel::DECONV_U: snprintf(buf, sizeof(buf), "k_deconv_u<%d,3>", p.nt); break;
    case LayerKernel::GEMM_WS: snprintf(buf, sizeof(buf), "k_gemm_ws<%d,%d,%d,%d>", p.nt, p.mode, p.s, p.pxb); break;
    case LayerKernel::GEMM_LAYER: snprintf(buf, sizeof(buf), "k_gemm_layer<%d,%d>", p.nt, p.mode); break;
    }
    return std::string(buf);
}
