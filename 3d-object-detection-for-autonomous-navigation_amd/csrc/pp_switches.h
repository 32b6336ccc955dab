// The PP_* environment switches of libpp_hip.so as one plain struct.  The process-wide
// instance is parsed from the environment on first use and never again (pp_parse_switches / pp_switches, both in
// pp_api.hip: the only place in csrc/ that reads the environment).  Nothing else in the library calls getenv: a handle
// copies the table at pp_create (PlanEnv, pp_plan.h) and every choice that depends on a switch takes it as an argument.
// Plain C++: no HIP, no engine.
#pragma once

// The PP_TRAIN_* switches (the training step, train.hip)
struct TrainSwitches {
    long fused_min = 32768;       // PP_TRAIN_FUSED_MIN: fused separable forward from this many output pixels on
    bool split_gemm = true;       // PP_TRAIN_GEMM=f32 clears it: every product on k_tr_gemm
    long fin256 = 128, fin64 = 32;   // PP_TRAIN_FIN_THR=a,b: BatchNorm finalize widths
    long arena_floats = 0;        // PP_TRAIN_ARENA_FLOATS: cap of the split-K / deferred-reduction arena (0: none)
};

struct PpSwitches {
    bool gemm_f32 = false;        // PP_GEMM_PREC=f32: the float32 MFMA instead of the split-precision float16 one
    bool sep_ws = false;          // PP_SEP_KERNEL=ws: separable layers on k_gemm_ws instead of the uniform-wave kernels
    int sep_nt = 0;               // PP_SEP_NT: 64 or 128 forces k_sep_u's channel tile (any other value: the heuristic)
    int sep_k4 = -1;              // PP_SEP_K4: -1 (unset) the measured limits, 0 never, n > 0 up to n workgroups per CU
    int deconv_k4 = -1;           // PP_DECONV_K4: likewise for k_deconv_k4
    bool pfn_first_generation = false;   // PP_PFN_KERNEL=1: the first-generation PFN kernel for the fused path
    bool dense_canvas = false;    // PP_DENSE_CANVAS=1: no sparse canvas
    bool no_graph = false;        // PP_NO_GRAPH=1: plain launches, no captured graphs
    bool no_head_fusion = false;  // PP_NO_HEAD_FUSION set (to anything): the heads as a layer of their own
    TrainSwitches train;
};

PpSwitches pp_parse_switches();        // from the environment
const PpSwitches& pp_switches();       // the process-wide table: pp_parse_switches() on first use
