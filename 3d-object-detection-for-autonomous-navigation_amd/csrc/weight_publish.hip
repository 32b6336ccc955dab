// Trainer weights -> detector weights on the device (pp_publish_train_weights, api_publish.hip): the kernels read the
// flat parameter / state buffers of pp_train_layout and write every array pp_finalize_weights produces on the host, in
// the same layouts and with the same float32 values -- BatchNorm folded from the moving statistics (bn_fold), the
// pointwise kernels transposed, the head matrix assembled, the float16 piece pairs of split_weights_f16x2 and the range
// rule of f16_pair_range_ok.  Host-equal arithmetic as in targets.hip: the build has -ffp-contract=off, division and
// sqrt are IEEE, float -> float16 rounds to nearest even.
//
// Two launches.  k_publish_fold: one thread per float32 output element, a run of whole workgroups per task (a task is
// one output array; the table lives in a small device array and a workgroup finds its task by bisection on uniform
// values).  Threads run along the output's fastest dimension, so every store is coalesced; the transposed reads of
// the pointwise kernels stride by cout and are served by the L2 (the whole network is 4.4 MB).  k_publish_split, behind
// it on the stream: one thread per 16-channel group of a folded array (64 contiguous bytes in, 2 x 32 contiguous bytes
// out, consecutive threads on consecutive output groups) writes the two float16 pieces and raises the layer's range
// flag.  The parameter and state buffers are only read.
#include <math.h>

#include "pp_common.h"

namespace {

constexpr int PUB_BLOCK = 256;

__device__ __forceinline__ const PubTask& find_task(const PubTask* tasks, int ntasks) {
    int lo = 0, hi = ntasks - 1;            // the last task whose first workgroup is <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tasks[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return tasks[lo];
}

// bn_fold of one channel: scale = gamma / sqrtf(var + 1e-3f), shift = beta - mean * scale
__device__ __forceinline__ float bn_scale(const PubTask& t, const float* params, const float* state, int c) {
    return params[t.gamma + c] / sqrtf(state[t.var + c] + 1e-3f);
}

// element (o, ci) of the [PP_HEAD_COLS][CC] head matrix: rows box | cls | dir | zero pad
__device__ __forceinline__ float head_w(const PubHead& h, const float* params, int o, int ci) {
    if (o < h.nb) return params[h.box_k + (long long)ci * h.nb + o];
    o -= h.nb;
    if (o < h.nc) return params[h.cls_k + (long long)ci * h.nc + o];
    o -= h.nc;
    if (o < h.nd) return params[h.dir_k + (long long)ci * h.nd + o];
    return 0.f;
}

__global__ __launch_bounds__(PUB_BLOCK) void k_publish_fold(const PubTask* __restrict__ tasks, int ntasks, PubHead hd,
                                                             const float* __restrict__ params,
                                                             const float* __restrict__ state) {
    const PubTask& t = find_task(tasks, ntasks);
    const int i = ((int)blockIdx.x - t.block0) * PUB_BLOCK + (int)threadIdx.x;
    if (i >= t.n) return;
    float v;
    switch (t.kind) {
    case PUB_PFN_W: {          // [FA][C] * scale[c]
        v = params[t.src + i] * bn_scale(t, params, state, i % t.cout);
        break;
    }
    case PUB_SHIFT: {          // [c]
        const float inv = bn_scale(t, params, state, i);
        v = params[t.beta + i] - state[t.mean + i] * inv;
        break;
    }
    case PUB_COPY:
        v = params[t.src + i];
        break;
    case PUB_SEP_WT: {         // out[co][ci] = pointwise[ci][co] * scale[co]
        const int co = i / t.cin, ci = i % t.cin;
        v = params[t.src + (long long)ci * t.cout + co] * bn_scale(t, params, state, co);
        break;
    }
    case PUB_DEC_WT: {         // out[n][ci] = k[n][ci] * scale[n % cout]
        const int n = i / t.cin;
        v = params[t.src + i] * bn_scale(t, params, state, n % t.cout);
        break;
    }
    case PUB_HEAD_WT: {        // out[o][c] = head[o][co_off + c]
        const int o = i / t.cout, c = i % t.cout;
        v = head_w(hd, params, o, t.co_off + c);
        break;
    }
    default: {                 // PUB_HEAD_BIAS [PP_HEAD_COLS]
        int o = i;
        if (o < hd.nb) v = params[hd.box_b + o];
        else if ((o -= hd.nb) < hd.nc) v = params[hd.cls_b + o];
        else if ((o -= hd.nc) < hd.nd) v = params[hd.dir_b + o];
        else v = 0.f;
        break;
    }
    }
    t.out[i] = v;
}

__device__ __forceinline__ unsigned f16_bits(_Float16 h) { return (unsigned)__builtin_bit_cast(unsigned short, h); }

// [cin / 16][PP_NPIECE][n_total][16] from wt [n_total][cin]; thread = (16-channel group kc, row n), n fastest
__global__ __launch_bounds__(PUB_BLOCK) void k_publish_split(const PubTask* __restrict__ tasks, int ntasks,
                                                              int* __restrict__ flags) {
    const PubTask& t = find_task(tasks, ntasks);
    const int i = ((int)blockIdx.x - t.block0) * PUB_BLOCK + (int)threadIdx.x;
    if (i >= t.n) return;
    const int kc = i / t.n_total, n = i % t.n_total;
    float w[16];
    if (t.kind == PUB_SPLIT) {
        const float4* src = reinterpret_cast<const float4*>(t.wt + (size_t)n * t.cin + (size_t)kc * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 x = src[q];
            w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w;
        }
    } else {
        // PUB_SPLIT_HEAD: the head slice in the accumulator-register order of the deconv kernels -- slot (h, j) of
        // 16-channel group (nn, g) holds channel nn*32 + (j&3) + 8*(2g + (j>>2)) + 4h
        const int nn = kc >> 1, g = kc & 1;
        const float* row = t.wt + (size_t)n * t.cin;
#pragma unroll
        for (int sl = 0; sl < 16; ++sl) {
            const int hh = sl >> 3, j = sl & 7;
            w[sl] = row[nn * 32 + (j & 3) + 8 * (2 * g + (j >> 2)) + 4 * hh];
        }
    }
    bool bad = false;
    unsigned hi[8], mid[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        unsigned ph[2], pm[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const float x = w[2 * q + r];
            bad = bad || !(fabsf(x) < 32768.f);
            const _Float16 hf = (_Float16)x;
            const _Float16 mf = (_Float16)(x - (float)hf);
            ph[r] = f16_bits(hf);
            pm[r] = f16_bits(mf);
        }
        hi[q] = ph[0] | (ph[1] << 16);
        mid[q] = pm[0] | (pm[1] << 16);
    }
    uint4* o0 = reinterpret_cast<uint4*>(t.out16 + (((size_t)kc * PP_NPIECE + 0) * t.n_total + n) * 16);
    uint4* o1 = reinterpret_cast<uint4*>(t.out16 + (((size_t)kc * PP_NPIECE + 1) * t.n_total + n) * 16);
    o0[0] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    o0[1] = make_uint4(hi[4], hi[5], hi[6], hi[7]);
    o1[0] = make_uint4(mid[0], mid[1], mid[2], mid[3]);
    o1[1] = make_uint4(mid[4], mid[5], mid[6], mid[7]);
    if (bad) atomicOr(&flags[t.flag], 1);      // f16_pair_range_ok failed for this array (NaN / inf included)
}

}  // namespace

int publish_blocks(int n) { return (n + PUB_BLOCK - 1) / PUB_BLOCK; }

void launch_publish_fold(const PubTask* tasks, int ntasks, int blocks, const PubHead& hd, const float* params,
                         const float* state, hipStream_t s) {
    if (ntasks < 1 || blocks < 1) return;
    PP_LAUNCH("k_publish_fold", k_publish_fold, dim3(blocks), dim3(PUB_BLOCK), 0, s, tasks, ntasks, hd, params, state);
}

void launch_publish_split(const PubTask* tasks, int ntasks, int blocks, int* flags, hipStream_t s) {
    if (ntasks < 1 || blocks < 1) return;
    PP_LAUNCH("k_publish_split", k_publish_split, dim3(blocks), dim3(PUB_BLOCK), 0, s, tasks, ntasks, flags);
}
