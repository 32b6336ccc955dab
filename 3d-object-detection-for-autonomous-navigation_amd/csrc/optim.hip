// AdamW parameter update (the reference's optimizer step, train.py:228-239, :301).
//
// The reference uses tfa.optimizers.AdamW (tensorflow-addons 0.11.2, configs/pip/requirements_short.txt:4) over
// tf.keras.optimizers.Adam (TensorFlow 2.2.0); neither is vendored.  Their published update for one variable:
//   var -= weight_decay * var                          (decoupled decay, applied first, NOT scaled by the rate)
//   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2
//   var -= lr_t * m / (sqrt(v) + epsilon),   lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t),  t = iterations + 1
// with lr from the ExponentialDecay schedule (host side, optim.py).  One flat float32 buffer per state:
// HBM-bound, 16 bytes read + 12 written per parameter, 16-byte accesses.
#include <string.h>

#include "pp_common.h"

__global__ __launch_bounds__(256) void k_adamw(float* __restrict__ w, const float* __restrict__ g,
                                               float* __restrict__ m, float* __restrict__ v, int64_t n,
                                               float lr_t, float beta1, float beta2, float eps, float wd) {
    const int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 >= n) return;
    float wv[4], gv[4], mv[4], vv[4];
    const bool full = i4 + 4 <= n;
    if (full) {
        const float4 a = *reinterpret_cast<const float4*>(w + i4), b = *reinterpret_cast<const float4*>(g + i4);
        const float4 c = *reinterpret_cast<const float4*>(m + i4), d = *reinterpret_cast<const float4*>(v + i4);
        wv[0] = a.x; wv[1] = a.y; wv[2] = a.z; wv[3] = a.w;
        gv[0] = b.x; gv[1] = b.y; gv[2] = b.z; gv[3] = b.w;
        mv[0] = c.x; mv[1] = c.y; mv[2] = c.z; mv[3] = c.w;
        vv[0] = d.x; vv[1] = d.y; vv[2] = d.z; vv[3] = d.w;
    } else {
        for (int k = 0; k < 4; ++k) {
            const bool ok = i4 + k < n;
            wv[k] = ok ? w[i4 + k] : 0.f; gv[k] = ok ? g[i4 + k] : 0.f;
            mv[k] = ok ? m[i4 + k] : 0.f; vv[k] = ok ? v[i4 + k] : 0.f;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float wd_w = __fsub_rn(wv[k], __fmul_rn(wd, wv[k]));
        mv[k] = __fadd_rn(__fmul_rn(beta1, mv[k]), __fmul_rn(1.f - beta1, gv[k]));
        vv[k] = __fadd_rn(__fmul_rn(beta2, vv[k]), __fmul_rn(1.f - beta2, __fmul_rn(gv[k], gv[k])));
        wv[k] = __fsub_rn(wd_w, __fdiv_rn(__fmul_rn(lr_t, mv[k]), __fadd_rn(__fsqrt_rn(vv[k]), eps)));
    }
    if (full) {
        *reinterpret_cast<float4*>(w + i4) = make_float4(wv[0], wv[1], wv[2], wv[3]);
        *reinterpret_cast<float4*>(m + i4) = make_float4(mv[0], mv[1], mv[2], mv[3]);
        *reinterpret_cast<float4*>(v + i4) = make_float4(vv[0], vv[1], vv[2], vv[3]);
    } else {
        for (int k = 0; k < 4; ++k)
            if (i4 + k < n) { w[i4 + k] = wv[k]; m[i4 + k] = mv[k]; v[i4 + k] = vv[k]; }
    }
}

void launch_adamw(float* w, const float* g, float* m, float* v, int64_t n, float lr_t, float beta1, float beta2,
                  float eps, float wd, hipStream_t s) {
    if (n <= 0) return;
    const int64_t blocks = (n + 1023) / 1024;
    hipLaunchKernelGGL(k_adamw, dim3((unsigned)blocks), dim3(256), 0, s, w, g, m, v, n, lr_t, beta1, beta2, eps, wd);
}

// The same update over the trainable part of the buffer only (frozen layers, trainer.py): `nseg` (offset, size)
// segments of it, in one launch per PP_ADAMW_SEGS segments; nothing outside them is read or written.  Per element the
// arithmetic is k_adamw's, operation for operation, so an updated entry is bit-identical to a full-buffer launch's.
// Segments need not start on a 16-byte boundary: a workgroup owns 1 024 consecutive floats of one segment and a thread
// every 256th of them (coalesced 4-byte accesses; the update stays HBM-bound).
int adamw_fill_table(AdamwSegs& t, const int64_t* seg, int nseg, int* done, int* src) {
    memset(&t, 0, sizeof(t));
    int blocks = 0;
    while (*done < nseg && t.n < PP_ADAMW_SEGS) {
        const int64_t size = seg[2 * *done + 1];
        if (size > 0) {
            t.off[t.n] = seg[2 * *done];
            t.size[t.n] = size;
            t.block_start[t.n] = blocks;
            if (src) src[t.n] = *done;
            blocks += (int)((size + 1023) / 1024);
            ++t.n;
        }
        ++*done;
    }
    for (int k = t.n; k <= PP_ADAMW_SEGS; ++k) t.block_start[k] = blocks;
    return blocks;
}

// (k_adamw_seg_clip in grad_clip.hip is this kernel on a clipped gradient: same table, same map, same operations --
// a change here belongs there, too; tests/test_gpu_grad_clip.py holds the two to bit-identity)
__global__ __launch_bounds__(256) void k_adamw_seg(float* __restrict__ w, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, AdamwSegs t,
                                                   float lr_t, float beta1, float beta2, float eps, float wd) {
    int j = 0;
    while (j + 1 < t.n && (int)blockIdx.x >= t.block_start[j + 1]) ++j;     // uniform
    const int64_t base = ((int64_t)blockIdx.x - t.block_start[j]) * 1024;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t e = base + k * 256 + threadIdx.x;
        if (e >= t.size[j]) break;
        const int64_t i = t.off[j] + e;
        const float wv = w[i], gv = g[i];
        float mv = m[i], vv = v[i];
        const float wd_w = __fsub_rn(wv, __fmul_rn(wd, wv));
        mv = __fadd_rn(__fmul_rn(beta1, mv), __fmul_rn(1.f - beta1, gv));
        vv = __fadd_rn(__fmul_rn(beta2, vv), __fmul_rn(1.f - beta2, __fmul_rn(gv, gv)));
        w[i] = __fsub_rn(wd_w, __fdiv_rn(__fmul_rn(lr_t, mv), __fadd_rn(__fsqrt_rn(vv), eps)));
        m[i] = mv;
        v[i] = vv;
    }
}

void launch_adamw_segments(float* w, const float* g, float* m, float* v, const int64_t* seg, int nseg, float lr_t,
                           float beta1, float beta2, float eps, float wd, hipStream_t s) {
    for (int done = 0; done < nseg;) {
        AdamwSegs t;
        const int blocks = adamw_fill_table(t, seg, nseg, &done, nullptr);
        if (blocks > 0)
            PP_LAUNCH("k_adamw_seg", k_adamw_seg, dim3((unsigned)blocks), dim3(256), 0, s, w, g, m, v, t, lr_t, beta1,
                      beta2, eps, wd);
    }
}
