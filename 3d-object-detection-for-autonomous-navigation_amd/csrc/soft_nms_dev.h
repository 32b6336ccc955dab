// Soft-NMS: soft_nms_jit of second/core/non_max_suppression/nms_cpu.py:79-169 (compiled and exported by the reference,
// never called), shared by k_soft_nms (soft_nms.hip) and by the PP_NMS_SOFT instantiation of k_postprocess
// (postprocess.hip): one re-scoring function and one round loop, so the two cannot drift.
//
// The rule, with numba's typing (float32 meeting an integer literal becomes float64, as in iou_device): every round
// selects the alive, unselected box with the largest current score -- its score is final -- and re-scores every other
// alive box j that overlaps it under the `+1` pixel convention:
//   iw = (double)(min(tx2, x2) - max(tx1, x1)) + 1          (the difference in float32), ih likewise; both must be > 0
//   ua = ((double)(tx2 - tx1) + 1) * ((double)(ty2 - ty1) + 1) + ((double)(x2 - x1) + 1) * ((double)(y2 - y1) + 1) - iw * ih
//   ov = iw * ih / ua                                       (the stand-up rule's inter / (sa + sb - inter), same order)
//   weight: hard ov > Nt ? 0 : 1; linear ov > Nt ? 1 - ov : 1; Gaussian exp(-(ov * ov) / sigma)
//   score_j = (float)(weight * (double)score_j); score_j < floor (float32): box j dies
// The floor is checked only where a box was re-scored (weight 1 included): a box below the floor that overlaps no
// selected box is kept.  Equal current scores: the lower index wins (the reference decides by array slot after its
// in-place swaps, which is not reproduced).  No floating-point atomics; the same input gives the same bytes.
#pragma once

#include <hip/hip_runtime.h>

#define SNMS_NONE 0x7fffffff     // "no candidate" index of the argmax

// the re-scored value of box (x1, y1, x2, y2, s) against the selected box t; hit: the overlap branch was taken
__device__ __forceinline__ float snms_rescore(float tx1, float ty1, float tx2, float ty2, float x1, float y1, float x2,
                                              float y2, float s, int method, double nt, double sigma, bool& hit) {
#pragma clang fp contract(off)      // ua never becomes an FMA, wherever this is inlined
    hit = false;
    const double iw = (double)(fminf(tx2, x2) - fmaxf(tx1, x1)) + 1.0;
    if (!(iw > 0.0)) return s;
    const double ih = (double)(fminf(ty2, y2) - fmaxf(ty1, y1)) + 1.0;
    if (!(ih > 0.0)) return s;
    const double area = ((double)(x2 - x1) + 1.0) * ((double)(y2 - y1) + 1.0);
    const double inter = iw * ih;
    const double ua = ((double)(tx2 - tx1) + 1.0) * ((double)(ty2 - ty1) + 1.0) + area - inter;
    const double ov = inter / ua;
    double w;
    if (method == 1) w = (ov > nt) ? 1.0 - ov : 1.0;
    else if (method == 2) w = exp(-(ov * ov) / sigma);
    else w = (ov > nt) ? 0.0 : 1.0;
    hit = true;
    return (float)(w * (double)s);
}

// the better of two (score, index) candidates on every lane: larger score, lower index on ties; the order is total, so
// the xor butterfly over `width` lanes (a power of two) leaves each of them with the same winner
__device__ __forceinline__ void snms_best(float& v, int& idx, int width) {
    for (int m = width >> 1; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(v, m, 64);
        const int oi = __shfl_xor(idx, m, 64);
        const bool take = oi != SNMS_NONE && (idx == SNMS_NONE || ov > v || (ov == v && oi < idx));
        if (take) { v = ov; idx = oi; }
    }
}

// The rounds over boxes 0 .. n-1 (box [n][4] and score [n] in LDS, n <= NT * PER) by NT threads -- every thread of the
// NT calls this, NT = 64 (one wavefront, no barrier) or a whole workgroup of NT = 64 * 2^k <= 1024 threads.  Thread t
// keeps boxes t, t + NT, ... and their current scores in registers.  Per round: argmax (wavefront butterfly, then across
// the wavefronts through s_red, double-buffered: one barrier per round), the selected box's corners by a broadcast read
// of LDS, every thread decays its own boxes.  emit(round, index, final score) is called by the thread that owns the
// selected box.  Stops after post_max selections or when nothing is alive; returns the number of selections.
template <int NT, int PER, typename Emit>
__device__ __forceinline__ int snms_rounds(const float (*box)[4], const float* score, int n, int post_max, int method,
                                           float nt, float sigma, float score_floor, int tid, float (*s_red_v)[NT / 64],
                                           int (*s_red_i)[NT / 64], Emit&& emit) {
    static_assert(NT % 64 == 0 && (NT / 64 & (NT / 64 - 1)) == 0 && NT <= 1024, "NT: 64 * 2^k threads");
    constexpr int NW = NT / 64;
    float bx[PER][4], sc[PER];
    bool live[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = tid + k * NT;
        live[k] = i < n;
        sc[k] = live[k] ? score[i] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) bx[k][q] = live[k] ? box[i][q] : 0.f;
    }
    const double dnt = (double)nt, dsig = (double)sigma;
    int nk = 0;
    while (nk < post_max) {
        float v = 0.f;
        int idx = SNMS_NONE;
#pragma unroll
        for (int k = 0; k < PER; ++k)       // ascending index: a later equal score does not replace an earlier one
            if (live[k] && (idx == SNMS_NONE || sc[k] > v)) { v = sc[k]; idx = tid + k * NT; }
        snms_best(v, idx, 64);
        if constexpr (NW > 1) {
            const int buf = nk & 1;
            if ((tid & 63) == 0) { s_red_v[buf][tid >> 6] = v; s_red_i[buf][tid >> 6] = idx; }
            __syncthreads();
            v = s_red_v[buf][tid & (NW - 1)];
            idx = s_red_i[buf][tid & (NW - 1)];
            snms_best(v, idx, NW);
        }
        if (idx == SNMS_NONE) break;        // (the same on every thread)
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (idx == tid + k * NT) { live[k] = false; emit(nk, idx, sc[k]); }
        ++nk;
        const float tx1 = box[idx][0], ty1 = box[idx][1], tx2 = box[idx][2], ty2 = box[idx][3];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (!live[k]) continue;
            bool hit;
            const float r = snms_rescore(tx1, ty1, tx2, ty2, bx[k][0], bx[k][1], bx[k][2], bx[k][3], sc[k], method, dnt,
                                         dsig, hit);
            if (hit) { sc[k] = r; if (r < score_floor) live[k] = false; }
        }
    }
    return nk;
}
