// Device functions of the rotated-rectangle overlap, shared by the AP evaluator's k_riou_pairs (rotate_iou.hip), the
// rotated NMS (rotate_nms.hip) and the detector's rotated-NMS mode (postprocess.hip).
//
// The reference's rbbox_to_corners / quadrilateral_intersection / sort_vertex_in_convex_polygon / area
// (second/core/non_max_suppression/nms_gpu.py:180-407), float32 in the reference's operation order (no contraction: the
// library is built with -ffp-contract=off); cos / sin / sqrt are evaluated in double and rounded, like math.cos on a
// float32 scalar.  The clip is NOT symmetric bit for bit: c1 is the first argument of devRotateIoU / devRotateIoUEval.
//
// The per-thread polygon (<= RIOU_MAXP points) and its sort keys live in LDS in a [slot][thread] layout: three float
// arrays of RIOU_MAXP * STRIDE words, thread t using column t (dynamic indexing of a private array would go to scratch
// memory; this layout is bank-conflict free).  The reference's int_pts array holds 8 points; a pair that produced more
// (possible only through duplicated corner hits, e.g. identical boxes that also report edge crossings) would index out
// of bounds there -- here the extra points are dropped.
#pragma once

#include "pp_common.h"

#define RIOU_MAXP 8

// corners[0..7] = the four corners (x, y) of [centre x, centre y, x size, y size, angle], corners[8] = its area
__device__ __forceinline__ void riou_box_corners(float cx, float cy, float xd, float yd, float angle, float* c) {
    const float a_cos = (float)cos((double)angle), a_sin = (float)sin((double)angle);
    const float px[4] = {-xd / 2, -xd / 2, xd / 2, xd / 2};
    const float py[4] = {-yd / 2, yd / 2, yd / 2, -yd / 2};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[2 * j] = __fadd_rn(__fadd_rn(__fmul_rn(a_cos, px[j]), __fmul_rn(a_sin, py[j])), cx);
        c[2 * j + 1] = __fadd_rn(__fadd_rn(__fmul_rn(-a_sin, px[j]), __fmul_rn(a_cos, py[j])), cy);
    }
    c[8] = __fmul_rn(xd, yd);
}

__device__ __forceinline__ bool riou_in_quad(float x, float y, const float (&c)[8]) {
    const float ab0 = c[2] - c[0], ab1 = c[3] - c[1];
    const float ad0 = c[6] - c[0], ad1 = c[7] - c[1];
    const float ap0 = x - c[0], ap1 = y - c[1];
    const float abab = __fadd_rn(__fmul_rn(ab0, ab0), __fmul_rn(ab1, ab1));
    const float abap = __fadd_rn(__fmul_rn(ab0, ap0), __fmul_rn(ab1, ap1));
    const float adad = __fadd_rn(__fmul_rn(ad0, ad0), __fmul_rn(ad1, ad1));
    const float adap = __fadd_rn(__fmul_rn(ad0, ap0), __fmul_rn(ad1, ap1));
    return abab >= abap && abap >= 0.f && adad >= adap && adap >= 0.f;
}

// Area of the intersection of the quadrilaterals c1 (first argument) and c2.  s_px / s_py / s_vs: the LDS scratch
// described above, [RIOU_MAXP][STRIDE] floats each; t < STRIDE: this thread's column.
template <int STRIDE>
__device__ __forceinline__ float riou_clip_area(const float (&c1)[8], const float (&c2)[8], float* __restrict__ s_px,
                                                float* __restrict__ s_py, float* __restrict__ s_vs, int t) {
    int np = 0;
#define RIOU_PUSH(X, Y) { if (np < RIOU_MAXP) { s_px[np * STRIDE + t] = (X); s_py[np * STRIDE + t] = (Y); } ++np; }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (riou_in_quad(c1[2 * i], c1[2 * i + 1], c2)) RIOU_PUSH(c1[2 * i], c1[2 * i + 1])
        if (riou_in_quad(c2[2 * i], c2[2 * i + 1], c1)) RIOU_PUSH(c2[2 * i], c2[2 * i + 1])
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float A0 = c1[2 * i], A1 = c1[2 * i + 1], B0 = c1[2 * ((i + 1) & 3)], B1 = c1[2 * ((i + 1) & 3) + 1];
        const float BA0 = B0 - A0, BA1 = B1 - A1;
        const float ABBA = __fsub_rn(__fmul_rn(A0, B1), __fmul_rn(B0, A1));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float C0 = c2[2 * j], C1 = c2[2 * j + 1], D0 = c2[2 * ((j + 1) & 3)], D1 = c2[2 * ((j + 1) & 3) + 1];
            const float DA0 = D0 - A0, CA0 = C0 - A0, DA1 = D1 - A1, CA1 = C1 - A1;
            const bool acd = __fmul_rn(DA1, CA0) > __fmul_rn(CA1, DA0);
            const bool bcd = __fmul_rn(D1 - B1, C0 - B0) > __fmul_rn(C1 - B1, D0 - B0);
            if (acd != bcd) {
                const bool abc = __fmul_rn(CA1, BA0) > __fmul_rn(BA1, CA0);
                const bool abd = __fmul_rn(DA1, BA0) > __fmul_rn(BA1, DA0);
                if (abc != abd) {
                    const float DC0 = D0 - C0, DC1 = D1 - C1;
                    const float CDDC = __fsub_rn(__fmul_rn(C0, D1), __fmul_rn(D0, C1));
                    const float DH = __fsub_rn(__fmul_rn(BA1, DC0), __fmul_rn(BA0, DC1));
                    const float Dx = __fsub_rn(__fmul_rn(ABBA, DC0), __fmul_rn(BA0, CDDC));
                    const float Dy = __fsub_rn(__fmul_rn(ABBA, DC1), __fmul_rn(BA1, CDDC));
                    RIOU_PUSH(__fdiv_rn(Dx, DH), __fdiv_rn(Dy, DH))
                }
            }
        }
    }
#undef RIOU_PUSH
    if (np > RIOU_MAXP) np = RIOU_MAXP;
    float area = 0.f;
    if (np > 0) {
        float cx = 0.f, cy = 0.f;
        for (int i = 0; i < np; ++i) { cx = __fadd_rn(cx, s_px[i * STRIDE + t]); cy = __fadd_rn(cy, s_py[i * STRIDE + t]); }
        cx = __fdiv_rn(cx, (float)np);
        cy = __fdiv_rn(cy, (float)np);
        for (int i = 0; i < np; ++i) {
            float v0 = s_px[i * STRIDE + t] - cx, v1 = s_py[i * STRIDE + t] - cy;
            const float d = (float)sqrt((double)__fadd_rn(__fmul_rn(v0, v0), __fmul_rn(v1, v1)));
            v0 = __fdiv_rn(v0, d);
            v1 = __fdiv_rn(v1, d);
            if (v1 < 0.f) v0 = -2.f - v0;
            s_vs[i * STRIDE + t] = v0;
        }
        for (int i = 1; i < np; ++i) {
            if (s_vs[(i - 1) * STRIDE + t] > s_vs[i * STRIDE + t]) {
                const float temp = s_vs[i * STRIDE + t], tx = s_px[i * STRIDE + t], ty = s_py[i * STRIDE + t];
                int j = i;
                while (j > 0 && s_vs[(j - 1) * STRIDE + t] > temp) {
                    s_vs[j * STRIDE + t] = s_vs[(j - 1) * STRIDE + t];
                    s_px[j * STRIDE + t] = s_px[(j - 1) * STRIDE + t];
                    s_py[j * STRIDE + t] = s_py[(j - 1) * STRIDE + t];
                    --j;
                }
                s_vs[j * STRIDE + t] = temp;
                s_px[j * STRIDE + t] = tx;
                s_py[j * STRIDE + t] = ty;
            }
        }
        const float a0 = s_px[t], a1 = s_py[t];
        for (int i = 0; i < np - 2; ++i) {
            const float b0 = s_px[(i + 1) * STRIDE + t], b1 = s_py[(i + 1) * STRIDE + t];
            const float q0 = s_px[(i + 2) * STRIDE + t], q1 = s_py[(i + 2) * STRIDE + t];
            const float tri = __fsub_rn(__fmul_rn(a0 - q0, b1 - q1), __fmul_rn(a1 - q1, b0 - q0)) / 2.0f;
            area = __fadd_rn(area, fabsf(tri));
        }
    }
    return area;
}

// devRotateIoU: c1 / area1 belong to the FIRST argument
template <int STRIDE>
__device__ __forceinline__ float riou_iou(const float (&c1)[8], float area1, const float (&c2)[8], float area2,
                                          float* __restrict__ s_px, float* __restrict__ s_py, float* __restrict__ s_vs, int t) {
    const float area = riou_clip_area<STRIDE>(c1, c2, s_px, s_py, s_vs, t);
    return __fdiv_rn(area, __fsub_rn(__fadd_rn(area1, area2), area));
}
