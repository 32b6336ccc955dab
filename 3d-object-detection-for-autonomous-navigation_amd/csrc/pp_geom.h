// Box geometry shared by the augmentation (augment.hip) and the GT-database sampling (gt_sample.hip): float64, in the
// reference's operation order (the build has -ffp-contract=off).
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ void rot2(double px, double py, double c, double s, double& ox, double& oy) {
    // [px, py] @ [[c, -s], [s, c]]
    ox = px * c + py * s;
    oy = px * (-s) + py * c;
}

// box2d_to_corner_jit (load_data.py:1187-1205): corners_norm (-.5,-.5) (-.5,.5) (.5,.5) (.5,-.5)
__device__ __forceinline__ void corners2(double x, double y, double w, double l, double yaw, double* cx, double* cy) {
    const double c = cos(yaw), s = sin(yaw);
    const double nx[4] = {-0.5, -0.5, 0.5, 0.5}, ny[4] = {-0.5, 0.5, 0.5, -0.5};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double ox, oy;
        rot2(w * nx[k], l * ny[k], c, s, ox, oy);
        cx[k] = ox + x;
        cy[k] = oy + y;
    }
}

// box_collision_test as executed (augment.py): standup overlap and a proper crossing of two edges
__device__ __forceinline__ bool collide(const double* ax, const double* ay, const double* bx, const double* by) {
    double a0x = ax[0], a1x = ax[0], a0y = ay[0], a1y = ay[0], b0x = bx[0], b1x = bx[0], b0y = by[0], b1y = by[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        a0x = fmin(a0x, ax[k]); a1x = fmax(a1x, ax[k]); a0y = fmin(a0y, ay[k]); a1y = fmax(a1y, ay[k]);
        b0x = fmin(b0x, bx[k]); b1x = fmax(b1x, bx[k]); b0y = fmin(b0y, by[k]); b1y = fmax(b1y, by[k]);
    }
    const double iw = fmin(a1x, b1x) - fmax(a0x, b0x);
    if (!(iw > 0.0)) return false;
    const double ih = fmin(a1y, b1y) - fmax(a0y, b0y);
    if (!(ih > 0.0)) return false;
    for (int k = 0; k < 4; ++k) {
        const double Ax = ax[k], Ay = ay[k], Bx = ax[(k + 1) & 3], By = ay[(k + 1) & 3];
        for (int m = 0; m < 4; ++m) {
            const double Cx = bx[m], Cy = by[m], Dx = bx[(m + 1) & 3], Dy = by[(m + 1) & 3];
            const bool acd = (Dy - Ay) * (Cx - Ax) > (Cy - Ay) * (Dx - Ax);
            const bool bcd = (Dy - By) * (Cx - Bx) > (Cy - By) * (Dx - Bx);
            if (acd != bcd) {
                const bool abc = (Cy - Ay) * (Bx - Ax) > (By - Ay) * (Cx - Ax);
                const bool abd = (Dy - Ay) * (Bx - Ax) > (By - Ay) * (Dx - Ax);
                if (abc != abd) return true;
            }
        }
    }
    return false;
}

// Plane equations of a 3-D box q (x y z w l h r): center_to_corner_box3d(origin [.5, .5, 0], axis 2),
// corner_to_surfaces_3d_jit, surface_equ_3d_jit; a point is outside when p . n + d >= 0 for some face
__device__ __forceinline__ void box_planes3(const double* q, double (*n)[3], double* d) {
    const double nx3[8] = {-0.5, -0.5, -0.5, -0.5, 0.5, 0.5, 0.5, 0.5};
    const double ny3[8] = {-0.5, -0.5, 0.5, 0.5, -0.5, -0.5, 0.5, 0.5};
    const double nz3[8] = {0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0};
    const int faces[6][3] = {{0, 1, 2}, {7, 6, 5}, {0, 3, 7}, {1, 5, 6}, {0, 4, 5}, {3, 2, 6}};
    double c3[8][3];
    const double c = cos(q[6]), s = sin(q[6]);
    for (int k = 0; k < 8; ++k) {
        double rx, ry;
        rot2(q[3] * nx3[k], q[4] * ny3[k], c, s, rx, ry);
        c3[k][0] = rx + q[0];
        c3[k][1] = ry + q[1];
        c3[k][2] = q[5] * nz3[k] + q[2];
    }
    for (int f = 0; f < 6; ++f) {
        const double* s0 = c3[faces[f][0]];
        const double* s1 = c3[faces[f][1]];
        const double* s2 = c3[faces[f][2]];
        const double v0[3] = {s0[0] - s1[0], s0[1] - s1[1], s0[2] - s1[2]};
        const double v1[3] = {s1[0] - s2[0], s1[1] - s2[1], s1[2] - s2[2]};
        const double n0 = v0[1] * v1[2] - v0[2] * v1[1];
        const double n1 = v0[2] * v1[0] - v0[0] * v1[2];
        const double n2 = v0[0] * v1[1] - v0[1] * v1[0];
        n[f][0] = n0; n[f][1] = n1; n[f][2] = n2;
        d[f] = -((n0 * s0[0] + n1 * s0[1]) + n2 * s0[2]);
    }
}

}  // namespace
