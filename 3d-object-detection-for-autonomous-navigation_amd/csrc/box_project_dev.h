// Image box of one camera-frame 3D box: box3d_to_bbox of second/core/box_np_ops.py:849-857 (corners_nd :170-201,
// rotation_3d_in_axis :259-277, project_to_image :605-611) in float64.  Shared by the tail of k_postprocess and by
// k_box3d_to_bbox (box_project.hip): one function, so the two give the same bits on the same seven doubles.
//
// The reference's quirks are kept (projection.py states the rule): the origin of a box is its bottom face centre; the
// zero terms of the rotation matrix are multiplied out (they decide the sign of a zero result and make inf * 0 = NaN
// as the einsum does); project_to_image appends zeros as the homogeneous coordinate, so only the left 3 x 3 of P2
// enters; min / max propagate NaN as np.min / np.max do; nothing clips, nothing treats w' <= 0.
#pragma once

#include <hip/hip_runtime.h>

// box: x y z l h w ry.  P: rows 0..2, columns 0..2 of P2, row-major [9].  out: min u, min v, max u, max v.
__device__ __forceinline__ void box3d_to_bbox_dev(const double* box, const double* P, double* out) {
#pragma clang fp contract(off)      // every product rounds on its own, wherever this is inlined: same bits in both kernels
    double s, c;
    sincos(box[6], &s, &c);
    const double ns = -s;
    double u0 = 0.0, v0 = 0.0, u1 = 0.0, v1 = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        // corners_nd's order: (ux, uy, uz) = unravel(k) reordered by [0, 1, 3, 2, 4, 5, 7, 6]; min / max do not depend on it
        const double x = box[3] * ((k & 4) ? 0.5 : -0.5);
        const double y = box[4] * ((k & 2) ? 0.0 : -1.0);
        const double z = box[5] * ((((k >> 1) ^ k) & 1) ? 0.5 : -0.5);
        const double X = (x * c + y * 0.0 + z * s) + box[0];
        const double Y = (x * 0.0 + y * 1.0 + z * 0.0) + box[1];
        const double Z = (x * ns + y * 0.0 + z * c) + box[2];
        const double wn = X * P[6] + Y * P[7] + Z * P[8];
        const double u = (X * P[0] + Y * P[1] + Z * P[2]) / wn;
        const double v = (X * P[3] + Y * P[4] + Z * P[5]) / wn;
        if (k == 0) { u0 = u1 = u; v0 = v1 = v; }
        else {      // a NaN enters and then stays: every comparison with it is false
            u0 = (u < u0 || u != u) ? u : u0;
            u1 = (u > u1 || u != u) ? u : u1;
            v0 = (v < v0 || v != v) ? v : v0;
            v1 = (v > v1 || v != v) ? v : v1;
        }
    }
    out[0] = u0; out[1] = v0; out[2] = u1; out[3] = v1;
}
