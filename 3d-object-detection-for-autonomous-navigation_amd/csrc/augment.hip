// Training-time augmentation of the resident frames and their ground-truth boxes: the
// reference's prep_pointcloud training branch after GT-database sampling (load_data.py:2751-2866), restated in
// augment.py (augment_np), whose docstring lists the stages and the collision rule as the reference executes it.
// The random numbers are drawn on the host (augment.draw); everything here is decided in float64 in the reference's
// operation order (the build has -ffp-contract=off), and point coordinates are rounded to float32 once, on store.
//
// k_aug_select   a workgroup per frame: the frame's 2-D box corners in LDS; the valid boxes are walked in order, a lane
//                per try; the first try whose moved corners collide with no other box's current corners wins and
//                replaces that box's corners before the next box (noise_per_box / noise_per_box_v2_).  Then a thread
//                per box: the plane equations of the ORIGINAL 3-D box for the point pass, and the box's own stages
//                (transform, flip, rotation, scale, translation, limit_period, centre filter) with its keep flag.
// k_aug_points   a thread per output point i: input point perm[i] of its frame (aug_perm: the shuffle), moved by the
//                first valid box that contains it, then flipped, rotated, scaled and translated; features ride along.
// k_aug_compact  a workgroup per frame: the kept boxes and classes, in order, behind the frames before.
#include <math.h>

#include "pp_common.h"
#include "pp_geom.h"

namespace {

constexpr int kSelThreads = 128;   // >= PP_AUG_MAX_TRY: one lane per try

__device__ __forceinline__ int frame_start(const int* cnt, int b) {
    int g0 = 0;
    for (int i = 0; i < b; ++i) g0 += cnt[i];
    return g0;
}

// the box's stages 1-7 and the centre filter, float64 (augment_np)
__device__ void box_stages(const AugParams& p, const AugFrame& fr, const double* q, bool valid, const double* tr,
                           double* o, bool* keep) {
    for (int k = 0; k < 7; ++k) o[k] = q[k];
    if (valid) {
        o[0] += tr[0]; o[1] += tr[1]; o[2] += tr[2];
        o[6] += tr[3];
    }
    if (fr.flip) { o[1] = -o[1]; o[6] = -o[6]; }
    const double c = cos(fr.theta), s = sin(fr.theta);
    double x, y;
    rot2(o[0], o[1], c, s, x, y);
    o[0] = x; o[1] = y;
    o[6] += fr.theta;
    for (int k = 0; k < 6; ++k) o[k] *= fr.scale;
    o[0] += fr.t[0]; o[1] += fr.t[1]; o[2] += fr.t[2];
    const double tp = 6.283185307179586;   // 2 * np.pi
    o[6] = o[6] - floor(o[6] / tp + 0.5) * tp;
    // points_in_convex_polygon_jit against minmax_to_corner_2d(pc_range[[0, 1, 3, 4]]), clockwise
    const double x0 = p.pc[0], y0 = p.pc[1], wx = p.pc[2] - p.pc[0], wy = p.pc[3] - p.pc[1];
    const double px[4] = {x0 + wx * 0.0, x0 + wx * 0.0, x0 + wx * 1.0, x0 + wx * 1.0};
    const double py[4] = {y0 + wy * 0.0, y0 + wy * 1.0, y0 + wy * 1.0, y0 + wy * 0.0};
    bool in = valid;
    for (int k = 0; k < 4; ++k) {
        const int km = (k + 3) & 3;
        const double vx = px[k] - px[km], vy = py[k] - py[km];
        const double cross = vy * (px[k] - o[0]) - vx * (py[k] - o[1]);
        if (cross >= 0.0) in = false;
    }
    *keep = in;
}

__global__ __launch_bounds__(kSelThreads) void k_aug_select(AugParams p) {
    __shared__ double cx[PP_MAX_GT_PER_FRAME][4], cy[PP_MAX_GT_PER_FRAME][4];
    __shared__ double tr[PP_MAX_GT_PER_FRAME][4];
    __shared__ int s_sel[PP_MAX_GT_PER_FRAME];
    __shared__ int s_best, s_kept;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int G = p.cnt_in[b];
    const int g0 = frame_start(p.cnt_in, b);
    const int d0 = p.draw_off ? p.draw_off[b] : g0;
    const AugFrame fr = p.frames[b];
    for (int g = tid; g < G; g += kSelThreads) {
        const float* q = p.gt_in + (size_t)(g0 + g) * 7;
        corners2(q[0], q[1], q[3], q[4], q[6], cx[g], cy[g]);
        tr[g][0] = tr[g][1] = tr[g][2] = tr[g][3] = 0.0;
        s_sel[g] = -1;
    }
    if (tid == 0) {
        s_kept = 0;
        p.frame_cs[2 * b] = cos(fr.theta);
        p.frame_cs[2 * b + 1] = sin(fr.theta);
    }
    __syncthreads();
    const int T = p.T;
    for (int i = 0; i < G; ++i) {
        if (p.valid && p.valid[g0 + i] == 0) continue;    // uniform across the workgroup
        if (tid == 0) s_best = T;
        __syncthreads();
        const float* q = p.gt_in + (size_t)(g0 + i) * 7;
        const double x = q[0], y = q[1], w = q[3], l = q[4], yaw = q[6];
        double ax[4], ay[4], ddx = 0.0, ddy = 0.0, drot = 0.0;
        const int j = tid;
        if (j < T) {
            const double* d = p.draws + ((size_t)(d0 + i) * T + j) * 5;
            double px = x, py = y;
            if (p.v2) {
                const double radius = sqrt(x * x + y * y);
                const double cg = atan2(x, y);
                const double dg = cg + d[4];
                px = radius * sin(dg);
                py = radius * cos(dg);
                corners2(px, py, w, l, yaw + (dg - cg), ax, ay);
                ddx = px - x; ddy = py - y; drot = dg - cg;
            } else {
                for (int k = 0; k < 4; ++k) { ax[k] = cx[i][k]; ay[k] = cy[i][k]; }
            }
            const double c = cos(d[3]), s = sin(d[3]);
            const double ox = px + d[0], oy = py + d[1];
            for (int k = 0; k < 4; ++k) {
                double rx, ry;
                rot2(ax[k] - px, ay[k] - py, c, s, rx, ry);
                ax[k] = rx + ox;
                ay[k] = ry + oy;
            }
            bool hit = false;
            for (int k = 0; k < G && !hit; ++k)
                if (k != i) hit = collide(ax, ay, cx[k], cy[k]);
            if (!hit) atomicMin(&s_best, j);
        }
        __syncthreads();
        if (j < T && j == s_best) {
            const double* d = p.draws + ((size_t)(d0 + i) * T + j) * 5;
            for (int k = 0; k < 4; ++k) { cx[i][k] = ax[k]; cy[i][k] = ay[k]; }
            tr[i][0] = d[0] + ddx;
            tr[i][1] = d[1] + ddy;
            tr[i][2] = d[2];
            tr[i][3] = d[3] + drot;
            s_sel[i] = j;
        }
        __syncthreads();
    }
    for (int g = tid; g < G; g += kSelThreads) {
        const float* qf = p.gt_in + (size_t)(g0 + g) * 7;
        double q[7];
        for (int k = 0; k < 7; ++k) q[k] = qf[k];
        const bool valid = p.valid == nullptr || p.valid[g0 + g] != 0;
        AugBox& r = p.boxrec[(size_t)b * PP_MAX_GT_PER_FRAME + g];
        box_planes3(q, r.n, r.d);
        r.c[0] = q[0]; r.c[1] = q[1]; r.c[2] = q[2];
        r.loc[0] = tr[g][0]; r.loc[1] = tr[g][1]; r.loc[2] = tr[g][2];
        r.cr = cos(tr[g][3]); r.sr = sin(tr[g][3]);
        r.valid = valid ? 1 : 0;
        if (p.sel) p.sel[g0 + g] = s_sel[g];
        double o[7];
        bool keep;
        box_stages(p, fr, q, valid, tr[g], o, &keep);
        float* ob = p.box_tmp + ((size_t)b * PP_MAX_GT_PER_FRAME + g) * 7;
        for (int k = 0; k < 7; ++k) ob[k] = (float)o[k];
        p.keep[(size_t)b * PP_MAX_GT_PER_FRAME + g] = keep ? 1 : 0;
        if (keep) atomicAdd(&s_kept, 1);
    }
    __syncthreads();
    if (tid == 0) p.cnt_out[b] = s_kept;
}

__device__ __forceinline__ unsigned mix32(unsigned x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// augment.shuffle_perm: a 4-round Feistel network over 2^(2h) >= n values, cycle-walked into [0, n)
__device__ __forceinline__ unsigned aug_perm(unsigned seed, unsigned n, unsigned i) {
    const int bits = n > 1 ? 32 - __clz((int)(n - 1)) : 1;
    const int h = (bits + 1) / 2;
    const unsigned mask = (1u << h) - 1u;
    unsigned key[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) key[r] = mix32(seed ^ (0x9E3779B9u * (unsigned)(r + 1)));
    unsigned x = i;
    do {
        unsigned L = x >> h, R = x & mask;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned nr = L ^ (mix32(R ^ key[r]) & mask);
            L = R;
            R = nr;
        }
        x = (L << h) | R;
    } while (x >= n);
    return x;
}

__global__ __launch_bounds__(256) void k_aug_points(AugParams p) {
    const int b = blockIdx.y;
    const int o0 = p.offsets[b];
    const int n = p.offsets[b + 1] - o0;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const AugFrame fr = p.frames[b];
    const unsigned src = aug_perm(fr.seed, (unsigned)n, (unsigned)i);
    const float* in = p.pts_in + ((size_t)o0 + src) * p.F;
    double x = in[0], y = in[1], z = in[2];
    const int G = p.cnt_in[b];
    const AugBox* rec = p.boxrec + (size_t)b * PP_MAX_GT_PER_FRAME;
    for (int g = 0; g < G; ++g) {
        const AugBox& r = rec[g];
        if (!r.valid) continue;
        bool inside = true;
        for (int f = 0; f < 6 && inside; ++f)
            if (((x * r.n[f][0] + y * r.n[f][1]) + z * r.n[f][2]) + r.d[f] >= 0.0) inside = false;
        if (inside) {
            double rx, ry;
            rot2(x - r.c[0], y - r.c[1], r.cr, r.sr, rx, ry);
            const double rz = z - r.c[2];
            x = (rx + r.c[0]) + r.loc[0];
            y = (ry + r.c[1]) + r.loc[1];
            z = (rz + r.c[2]) + r.loc[2];
            break;
        }
    }
    if (fr.flip) y = -y;
    const double c = p.frame_cs[2 * b], s = p.frame_cs[2 * b + 1];
    double rx, ry;
    rot2(x, y, c, s, rx, ry);
    x = rx * fr.scale + fr.t[0];
    y = ry * fr.scale + fr.t[1];
    z = z * fr.scale + fr.t[2];
    float* out = p.pts_out + ((size_t)o0 + i) * p.F;
    out[0] = (float)x;
    out[1] = (float)y;
    out[2] = (float)z;
    for (int k = 3; k < p.F; ++k) out[k] = in[k];
}

__global__ __launch_bounds__(256) void k_aug_compact(AugParams p) {
    const int b = blockIdx.x;
    const int G = p.cnt_in[b];
    const int g0 = frame_start(p.cnt_in, b);
    const int o0 = frame_start(p.cnt_out, b);
    const uint8_t* keep = p.keep + (size_t)b * PP_MAX_GT_PER_FRAME;
    for (int g = threadIdx.x; g < G; g += 256) {
        if (!keep[g]) continue;
        int rank = 0;
        for (int k = 0; k < g; ++k) rank += keep[k];
        const float* src = p.box_tmp + ((size_t)b * PP_MAX_GT_PER_FRAME + g) * 7;
        float* dst = p.gt_out + (size_t)(o0 + rank) * 7;
        for (int k = 0; k < 7; ++k) dst[k] = src[k];
        p.cls_out[o0 + rank] = p.cls_in ? p.cls_in[g0 + g] : 1;
    }
}

}  // namespace

void launch_augment(const AugParams& p, int max_n, hipStream_t s) {
    if (p.batch <= 0) return;
    PP_LAUNCH("k_aug_select", k_aug_select, dim3((unsigned)p.batch), dim3(kSelThreads), 0, s, p);
    if (max_n > 0)
        PP_LAUNCH("k_aug_points", k_aug_points, dim3((unsigned)((max_n + 255) / 256), (unsigned)p.batch), dim3(256), 0, s, p);
    PP_LAUNCH("k_aug_compact", k_aug_compact, dim3((unsigned)p.batch), dim3(256), 0, s, p);
}
