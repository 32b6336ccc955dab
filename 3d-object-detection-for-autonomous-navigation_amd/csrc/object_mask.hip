// Per-point object mask (pp_set_object_mask / pp_object_mask_async, pp_object_mask_points; object_mask.py states the rule
// and names every operation).  Two launches whatever the batch (grid y = frame):
//   k_objmask_table   one workgroup per frame: the frame's detections, its stream's track slots (a COPY of each carried
//                     by the call's pose and predicted by its dt, as k_track_step's stages 0 and 1 would) or the rows the
//                     caller gave -> the frame's footprint table, compacted in source order by ballot as
//                     k_costmap_objects compacts its own; the frame's info words
//   k_objmask_rows    a lane per resident row: the table through LDS, a float32 box pretest, the float64 test; the wave's
//                     ballot is one 64-bit store by one lane, the masked count one integer atomic per wave
// All arithmetic of the test is float64 with + - * and comparisons (-ffp-contract=off keeps the products and sums apart);
// the only transcendental calls are the cos and sin of a footprint's yaw.  No floating-point atomic, no inline assembly:
// two runs give the same bytes.
// BOUNDS.  A table holds OM_ROWS records and a frame's sources are cut at OM_ROWS items before the loop; word w of a frame
// is stored only with w < stride; a row is read only with i < n, the frame's own count.
#include "pp_common.h"

namespace {

constexpr int OM_ROWS = PP_OBJMASK_MAX_FOOTPRINTS;
constexpr int OM_TABLE_BLOCK = 128;         // a lane per source item: one trip
constexpr int OM_BLOCK = 256;
constexpr int OM_FP_WORDS = (int)(sizeof(OmFootprint) / 4);
static_assert(sizeof(OmFootprint) == 64, "OmFootprint: 6 doubles, 4 floats (copied into LDS as 32-bit words)");
static_assert(sizeof(OmCall) == 120, "OmCall: 14 doubles, 2 int32 (api_object_mask.hip fills a pinned ring of them)");
static_assert(OM_ROWS == OM_TABLE_BLOCK && OM_ROWS >= PP_TRACK_MAX && OM_ROWS >= PP_TRACK_MASK_ROWS, "an item per lane of the table's workgroup");
static_assert(PP_OBJMASK_INFO == 4, "footprints, masked rows, rows, flagged");

__device__ __forceinline__ bool om_finite(double v) { return (v - v) == 0.0; }

// [lo, hi] as float32 around o +- ext: no float32 coordinate outside it lies within ext of o.  The slack is far above
// the rounding of these few operations AND of the conversion to float32 (2^-24 relative), which rounds to nearest
__device__ __forceinline__ void om_box_axis(double o, double ext, float* lo, float* hi) {
    const double slack = (ext + fabs(o)) * 1e-6 + 1e-30;
    *lo = (float)((o - ext) - slack);
    *hi = (float)((o + ext) + slack);
}

__global__ __launch_bounds__(OM_TABLE_BLOCK) void k_objmask_table(OmParams p) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const pp_object_mask_config& c = p.cfg;
    __shared__ int s_wave[OM_TABLE_BLOCK / 64];
    int nitems = 0, flag = 0;
    if (p.objects == OM_DETECTIONS) {
        const int raw = p.n_dets[b];
        flag = (raw & PP_NDETS_NONFINITE) ? 1 : 0;
        nitems = flag ? 0 : min(max(raw, 0), p.det_rows);
    } else if (p.objects == OM_TRACKS) {
        nitems = PP_TRACK_MAX;
    } else if (p.objects == OM_GIVEN) {
        nitems = max(p.given_off[b + 1] - p.given_off[b], 0);
    }
    nitems = min(nitems, OM_ROWS);
    OmFootprint* table = p.table + (size_t)b * OM_ROWS;
    bool valid = false;
    OmFootprint f;
    if (tid < nitems) {
        double ox, oy, w, l, yaw;
        if (p.objects == OM_DETECTIONS) {
            const pp_detection* d = p.dets + (size_t)b * p.det_rows + tid;
            ox = (double)d->box3d_lidar[0]; oy = (double)d->box3d_lidar[1];
            w = (double)d->box3d_lidar[3]; l = (double)d->box3d_lidar[4]; yaw = (double)d->box3d_lidar[6];
            valid = (double)d->score >= c.min_score;
        } else if (p.objects == OM_TRACKS) {
            const TrkSlot* t = p.slots + (size_t)b * PP_TRACK_MAX + tid;
            valid = t->live != 0 && (!c.confirmed_only || t->confirmed != 0);
            double x = t->x[0], y = t->x[1], z = t->x[2], vx = t->x[3], vy = t->x[4], vz = t->x[5];
            yaw = t->yaw;
            if (p.call) {
                const OmCall* q = p.call + b;
                const TrkPose* pv = p.pose_prev + b;
                if (q->has_pose && pv->has != 0) {       // the expressions of k_track_step's stage 0
                    const double* R = q->m;
                    const double* S = pv->m;
                    const double dpsi = q->psi - pv->psi;
                    const double d0 = S[3] - R[3], d1 = S[7] - R[7], d2 = S[11] - R[11];
                    double M[9], u[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) M[i * 3 + j] = (R[i] * S[j] + R[4 + i] * S[4 + j]) + R[8 + i] * S[8 + j];
                        u[i] = (R[i] * d0 + R[4 + i] * d1) + R[8 + i] * d2;
                    }
                    const double nx = ((M[0] * x + M[1] * y) + M[2] * z) + u[0];
                    const double ny = ((M[3] * x + M[4] * y) + M[5] * z) + u[1];
                    const double nvx = (M[0] * vx + M[1] * vy) + M[2] * vz;
                    const double nvy = (M[3] * vx + M[4] * vy) + M[5] * vz;
                    x = nx; y = ny; vx = nvx; vy = nvy;
                    yaw = yaw + dpsi;
                }
                if (q->has_dt) {                         // ... and of its stage 1
                    x = x + vx * q->dt;
                    y = y + vy * q->dt;
                }
            }
            valid = valid && (vx * vx + vy * vy) >= c.min_speed * c.min_speed;
            ox = x; oy = y; w = t->size[0]; l = t->size[1];
        } else {
            const double* g = p.given + ((size_t)p.given_off[b] + tid) * 5;
            ox = g[0]; oy = g[1]; w = g[2]; l = g[3]; yaw = g[4];
            valid = true;
        }
        f.ox = ox; f.oy = oy; f.c = cos(yaw); f.s = sin(yaw);
        f.hx = w * 0.5 + c.pad; f.hy = l * 0.5 + c.pad;
        valid = valid && om_finite(f.ox) && om_finite(f.oy) && om_finite(f.c) && om_finite(f.s) && om_finite(f.hx) && om_finite(f.hy);
        f.xlo = 1.0f; f.xhi = 0.0f; f.ylo = 1.0f; f.yhi = 0.0f;     // |u| <= hx never holds with hx < 0
        if (valid && f.hx >= 0.0 && f.hy >= 0.0) {
            const double ex = fabs(f.c) * f.hx + fabs(f.s) * f.hy, ey = fabs(f.s) * f.hx + fabs(f.c) * f.hy;
            om_box_axis(f.ox, ex, &f.xlo, &f.xhi);
            om_box_axis(f.oy, ey, &f.ylo, &f.yhi);
        }
    }
    const unsigned long long m = __ballot(valid);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < OM_TABLE_BLOCK / 64; ++q) {
        if (q < wave) off += s_wave[q];
        tot += s_wave[q];
    }
    if (valid) table[off + __popcll(m & ((1ull << lane) - 1ull))] = f;
    if (tid == 0) {
        int* info = p.info + (size_t)b * PP_OBJMASK_INFO;
        info[0] = tot;
        info[1] = 0;                                     // k_objmask_rows adds to it
        info[2] = max(p.offsets[b + 1] - p.offsets[b], 0);
        info[3] = flag;
    }
}

__global__ __launch_bounds__(OM_BLOCK) void k_objmask_rows(OmParams p) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int o0 = p.offsets[b], n = p.offsets[b + 1] - o0;
    const int i = blockIdx.x * OM_BLOCK + tid;
    const int w = i >> 6;                                  // the wave's word: rows 64 w .. 64 w + 63 of the frame
    unsigned long long* word = p.words + (size_t)b * p.stride + w;
    const int nfp = min(p.info[(size_t)b * PP_OBJMASK_INFO], OM_ROWS);
    if (nfp <= 0 || (int)blockIdx.x * OM_BLOCK >= n) {     // (the whole workgroup) an empty table, or no row: zeros
        if (lane == 0 && w < p.stride) *word = 0ull;
        return;
    }
    __shared__ OmFootprint s_fp[OM_ROWS];
    {
        const unsigned* src = reinterpret_cast<const unsigned*>(p.table + (size_t)b * OM_ROWS);
        unsigned* dst = reinterpret_cast<unsigned*>(s_fp);
        for (int k = tid; k < nfp * OM_FP_WORDS; k += OM_BLOCK) dst[k] = src[k];
    }
    __syncthreads();
    bool in = false;
    if (i < n) {
        const float* r = p.points + (size_t)(o0 + i) * p.F;
        const float xf = r[0], yf = r[1];
        const double x = (double)xf, y = (double)yf;
        for (int j = 0; j < nfp; ++j) {
            const OmFootprint& f = s_fp[j];                // one address in every lane: an LDS broadcast
            // the box only spares the float64 work: whatever passes it is decided by the test of the rule alone (a NaN
            // fails both)
            if (xf >= f.xlo && xf <= f.xhi && yf >= f.ylo && yf <= f.yhi) {
                const double dx = x - f.ox, dy = y - f.oy;
                const double u = (dx * f.c) - (dy * f.s), v = (dx * f.s) + (dy * f.c);
                in = in || (fabs(u) <= f.hx && fabs(v) <= f.hy);
            }
        }
    }
    const unsigned long long m = __ballot(in);
    if (lane == 0) {
        if (w < p.stride) *word = m;
        if (m) atomicAdd(p.info + (size_t)b * PP_OBJMASK_INFO + 1, __popcll(m));
    }
}

}  // namespace

void launch_object_mask(const OmParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    PP_LAUNCH("k_objmask_table", k_objmask_table, dim3(1, p.batch), dim3(OM_TABLE_BLOCK), 0, s, p);
    if (p.max_n > 0)
        PP_LAUNCH("k_objmask_rows", k_objmask_rows, dim3((p.max_n + OM_BLOCK - 1) / OM_BLOCK, p.batch), dim3(OM_BLOCK), 0, s, p);
}
