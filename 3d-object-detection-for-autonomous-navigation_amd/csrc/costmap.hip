// Obstacle costmap per frame (pp_set_costmap / pp_costmap_async; costmap.py states the rule and names every operation).
// Three launches behind a clear of the count words, whatever the batch (grid y = frame):
//   k_costmap_objects   the frame's detections or track slots -> its footprint table, compacted in source order
//   k_costmap_points    a lane per resident row: integer atomics into one word per cell
//   k_costmap_compose   a lane per four cells of a row: point layer, footprints (through LDS, box test first), one store
// All cell arithmetic is float64 with + - * / and comparisons (-ffp-contract=off keeps the products and sums apart); the
// only transcendental calls are the cos and sin of a footprint's yaw.
// OBJECT MASK (CostmapParams::mask, NULL while no mask is in force): an in-grid row whose bit is set in the wave's word
// marks its cell observed and adds no count, as a row outside the z band does.
// GROUND CLASSES (CostmapParams::obs, NULL while the ground stage does not name this reader): an in-grid row adds to the
// count iff its OBSTACLE bit is set, in the place of the z band.
#include "pp_common.h"

namespace {

constexpr int CM_BLOCK = 256;
constexpr int CM_TILE = 64;                 // footprints of an LDS tile
constexpr int CM_FP_WORDS = (int)(sizeof(CmFootprint) / 4);
static_assert(sizeof(CmFootprint) == 72, "CmFootprint: 6 doubles, 6 int32 (copied into LDS as 32-bit words)");

__device__ __forceinline__ bool cm_finite(double v) { return (v - v) == 0.0; }

// the cell range [i0, i1] that holds every cell whose centre lies within `ext` of `o` on one axis, clamped to 0 .. n - 1
__device__ __forceinline__ void cm_box_axis(double o, double ext, double lo0, double res, int n, int* i0, int* i1) {
    // a cell half a cell or more outside [o - ext, o + ext] cannot have its centre inside: one cell of slack on either
    // side, and a relative slack far above the rounding of these few operations
    const double slack = (ext + fabs(o) + fabs(lo0)) * 1e-9;
    double a = floor(((o - ext - slack) - lo0) / res) - 1.0;
    double b = floor(((o + ext + slack) - lo0) / res) + 1.0;
    a = fmin(fmax(a, 0.0), (double)n);          // (both finite from here: ext, o are finite, or +-inf clamps)
    b = fmin(fmax(b, -1.0), (double)(n - 1));
    *i0 = (int)a;
    *i1 = (int)b;
}

__global__ __launch_bounds__(CM_BLOCK) void k_costmap_objects(CostmapParams p) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const pp_costmap_config& c = p.cfg;
    __shared__ int s_wave[CM_BLOCK / 64];
    int nitems = 0, flag = 0;
    if (c.objects == 1) {
        const int raw = p.n_dets[b];
        flag = (raw & PP_NDETS_NONFINITE) ? 1 : 0;
        nitems = flag ? 0 : min(max(raw, 0), p.det_rows);
    } else if (c.objects == 2) {
        nitems = PP_TRACK_MAX * (1 + c.horizon_steps);
    }
    nitems = min(nitems, p.table_rows);
    CmFootprint* table = p.table + (size_t)b * p.table_rows;
    int base = 0;
    for (int i0 = 0; i0 < nitems; i0 += CM_BLOCK) {
        const int i = i0 + tid;
        bool valid = false;
        CmFootprint f;
        if (i < nitems) {
            double ox, oy, w, l, yaw;
            int cost = c.object_cost;
            if (c.objects == 1) {
                const pp_detection* d = p.dets + (size_t)b * p.det_rows + i;
                ox = (double)d->box3d_lidar[0]; oy = (double)d->box3d_lidar[1];
                w = (double)d->box3d_lidar[3]; l = (double)d->box3d_lidar[4]; yaw = (double)d->box3d_lidar[6];
                valid = (double)d->score >= c.min_score;
            } else {
                // source order is slot-major: item i is step i % (1 + steps) of slot i / (1 + steps)
                const int per = 1 + c.horizon_steps;
                const int slot = i / per, k = i - slot * per;
                const TrkSlot* t = p.slots + (size_t)b * PP_TRACK_MAX + slot;
                valid = t->live != 0 && (!c.confirmed_only || t->confirmed != 0);
                ox = t->x[0]; oy = t->x[1]; w = t->size[0]; l = t->size[1]; yaw = t->yaw;
                if (k > 0) {
                    const double tk = (double)k * c.horizon_dt;
                    ox = ox + t->x[3] * tk;
                    oy = oy + t->x[4] * tk;
                    cost = c.predict_cost[k - 1];
                }
            }
            f.ox = ox; f.oy = oy; f.c = cos(yaw); f.s = sin(yaw);
            f.hx = w * 0.5 + c.pad; f.hy = l * 0.5 + c.pad;
            f.cost = cost; f.pad = 0;
            valid = valid && cm_finite(f.ox) && cm_finite(f.oy) && cm_finite(f.c) && cm_finite(f.s) && cm_finite(f.hx) && cm_finite(f.hy);
            if (valid) {
                if (f.hx >= 0.0 && f.hy >= 0.0) {
                    const double ex = fabs(f.c) * f.hx + fabs(f.s) * f.hy, ey = fabs(f.s) * f.hx + fabs(f.c) * f.hy;
                    cm_box_axis(f.ox, ex, c.x_min, c.resolution, c.width, &f.ix0, &f.ix1);
                    cm_box_axis(f.oy, ey, c.y_min, c.resolution, c.height, &f.iy0, &f.iy1);
                } else {                            // |u| <= hx never holds
                    f.ix0 = 1; f.ix1 = 0; f.iy0 = 1; f.iy1 = 0;
                }
            }
        }
        const unsigned long long m = __ballot(valid);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int q = 0; q < CM_BLOCK / 64; ++q) {
            if (q < wave) off += s_wave[q];
            tot += s_wave[q];
        }
        if (valid) table[off + __popcll(m & ((1ull << lane) - 1ull))] = f;
        base += tot;
        __syncthreads();
    }
    if (tid == 0) {
        p.n_fp[b] = base;
        p.flagged[b] = flag;
    }
}

__global__ __launch_bounds__(CM_BLOCK) void k_costmap_points(CostmapParams p) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const pp_costmap_config& c = p.cfg;
    const int o0 = p.offsets[b], n = p.offsets[b + 1] - o0;
    if ((int)blockIdx.x * CM_BLOCK >= n) return;           // (the whole workgroup)
    const int i = blockIdx.x * CM_BLOCK + tid;
    int key = -1;
    bool zin = false, masked = false;
    if (i < n) {
        if (p.mask) masked = ((p.mask[(size_t)b * p.mask_stride + (i >> 6)] >> lane) & 1ull) != 0ull;   // one word per wave: rows 64 k .. 64 k + 63 of the frame
        const float* r = p.points + (size_t)(o0 + i) * p.F;
        const double x = (double)r[0], y = (double)r[1], z = (double)r[2];
        const double fx = (x - c.x_min) / c.resolution, fy = (y - c.y_min) / c.resolution;
        // fx >= 0 and floor(fx) < width, the latter as fx < width (the same set, and no integer conversion of a huge value)
        if (fx >= 0.0 && fx < (double)c.width && fy >= 0.0 && fy < (double)c.height) {
            key = (int)fy * p.pitch + (int)fx;
            // a masked row marks its cell observed and adds no count; the ground stage's OBSTACLE bit stands in the place
            // of the z band while it names this reader
            const bool band = p.obs ? ((p.obs[(size_t)b * p.cls_stride + (i >> 6)] >> lane) & 1ull) != 0ull : (c.z_min <= z && z <= c.z_max);
            zin = band && !masked;
        }
    }
    // lanes of a run of equal cells (depth-camera rows land in neighbouring cells in runs) add once, through the run's
    // first lane; every lane of the wave takes part in the ballots
    const int prev = __shfl_up(key, 1);
    const bool head = lane == 0 || key != prev;
    const unsigned long long heads = __ballot(head), zmask = __ballot(zin), ing = __ballot(key >= 0);
    if (head && key >= 0) {
        const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1));
        const int len = above ? __ffsll((long long)above) : 64 - lane;
        const unsigned long long run = (len >= 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
        const int cnt = __popcll(zmask & run);
        unsigned* w = p.words + (size_t)b * c.height * p.pitch + key;
        if (cnt) atomicAdd(w, (unsigned)cnt);
        else atomicOr(w, 0x80000000u);
    }
    if (lane == 0 && ing) atomicAdd(p.in_grid + b, __popcll(ing));
}

__global__ __launch_bounds__(CM_BLOCK) void k_costmap_compose(CostmapParams p) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const pp_costmap_config& c = p.cfg;
    const int qpr = p.pitch >> 2;                          // quads of a row
    const int q = blockIdx.x * CM_BLOCK + tid;
    const bool act = q < qpr * c.height;
    const int iy = act ? q / qpr : 0, ix0 = act ? (q - iy * qpr) * 4 : 0;
    const size_t at = (size_t)b * c.height * p.pitch + (size_t)iy * p.pitch + ix0;
    __shared__ CmFootprint s_fp[CM_TILE];
    static_assert(CM_TILE == 64, "k_costmap_compose: a lane per record of a tile");
    // the cells of this wave: rows wiy0 .. wiy1, and columns wix0 .. wix1 of it when it lies in one row (else all)
    const int lane = tid & 63, total = qpr * c.height, wq0 = q - lane;
    int wiy0 = 0, wiy1 = -1, wix0 = 0, wix1 = -1;          // (a wave past the grid: no record reaches it)
    if (wq0 < total) {
        const int wq1 = min(wq0 + 63, total - 1);
        wiy0 = wq0 / qpr;
        wiy1 = wq1 / qpr;
        wix0 = wiy0 == wiy1 ? (wq0 - wiy0 * qpr) * 4 : 0;
        wix1 = wiy0 == wiy1 ? (wq1 - wiy1 * qpr) * 4 + 3 : p.pitch - 1;
    }

    int best[4] = {-1, -1, -1, -1};
    int cnt[4] = {0, 0, 0, 0};
    double cx[4];
    const double cy = c.y_min + ((double)iy + 0.5) * c.resolution;
    if (act) {
        const uint4 w = *reinterpret_cast<const uint4*>(p.words + at);
        const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cnt[k] = (int)(ww[k] & 0x7fffffffu);
            best[k] = ww[k] != 0u ? 0 : -1;                // observed: a count, or bit 31
            if (cnt[k] >= c.min_points) best[k] = max(best[k], c.point_cost);
            cx[k] = c.x_min + ((double)(ix0 + k) + 0.5) * c.resolution;
        }
    }
    const int nfp = min(p.n_fp[b], p.table_rows);
    const CmFootprint* table = p.table + (size_t)b * p.table_rows;
    for (int t0 = 0; t0 < nfp; t0 += CM_TILE) {
        const int m = min(CM_TILE, nfp - t0);
        __syncthreads();
        const unsigned* src = reinterpret_cast<const unsigned*>(table + t0);
        unsigned* dst = reinterpret_cast<unsigned*>(s_fp);
        for (int k = tid; k < m * CM_FP_WORDS; k += CM_BLOCK) dst[k] = src[k];
        __syncthreads();
        // lane l holds the tile's record l against the cells of the whole wave: the wave then walks only the records
        // whose box reaches it (a tile is as wide as a wave), not all of them one LDS round trip after the other
        bool reach = false;
        if (lane < m) {
            const CmFootprint& g = s_fp[lane];
            reach = !(g.iy1 < wiy0 || g.iy0 > wiy1 || g.ix1 < wix0 || g.ix0 > wix1);
        }
        unsigned long long todo = __ballot(reach);
        while (todo) {
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const CmFootprint& f = s_fp[j];
            if (!act || iy < f.iy0 || iy > f.iy1 || ix0 > f.ix1 || ix0 + 3 < f.ix0) continue;
            const double dy = cy - f.oy;
            const double dys = dy * f.s, dyc = dy * f.c;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double dx = cx[k] - f.ox;
                const double u = (dx * f.c) - dys, v = (dx * f.s) + dyc;
                if (fabs(u) <= f.hx && fabs(v) <= f.hy) best[k] = max(best[k], f.cost);
            }
        }
    }
    if (act) {
        // cells of the row's padding (ix >= width) hold no word and lie in no box: -1, and never copied out
        const unsigned packed = ((unsigned)best[0] & 0xffu) | (((unsigned)best[1] & 0xffu) << 8) |
                                (((unsigned)best[2] & 0xffu) << 16) | (((unsigned)best[3] & 0xffu) << 24);
        *reinterpret_cast<unsigned*>(p.grid + at) = packed;
        *reinterpret_cast<int4*>(p.tap + at) = make_int4(cnt[0], cnt[1], cnt[2], cnt[3]);
    }
}

}  // namespace

void launch_costmap(const CostmapParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    const int quads = (p.pitch >> 2) * p.cfg.height;
    PP_LAUNCH("k_costmap_objects", k_costmap_objects, dim3(1, p.batch), dim3(CM_BLOCK), 0, s, p);
    if (p.max_n > 0)
        PP_LAUNCH("k_costmap_points", k_costmap_points, dim3((p.max_n + CM_BLOCK - 1) / CM_BLOCK, p.batch), dim3(CM_BLOCK), 0, s, p);
    PP_LAUNCH("k_costmap_compose", k_costmap_compose, dim3((quads + CM_BLOCK - 1) / CM_BLOCK, p.batch), dim3(CM_BLOCK), 0, s, p);
}
