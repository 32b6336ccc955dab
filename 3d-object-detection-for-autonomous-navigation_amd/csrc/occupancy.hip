// Rolling occupancy map per stream (pp_set_occupancy / pp_occupancy_update_async; occupancy.py states the rule and the
// order of every operation).  Three launches behind a clear of the marks, whatever the batch (grid y = frame = stream):
//   k_occ_endpoints   a lane per resident row: the float64 transform, the tests, one mark word per end cell; the lane
//                     that marks a cell first appends it to the stream's list
//   k_occ_rays        a lane per listed cell: the integer walk from the sensor's cell outwards, a 1 into the `passed`
//                     byte of every cell it crosses
//   k_occ_apply       a lane per four cells of a row: the old window's cell (shifted), the step, the clamps, the cost
//                     through the table; writes the other state copy and its int8 row
// Marks are OR-only and idempotent, so neither the order of the rows nor of the list changes a byte: the end cells' HIT /
// GROUND bits are integer atomics behind a plain test (the returned word tells the first lane of a cell, which lists
// it), the walks' marks plain stores of one and the same byte -- a walk then waits for no memory round trip (the same
// walks through test-then-atomicOr on the words took 5 - 10 times as long).  The only floating-point work is the endpoint transform (float64, + * / and floor;
// -ffp-contract=off keeps products and sums apart); there is no floating-point atomic and no transcendental call.
// OBJECT MASK (OccParams::mask, NULL while no mask is in force): a row of the hit band whose bit is set in the wave's word
// is a MASKED end -- a third mark bit, so its cell is listed and gets its ray like any end cell, while k_occ_apply, which
// reads HIT and GROUND alone, neither hits nor frees it.  A wave covers rows 64 k .. 64 k + 63 of a frame: one word.
// GROUND CLASSES (OccParams::gnd / obs, NULL while the ground stage does not name this reader): the z <= z_max test and the
// z >= z_min split are dropped; an in-window, in-range row is a hit iff its OBSTACLE bit is set, a ground return iff its
// GROUND bit is set, and ignored otherwise.  Two more words per wave.
#include "pp_common.h"

namespace {

constexpr int OCC_BLOCK = 256;
static_assert(PP_OCC_HIT == 1u && PP_OCC_GROUND == 2u && PP_OCC_MASKED == 4u, "k_occ_endpoints: the mark bit of kind k is 1 << k");
static_assert(sizeof(OccCall) == 96, "OccCall: 8 doubles, 8 int32 (api_occupancy.hip fills a pinned ring of them)");

__global__ __launch_bounds__(OCC_BLOCK) void k_occ_endpoints(OccParams p) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const pp_occupancy_config& c = p.cfg;
    const int o0 = p.offsets[b], n = p.offsets[b + 1] - o0;
    if ((int)blockIdx.x * OCC_BLOCK >= n) return;          // (the whole workgroup)
    const int i = blockIdx.x * OCC_BLOCK + tid;
    const bool row = i < n;
    int code = -1;                                         // cell * 4 + kind of a used row: 0 hit, 1 ground, 2 masked end
    bool masked = false;
    if (row) {
        if (p.mask) masked = ((p.mask[(size_t)b * p.mask_stride + (i >> 6)] >> lane) & 1ull) != 0ull;   // one word per wave: rows 64 k .. 64 k + 63 of the frame
        const OccCall& q = p.call[b];
        const float* r = p.points + (size_t)(o0 + i) * p.F;
        const double x = (double)r[0], y = (double)r[1], z = (double)r[2];
        const double px = ((q.r0[0] * x + q.r0[1] * y) + q.r0[2] * z) + q.tx;
        const double py = ((q.r1[0] * x + q.r1[1] * y) + q.r1[2] * z) + q.ty;
        // the window index stays a double until it is known to lie in the window (a huge or non-finite value fails here)
        const double gx = floor(px / c.resolution) - (double)q.ox, gy = floor(py / c.resolution) - (double)q.oy;
        const bool inwin = gx >= 0.0 && gx < (double)c.width && gy >= 0.0 && gy < (double)c.height &&
                           (x * x + y * y) <= c.max_range * c.max_range;
        bool used, hitband;
        if (p.obs) {                                       // the ground stage's classes in the place of the z band
            const size_t w = (size_t)b * p.cls_stride + (i >> 6);
            hitband = ((p.obs[w] >> lane) & 1ull) != 0ull;
            used = inwin && (hitband || ((p.gnd[w] >> lane) & 1ull) != 0ull);
        } else {
            used = inwin && z <= c.z_max;
            hitband = z >= c.z_min;
        }
        if (used) code = ((int)gy * p.pitch + (int)gx) * 4 + (hitband ? (masked ? 2 : 0) : 1);
    }
    // lanes of a run of equal codes (depth-camera rows end in neighbouring cells in runs) mark once, through the run's
    // first lane; every lane of the wave takes part in the shuffle and the ballots
    const int prev = __shfl_up(code, 1);
    const bool head = lane == 0 || code != prev;
    const unsigned long long hit = __ballot(code >= 0 && (code & 3) == 0), gnd = __ballot(code >= 0 && (code & 3) == 1),
                             msk = __ballot(code >= 0 && (code & 3) == 2), ign = __ballot(row && code < 0);
    if (head && code >= 0) {
        const int cell = code >> 2;
        const unsigned bits = 1u << (code & 3);            // PP_OCC_HIT, PP_OCC_GROUND, PP_OCC_MASKED
        unsigned* w = p.marks + (size_t)b * c.height * p.pitch + cell;
        if ((*w & bits) != bits) {
            const unsigned old = atomicOr(w, bits);
            if (!(old & (PP_OCC_HIT | PP_OCC_GROUND | PP_OCC_MASKED))) {   // the first endpoint of this cell: its one ray
                const int k = atomicAdd(p.info + (size_t)b * PP_OCC_INFO + 5, 1);
                if (k < p.list_cap) p.list[(size_t)b * p.list_cap + k] = cell;
            }
        }
    }
    if (lane == 0) {
        int* info = p.info + (size_t)b * PP_OCC_INFO;
        if (hit) atomicAdd(info + 0, __popcll(hit));
        if (gnd) atomicAdd(info + 1, __popcll(gnd));
        if (ign) atomicAdd(info + 2, __popcll(ign));
        if (msk) atomicAdd(info + 6, __popcll(msk));
    }
}

__global__ __launch_bounds__(OCC_BLOCK) void k_occ_rays(OccParams p) {
    const int b = blockIdx.y;
    const pp_occupancy_config& c = p.cfg;
    const int listed = min(p.info[(size_t)b * PP_OCC_INFO + 5], p.list_cap);
    const int i = blockIdx.x * OCC_BLOCK + threadIdx.x;
    if (i >= listed) return;
    const int cell = p.list[(size_t)b * p.list_cap + i];
    const int y1 = cell / p.pitch, x1 = cell - y1 * p.pitch;
    int x = c.width / 2, y = c.height / 2;
    const int dx = abs(x1 - x), dy = abs(y1 - y);
    const int sx = x1 > x ? 1 : -1, sy = y1 > y ? 1 : -1;
    int err = dx - dy;
    unsigned char* passed = p.passed + (size_t)b * c.height * p.pitch;
    // the walk stays inside the box of its two ends and takes at most dx + dy steps; both are held here as well, so that
    // no input can carry a store out of the window
    for (int step = 0; step < dx + dy && (x != x1 || y != y1); ++step) {
        if ((unsigned)x < (unsigned)c.width && (unsigned)y < (unsigned)c.height) {
            passed[(size_t)y * p.pitch + x] = 1;
        }
        const int e2 = 2 * err;
        if (e2 > -dy) { err -= dy; x += sx; }
        if (e2 < dx) { err += dx; y += sy; }
    }
}

__global__ __launch_bounds__(OCC_BLOCK) void k_occ_apply(OccParams p) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const pp_occupancy_config& c = p.cfg;
    const int qpr = p.pitch >> 2;                          // quads of a row
    const int q = blockIdx.x * OCC_BLOCK + tid;
    const bool act = q < qpr * c.height;
    int n_hit = 0, n_free = 0;
    if (act) {
        const int iy = q / qpr, ix0 = (q - iy * qpr) * 4;
        const OccCall& k = p.call[b];
        const size_t cells = (size_t)c.height * p.pitch;
        const size_t at = (size_t)b * cells + (size_t)iy * p.pitch + ix0;
        const int16_t* l_old = p.logodds[k.src] + (size_t)b * cells;
        const int8_t* g_old = p.grid[k.src] + (size_t)b * cells;
        const uint4 m4 = *reinterpret_cast<const uint4*>(p.marks + at);
        const unsigned m[4] = {m4.x, m4.y, m4.z, m4.w};
        const uchar4 p4 = *reinterpret_cast<const uchar4*>(p.passed + at);
        const unsigned char walked[4] = {p4.x, p4.y, p4.z, p4.w};
        const int oy = iy + k.sdy;
        const bool row_kept = !k.fresh && (unsigned)oy < (unsigned)c.height;
        unsigned lo[4], cost[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ix = ix0 + j, ox = ix + k.sdx;
            int L = 0;
            bool known = false;
            if (row_kept && ix < c.width && (unsigned)ox < (unsigned)c.width) {
                const size_t o = (size_t)oy * p.pitch + ox;
                known = g_old[o] != -1;
                L = l_old[o];
            }
            const bool hit = m[j] & PP_OCC_HIT, passed = walked[j] || (m[j] & PP_OCC_GROUND);   // a ground end frees its own cell
            L = min(max(L + (hit ? c.l_hit : passed ? -c.l_miss : 0), c.l_min), c.l_max);
            known = known || hit || passed;
            n_hit += hit ? 1 : 0;
            n_free += passed && !hit ? 1 : 0;
            lo[j] = (unsigned)L & 0xffffu;
            cost[j] = (unsigned)(known ? (int)p.table[L - c.l_min] : -1) & 0xffu;
        }
        // cells of the row's padding (ix >= width) are never marked and never read back: L 0, -1
        *reinterpret_cast<uint2*>(p.logodds[1 - k.src] + at) = make_uint2(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16));
        *reinterpret_cast<unsigned*>(p.grid[1 - k.src] + at) = cost[0] | (cost[1] << 8) | (cost[2] << 16) | (cost[3] << 24);
    }
    // (every lane of the wave is here)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_hit += __shfl_down(n_hit, o);
        n_free += __shfl_down(n_free, o);
    }
    if (lane == 0) {
        int* info = p.info + (size_t)b * PP_OCC_INFO;
        if (n_hit) atomicAdd(info + 3, n_hit);
        if (n_free) atomicAdd(info + 4, n_free);
    }
}

}  // namespace

void launch_occupancy(const OccParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    const int quads = (p.pitch >> 2) * p.cfg.height;
    const int rays = p.max_n < p.list_cap ? p.max_n : p.list_cap;   // a frame lists at most a cell per row
    if (p.max_n > 0) {
        PP_LAUNCH("k_occ_endpoints", k_occ_endpoints, dim3((p.max_n + OCC_BLOCK - 1) / OCC_BLOCK, p.batch), dim3(OCC_BLOCK), 0, s, p);
        PP_LAUNCH("k_occ_rays", k_occ_rays, dim3((rays + OCC_BLOCK - 1) / OCC_BLOCK, p.batch), dim3(OCC_BLOCK), 0, s, p);
    }
    PP_LAUNCH("k_occ_apply", k_occ_apply, dim3((quads + OCC_BLOCK - 1) / OCC_BLOCK, p.batch), dim3(OCC_BLOCK), 0, s, p);
}
