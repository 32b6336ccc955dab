// Correlative scan-to-map matching per stream (pp_set_scan_match / pp_scan_match_async, pp_scan_match_grids; scan_match.py
// states the rule and the order of every operation).  Three launches behind one clear of the marks, whatever the batch
// (the last grid dimension = frame = stream):
//   k_scan_cells    a lane per resident row: the float64 rotation, the tests, one mark BIT per cell; the lane that marks a
//                   cell first appends its (ux, uy) to the stream's list; the tallies through ballots
//   k_scan_scores   one workgroup per (tile of SCAN_TILE translation candidates, heading, stream).  The workgroup rotates
//                   the list chunk by chunk into LDS -- once per heading, not once per candidate; the trig entry is
//                   uniform in the workgroup.  Lane l of every wave owns candidate tile * 64 + l (ix fastest: with xy_step
//                   = 1024 neighbouring lanes read neighbouring int16 of a row), and the sixteen waves share a chunk's
//                   cells between them, every sixteenth each: the list is the long axis (thousands of cells against 64
//                   candidates), and a gather costs a trip to L2, so splitting the list over the waves and keeping eight
//                   lookups in flight per wave is what shortens a workgroup's chain (four waves of four lookups: 46.7 us
//                   at the benchmark shape, this: 39.8 us).  The waves' sums meet in LDS; wave 0 stores
//                   the scores and shuffles the tile's least key into `partial`.
//   k_scan_finish   one wave per stream: the least of the partial keys, the status bits, the eight words.
// Marks are OR-only, the sums are integer and the keys are unique (the candidate index is their low 16 bits), so neither
// the order of the rows nor of the list changes a byte.  The only floating-point work is the row rotation of k_scan_cells
// (float64, + * / and floor; -ffp-contract=off keeps products and sums apart); there is no floating-point atomic.
// WIDTHS.  ux, uy, sx, the shifts and the rotated cell stay inside int32 (scan_match.py asserts the bound from width *
// height <= 2^20); the rotation's products C * ux reach 2^14 * 2^30 and are formed in int64; |score| <= 2^20 cells * 1000
// < 2^30 fits int32.  The log-odds are read with no `known` test: the occupancy state holds 0 wherever a cell is not known.
// OBJECT MASK (ScanParams::mask, NULL while no mask is in force): a row whose bit is set in the wave's word takes no part
// and is counted with the ignored rows.
// GROUND CLASSES (ScanParams::obs, NULL while the ground stage does not name this reader): a row takes part iff its OBSTACLE
// bit is set, in the place of the z band.
// BOUNDS.  A lookup outside the window reads cell 0 of the stream and adds 0, so every load lies in the stream's map; the
// list is written below list_cap only and read below min(count, list_cap); a mark word lies below mark_words because the
// cell passed the window test.
#include "pp_common.h"

namespace {

constexpr int SCAN_ROWS = 256;              // rows of a workgroup of k_scan_cells
constexpr int SCAN_BLOCK = 1024;            // lanes of a workgroup of k_scan_scores: 16 waves share a chunk's cells
constexpr int SCAN_WAVES = SCAN_BLOCK / 64;
constexpr int SCAN_CHUNK = 1024;            // scan cells rotated into LDS at a time: 8 KiB
constexpr unsigned long long SCAN_NO_KEY = ~0ull;
static_assert(sizeof(ScanCall) == 64, "ScanCall: 6 doubles, 4 int32 (api_scan_match.hip fills a pinned ring of them)");
static_assert(SCAN_TILE == 64 && SCAN_CHUNK % SCAN_BLOCK == 0, "a candidate per lane of a wave; whole rounds of rotation");
static_assert(PP_LOCAL_SUB == 1024 && PP_LOCAL_HEADINGS == 4096, "cells and ticks by shift and mask");
static_assert(PP_SCAN_MAX_CANDIDATES == 65536, "a key's low 16 bits are the candidate index");

__device__ __forceinline__ unsigned long long scan_wave_min(unsigned long long key) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(key, m);
        key = o < key ? o : key;
    }
    return key;
}

__global__ __launch_bounds__(SCAN_ROWS) void k_scan_cells(ScanParams p) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const pp_occupancy_config& c = p.occ;
    const int o0 = p.offsets[b], n = p.offsets[b + 1] - o0;
    if ((int)blockIdx.x * SCAN_ROWS >= n) return;         // (the whole workgroup)
    const int i = blockIdx.x * SCAN_ROWS + tid;
    const bool row = i < n;
    int cell = -1;                                         // gy * width + gx of a used row
    bool masked = false;
    if (row) {
        if (p.mask) masked = ((p.mask[(size_t)b * p.mask_stride + (i >> 6)] >> lane) & 1ull) != 0ull;   // one word per wave: rows 64 k .. 64 k + 63 of the frame
        const ScanCall& q = p.call[b];
        const float* r = p.points + (size_t)(o0 + i) * p.F;
        const double x = (double)r[0], y = (double)r[1], z = (double)r[2];
        const double dx = (q.r0[0] * x + q.r0[1] * y) + q.r0[2] * z;
        const double dy = (q.r1[0] * x + q.r1[1] * y) + q.r1[2] * z;
        // the index stays a double until it is known to lie in the window (a huge or non-finite value fails here)
        const double gx = floor(dx / c.resolution) + (double)(c.width / 2), gy = floor(dy / c.resolution) + (double)(c.height / 2);
        // the ground stage's OBSTACLE bit in the place of the z band, while it names this reader
        const bool band = p.obs ? ((p.obs[(size_t)b * p.cls_stride + (i >> 6)] >> lane) & 1ull) != 0ull : (z <= c.z_max && z >= c.z_min);
        const bool used = gx >= 0.0 && gx < (double)c.width && gy >= 0.0 && gy < (double)c.height &&
                          (x * x + y * y) <= c.max_range * c.max_range && band;
        if (used && !masked) cell = (int)gy * c.width + (int)gx;          // a masked row takes no part: ignored
    }
    // lanes of a run of equal cells mark once, through the run's first lane; every lane of the wave takes part in the
    // shuffle and the ballots
    const int prev = __shfl_up(cell, 1);
    const bool head = lane == 0 || cell != prev;
    const unsigned long long use = __ballot(cell >= 0), ign = __ballot(row && cell < 0);
    int* info = p.info + (size_t)b * SCAN_INFO;
    if (head && cell >= 0) {
        unsigned* w = p.marks + (size_t)b * p.mark_words + (cell >> 5);
        const unsigned bit = 1u << (cell & 31);
        if (!(*w & bit)) {
            const unsigned old = atomicOr(w, bit);
            if (!(old & bit)) {                            // the first row of this cell: its one list entry
                const int k = atomicAdd(info + 2, 1);
                if (k < p.list_cap) {
                    const int gy = cell / c.width, gx = cell - gy * c.width;
                    p.list[(size_t)b * p.list_cap + k] = make_int2((gx - c.width / 2) * PP_LOCAL_SUB + PP_LOCAL_SUB / 2,
                                                                   (gy - c.height / 2) * PP_LOCAL_SUB + PP_LOCAL_SUB / 2);
                }
            }
        }
    }
    if (lane == 0) {
        if (use) atomicAdd(info + 0, __popcll(use));
        if (ign) atomicAdd(info + 1, __popcll(ign));
    }
}

// the key of candidate (ix, iy, it) with `score`; d and c as scan_match.py step 4
__device__ __forceinline__ unsigned long long scan_key(const pp_scan_match_config& g, int ix, int iy, int it, int score) {
    const unsigned d = (unsigned)(abs(it - g.nt) + abs(iy - g.ny) + abs(ix - g.nx));
    const unsigned c = (unsigned)((it * (2 * g.ny + 1) + iy) * (2 * g.nx + 1) + ix);
    return ((unsigned long long)(unsigned)((1 << 30) - score) << 32) | (unsigned long long)((d << 16) | c);
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_scores(ScanParams p) {
    __shared__ int2 s_rot[SCAN_CHUNK];
    __shared__ int s_sum[SCAN_WAVES][64];
    const int b = blockIdx.z, it = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const pp_scan_match_config& g = p.cfg;
    const ScanCall& q = p.call[b];
    const int W = p.occ.width, H = p.occ.height, wx = 2 * g.nx + 1;
    // a stream without a map, or whose prior lies outside its window, scores nothing: every sum stays 0 (wave-uniform)
    const int n = q.flags ? 0 : min(p.info[(size_t)b * SCAN_INFO + 2], p.list_cap);
    const unsigned tr = p.trig[((it - g.nt) * g.theta_step) & (PP_LOCAL_HEADINGS - 1)];
    const long long C = (short)(tr & 0xffffu), S = (short)(tr >> 16);
    const int t = (int)blockIdx.x * SCAN_TILE + lane;      // the lane's translation candidate of this heading
    const bool live = t < p.n_trans;
    const int iy = live ? t / wx : 0, ix = live ? t - iy * wx : 0;
    const int bx = q.sx + (ix - g.nx) * g.xy_step, by = q.sy + (iy - g.ny) * g.xy_step;
    const int16_t* L = p.logodds[q.src] + (size_t)b * p.map_stride;
    const int2* list = p.list + (size_t)b * p.list_cap;
    int sum = 0;
    for (int k0 = 0; k0 < n; k0 += SCAN_CHUNK) {
        const int m = min(SCAN_CHUNK, n - k0);
        for (int k = tid; k < m; k += SCAN_BLOCK) {
            const int2 u = list[k0 + k];
            s_rot[k] = make_int2((int)((C * u.x - S * u.y + 8192) >> 14), (int)((S * u.x + C * u.y + 8192) >> 14));
        }
        __syncthreads();
        // wave w takes cells w, w + 16, ...: the address is the same in every lane of a wave (an LDS broadcast); eight
        // lookups are in flight per wave, which is what hides the gathers' way to L2 and back
#pragma unroll 8
        for (int k = wave; k < m; k += SCAN_WAVES) {
            const int2 r = s_rot[k];
            const int cx = (bx + r.x) >> 10, cy = (by + r.y) >> 10;
            const bool in = (unsigned)cx < (unsigned)W && (unsigned)cy < (unsigned)H;
            const int v = L[in ? cy * p.pitch + cx : 0];
            sum += in ? v : 0;
        }
        __syncthreads();                                   // the chunk is read before the next one is written
    }
    s_sum[wave][lane] = sum;
    __syncthreads();
    if (wave != 0) return;
    int score = 0;
#pragma unroll
    for (int w = 0; w < SCAN_WAVES; ++w) score += s_sum[w][lane];
    unsigned long long key = SCAN_NO_KEY;
    if (live) {
        const int ncand = p.n_trans * (2 * g.nt + 1);
        p.scores[(size_t)b * ncand + (size_t)it * p.n_trans + t] = score;
        key = scan_key(g, ix, iy, it, score);
    }
    key = scan_wave_min(key);
    if (lane == 0) p.partial[((size_t)b * gridDim.y + it) * p.tiles + blockIdx.x] = key;
}

__global__ __launch_bounds__(64) void k_scan_finish(ScanParams p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const pp_scan_match_config& g = p.cfg;
    const int wt = 2 * g.nt + 1, wy = 2 * g.ny + 1, wx = 2 * g.nx + 1;
    const int parts = wt * p.tiles;
    const unsigned long long* part = p.partial + (size_t)b * parts;
    unsigned long long key = SCAN_NO_KEY;
    for (int k = lane; k < parts; k += 64) {
        const unsigned long long o = part[k];
        key = o < key ? o : key;
    }
    key = scan_wave_min(key);
    if (lane != 0) return;
    const int c = (int)(key & 0xffffu), best = (1 << 30) - (int)(unsigned)(key >> 32);
    const int ix = c % wx, iy = (c / wx) % wy, it = c / (wx * wy);
    const int* info = p.info + (size_t)b * SCAN_INFO;
    const int n_scan = info[2];
    const int centre = (g.nt * wy + g.ny) * wx + g.nx;
    int status = p.call[b].flags;
    if (n_scan < g.min_cells) status |= PP_SCAN_FEW_CELLS;
    if ((long long)best * 100 < (long long)g.min_mean * n_scan) status |= PP_SCAN_LOW_SCORE;
    if ((g.nx > 0 && abs(ix - g.nx) == g.nx) || (g.ny > 0 && abs(iy - g.ny) == g.ny) || (g.nt > 0 && abs(it - g.nt) == g.nt))
        status |= PP_SCAN_EDGE;
    int* w = p.words + (size_t)b * PP_SCAN_RESULT;
    w[0] = status; w[1] = ix - g.nx; w[2] = iy - g.ny; w[3] = it - g.nt;
    w[4] = best; w[5] = p.scores[(size_t)b * wt * p.n_trans + centre]; w[6] = n_scan; w[7] = info[1];
}

}  // namespace

void launch_scan_match(const ScanParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    if (p.max_n > 0)
        PP_LAUNCH("k_scan_cells", k_scan_cells, dim3((p.max_n + SCAN_ROWS - 1) / SCAN_ROWS, p.batch), dim3(SCAN_ROWS), 0, s, p);
    PP_LAUNCH("k_scan_scores", k_scan_scores, dim3(p.tiles, 2 * p.cfg.nt + 1, p.batch), dim3(SCAN_BLOCK), 0, s, p);
    PP_LAUNCH("k_scan_finish", k_scan_finish, dim3(p.batch), dim3(64), 0, s, p);
}
