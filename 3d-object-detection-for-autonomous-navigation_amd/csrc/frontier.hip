// Frontier clusters of an int8 OccupancyGrid (pp_set_frontier / pp_frontier_async / pp_frontier_grids; frontier.py states
// the rule): the free cells that touch unknown space, their connected components, and the components ranked as goals.
// Integer compares, adds, minima and one 64-bit division per frontier cell; no float.  Five launches, grid y = grid index
// whatever the batch:
//   mark     a lane per four cells of a row (one 32-bit load per row where the rows are word-aligned, bytes otherwise):
//            the frontier test, labels = own index or NONE, the accumulators of a frontier cell cleared, the cells counted
//            by one integer atomic per wave
//   label    connected components by a block-based union-find.  A workgroup owns a tile of 32 x 32 cells and returns at
//            once where the tile holds no frontier cell.  PHASE ONE joins the tile's cells in LDS: every cell unions itself
//            with its forward neighbours (E, S and under connectivity 8 SE, SW) inside the tile.  PHASE TWO carries the
//            result into the global label array as unions as well -- every cell with its tile root, and every cell with
//            its forward neighbours in OTHER tiles -- so a tile never has to wait for its neighbour: a union is find, find,
//            atomicMin of the smaller root into the larger root's slot, and when that slot had been lowered meanwhile the
//            union goes on with the value found there.  Parents only ever fall and a set's root is its least index, so the
//            partition and every root are the same whatever the order.  No rounds, no host loop.
//   stats    a lane per cell: finds its root and stores it (the flatten), adds n, sx, sy at the root -- one atomic per
//            wave where the wave's frontier cells share a root, which a run along a row does -- and lists the roots
//   rep      a lane per cell: the centroid cell from the root's sums, a 64-bit atomicMin of the representative key
//   select   one workgroup per grid over the listed roots: counts small / unreached / kept; up to 256 roots take a lane each
//            and a key's place in the order is the number of keys below it; past that max_frontiers passes, each the
//            least sort key above the last (the keys of the first 2048 roots stay in LDS behind pass 0)
// Every loop is bounded by the cell count: a chain of parents strictly falls, so a find takes at most `cells` steps, and
// every retry of a union lowers the sum of its two indices, so it takes at most 2 * cells.  Passing a bound raises the
// grid's FR_OVERRUN word, which the getter turns into PP_ERR_INTERNAL.  Integer atomics and same-value stores only.
#include "pp_common.h"

namespace {

constexpr int FR_BLOCK = 256, FR_TW = 32, FR_TH = 32;
constexpr int FR_TILE = FR_TW * FR_TH, FR_CPT = FR_TILE / FR_BLOCK;       // cells of a tile, and of a lane of it
constexpr int FR_CACHE = 2048;                                            // sort keys select keeps in LDS
constexpr unsigned FR_NONE = PP_FRONTIER_NONE;
constexpr unsigned long long FR_NOKEY = ~0ull;
static_assert(PP_OCC_MAX_CELLS == 1 << 20, "a label takes the low 20 bits of a key");
static_assert(FR_BLOCK % FR_TW == 0 && FR_CPT * FR_BLOCK == FR_TILE, "a lane owns FR_CPT cells of a tile");
static_assert(PP_FRONTIER_MAX <= FR_BLOCK, "select clears a grid's unused words with a lane per frontier");

#define FR_LOAD(p, scope) __hip_atomic_load((p), __ATOMIC_RELAXED, (scope))

// the root of `a`: parents strictly fall, so at most `cells` steps
template <int SCOPE>
__device__ __forceinline__ unsigned fr_find(unsigned* par, unsigned a, int cells, int* overrun) {
    for (int it = 0; it <= cells; ++it) {
        const unsigned q = FR_LOAD(par + a, SCOPE);
        if (q == a) return a;
        a = q;
    }
    *overrun = 1;
    return a;
}

// joins the sets of a and b: the larger root goes under the smaller.  Where the larger root's slot had been lowered by
// another lane meanwhile (`old`), a stays joined to whichever of old and b the slot now holds, and (old, b) remain to be
// joined: every retry lowers a + b.
template <int SCOPE>
__device__ __forceinline__ void fr_union(unsigned* par, unsigned a, unsigned b, int cells, int* overrun) {
    for (int it = 0; it <= 2 * cells; ++it) {
        a = fr_find<SCOPE>(par, a, cells, overrun);
        b = fr_find<SCOPE>(par, b, cells, overrun);
        if (a == b) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;
    }
    *overrun = 1;
}

// the bytes of cells x0 .. x0 + 3 of a row; a cell right of the width reads 0 (known)
__device__ __forceinline__ unsigned fr_row4(const int8_t* row, int x0, int W, bool aligned) {
    unsigned v = 0;
    if (aligned) {
        v = *(const unsigned*)(row + x0);
        const int keep = W - x0;
        if (keep < 4) v &= (1u << (8 * keep)) - 1u;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x0 + k < W) v |= (unsigned)(unsigned char)row[x0 + k] << (8 * k);
    }
    return v;
}

__device__ __forceinline__ int fr_wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(FR_BLOCK) void k_frontier_mark(FrontierParams p) {
    const int b = blockIdx.y, W = p.width, H = p.height;
    const int quads = (W + 3) / 4;
    const int i = (int)blockIdx.x * FR_BLOCK + (int)threadIdx.x;
    const size_t base = (size_t)b * W * H;
    int nf = 0;
    if (i < quads * H) {
        const int y = i / quads, x0 = (i % quads) * 4;
        unsigned front = 0;                              // bit k: cell x0 + k is a frontier cell
        if (p.call[b].flags & FRONTIER_KNOWN) {
            const int8_t* grid = p.grid + (size_t)b * p.stride;
            const bool aligned = ((((size_t)grid) | (size_t)p.pitch) & 3) == 0;
            const int8_t* row = grid + (size_t)y * p.pitch;
            const unsigned c = fr_row4(row, x0, W, aligned);
            const unsigned up = y > 0 ? fr_row4(row - p.pitch, x0, W, aligned) : 0u;
            const unsigned dn = y + 1 < H ? fr_row4(row + p.pitch, x0, W, aligned) : 0u;
            const unsigned lf = (c << 8) | (x0 > 0 ? (unsigned)(unsigned char)row[x0 - 1] : 0u);
            const unsigned rt = (c >> 8) | (x0 + 4 < W ? (unsigned)(unsigned char)row[x0 + 4] << 24 : 0u);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int g = (int)(int8_t)(c >> (8 * k));
                const bool unk = ((up >> (8 * k)) & 255u) == 255u || ((dn >> (8 * k)) & 255u) == 255u ||
                                 ((lf >> (8 * k)) & 255u) == 255u || ((rt >> (8 * k)) & 255u) == 255u;
                if (x0 + k < W && g >= 0 && g <= p.free_max && unk) front |= 1u << k;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (x0 + k >= W) continue;
            const unsigned idx = (unsigned)(y * W + x0 + k);
            const bool f = (front >> k) & 1u;
            p.labels[base + idx] = f ? idx : FR_NONE;
            if (f) {
                p.count[base + idx] = 0u;
                p.sums[(base + idx) * 2] = 0ull;
                p.sums[(base + idx) * 2 + 1] = 0ull;
                p.rep[base + idx] = FR_NOKEY;
            }
        }
        nf = __popc(front);
    }
    nf = fr_wave_sum(nf);
    if ((threadIdx.x & 63) == 0 && nf) atomicAdd(p.info + (size_t)b * FR_INFO_WORDS + FR_CELLS, nf);
}

__global__ __launch_bounds__(FR_BLOCK) void k_frontier_label(FrontierParams p) {
    __shared__ unsigned s_par[FR_TILE];
    const int b = blockIdx.y, tid = threadIdx.x, W = p.width, H = p.height, cells = W * H;
    const int tiles_x = (W + FR_TW - 1) / FR_TW;
    const int x0 = ((int)blockIdx.x % tiles_x) * FR_TW, y0 = ((int)blockIdx.x / tiles_x) * FR_TH;
    unsigned* labels = p.labels + (size_t)b * cells;
    const int nfw = p.conn == 8 ? 4 : 2;                 // forward neighbours E, S, SE, SW as (dx, dy)
    int overrun = 0, any = 0;
    unsigned front = 0;                                  // bit k: this lane's cell k is a frontier cell
#pragma unroll
    for (int k = 0; k < FR_CPT; ++k) {
        const int li = tid + k * FR_BLOCK, gx = x0 + (li % FR_TW), gy = y0 + (li / FR_TW);
        const bool f = gx < W && gy < H && FR_LOAD(labels + gy * W + gx, __HIP_MEMORY_SCOPE_AGENT) != FR_NONE;
        s_par[li] = f ? (unsigned)li : FR_NONE;
        front |= f ? 1u << k : 0u;
        any |= f;
    }
    if (!__syncthreads_or(any)) return;                  // (the same answer in every lane)

    // phase one: the tile's own unions, in LDS
#pragma unroll
    for (int k = 0; k < FR_CPT; ++k) {
        if (!((front >> k) & 1u)) continue;
        const int li = tid + k * FR_BLOCK, lx = li % FR_TW, ly = li / FR_TW;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int nx = lx + (d == 3 ? -1 : d == 1 ? 0 : 1), ny = ly + (d == 0 ? 0 : 1);
            if (d >= nfw || nx < 0 || nx >= FR_TW || ny >= FR_TH) continue;
            const int nl = ny * FR_TW + nx;
            if (FR_LOAD(s_par + nl, __HIP_MEMORY_SCOPE_WORKGROUP) != FR_NONE)
                fr_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, (unsigned)li, (unsigned)nl, FR_TILE, &overrun);
        }
    }
    __syncthreads();

    // phase two: every cell with its tile root, and with its forward neighbours in other tiles, on the global array
#pragma unroll
    for (int k = 0; k < FR_CPT; ++k) {
        if (!((front >> k) & 1u)) continue;
        const int li = tid + k * FR_BLOCK, lx = li % FR_TW, ly = li / FR_TW;
        const int gx = x0 + lx, gy = y0 + ly;
        const unsigned g = (unsigned)(gy * W + gx);
        const int r = (int)fr_find<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, (unsigned)li, FR_TILE, &overrun);
        if (r != li)                                     // (a tile's cells lie in the same order locally and globally)
            fr_union<__HIP_MEMORY_SCOPE_AGENT>(labels, g, (unsigned)((y0 + r / FR_TW) * W + x0 + r % FR_TW), cells, &overrun);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int dx = d == 3 ? -1 : d == 1 ? 0 : 1, dy = d == 0 ? 0 : 1;
            const int nx = lx + dx, ny = ly + dy;
            if (d >= nfw || (nx >= 0 && nx < FR_TW && ny < FR_TH)) continue;     // inside the tile: phase one
            if (gx + dx < 0 || gx + dx >= W || gy + dy >= H) continue;
            const unsigned gn = (unsigned)((gy + dy) * W + gx + dx);
            if (FR_LOAD(labels + gn, __HIP_MEMORY_SCOPE_AGENT) != FR_NONE)
                fr_union<__HIP_MEMORY_SCOPE_AGENT>(labels, g, gn, cells, &overrun);
        }
    }
    if (overrun) p.info[(size_t)b * FR_INFO_WORDS + FR_OVERRUN] = 1;
}

__global__ __launch_bounds__(FR_BLOCK) void k_frontier_stats(FrontierParams p) {
    const int b = blockIdx.y, W = p.width, cells = W * p.height, lane = threadIdx.x & 63;
    const int i = (int)blockIdx.x * FR_BLOCK + (int)threadIdx.x;
    const size_t base = (size_t)b * cells;
    unsigned* labels = p.labels + base;
    int* info = p.info + (size_t)b * FR_INFO_WORDS;
    int overrun = 0;
    unsigned r = FR_NONE;
    if (i < cells && FR_LOAD(labels + i, __HIP_MEMORY_SCOPE_AGENT) != FR_NONE) {
        r = fr_find<__HIP_MEMORY_SCOPE_AGENT>(labels, (unsigned)i, cells, &overrun);
        __hip_atomic_store(labels + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // the flatten: a lane on its way through i finds the old parent or the root
        if (r == (unsigned)i) p.roots[base + (unsigned)atomicAdd(info + FR_CLUSTERS, 1)] = r;
    }
    const bool f = r != FR_NONE;
    const unsigned long long m = __ballot(f);
    if (m) {                                             // (wave-uniform)
        const unsigned r0 = (unsigned)__shfl((int)r, __ffsll((long long)m) - 1);
        const int x = f ? i % W : 0, y = f ? i / W : 0;
        if (__all(!f || r == r0)) {                      // one root in the wave: one lane adds for all
            const int sx = fr_wave_sum(x), sy = fr_wave_sum(y);
            if (lane == __ffsll((long long)m) - 1) {
                atomicAdd(p.count + base + r0, (unsigned)__popcll(m));
                atomicAdd(p.sums + (base + r0) * 2, (unsigned long long)sx);
                atomicAdd(p.sums + (base + r0) * 2 + 1, (unsigned long long)sy);
            }
        } else if (f) {
            atomicAdd(p.count + base + r, 1u);
            atomicAdd(p.sums + (base + r) * 2, (unsigned long long)x);
            atomicAdd(p.sums + (base + r) * 2 + 1, (unsigned long long)y);
        }
    }
    if (overrun) info[FR_OVERRUN] = 1;
}

__global__ __launch_bounds__(FR_BLOCK) void k_frontier_rep(FrontierParams p) {
    const int b = blockIdx.y, W = p.width, cells = W * p.height, lane = threadIdx.x & 63;
    const int i = (int)blockIdx.x * FR_BLOCK + (int)threadIdx.x;
    const size_t base = (size_t)b * cells;
    const unsigned r = i < cells ? p.labels[base + i] : FR_NONE;
    const bool f = r != FR_NONE;
    unsigned long long key = FR_NOKEY;
    if (f) {
        const unsigned long long n = p.count[base + r], sx = p.sums[(base + r) * 2], sy = p.sums[(base + r) * 2 + 1];
        const long long cx = (long long)((2 * sx + n) / (2 * n)), cy = (long long)((2 * sy + n) / (2 * n));
        const long long dx = i % W - cx, dy = i / W - cy;
        key = ((unsigned long long)(dx * dx + dy * dy) << 20) | (unsigned)i;
    }
    const unsigned long long m = __ballot(f);
    if (m) {
        const int first = __ffsll((long long)m) - 1;
        const unsigned r0 = (unsigned)__shfl((int)r, first);
        if (__all(!f || r == r0)) {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const unsigned long long o = __shfl_xor(key, s);
                key = o < key ? o : key;
            }
            if (lane == first) atomicMin(p.rep + base + r0, key);
        } else if (f) atomicMin(p.rep + base + r, key);
    }
}

// what select knows of a root: the sort key (FR_NOKEY where the cluster is dropped: *why 1 small, 2 unreached) and D
__device__ __forceinline__ unsigned long long fr_sort_key(const FrontierParams& p, int b, unsigned r, int* why, unsigned long long* D_out) {
    const int W = p.width;
    const size_t base = (size_t)b * W * p.height;
    const unsigned n = p.count[base + r];
    *why = 0;
    if (n < (unsigned)p.min_size) { *why = 1; return FR_NOKEY; }
    const unsigned cell = (unsigned)(p.rep[base + r] & 0xFFFFFu);
    const int x = (int)(cell % (unsigned)W), y = (int)(cell / (unsigned)W);
    if (y >= p.height) {                                 // no member left its key: cannot happen behind rep; the getter refuses the run
        p.info[(size_t)b * FR_INFO_WORDS + FR_OVERRUN] = 1;
        *why = 1;
        return FR_NOKEY;
    }
    unsigned long long D;
    if (p.use_field) {
        const unsigned v = p.pot[(size_t)b * p.pot_stride + (size_t)y * p.pot_pitch + x];
        if (v == PP_NAVFN_UNREACHED) { *why = 2; return FR_NOKEY; }
        D = v;
    } else {
        const FrontierCall c = p.call[b];
        const long long dx = (long long)x - c.rx, dy = (long long)y - c.ry;
        D = (unsigned long long)(dx * dx + dy * dy);
    }
    if (D_out) *D_out = D;
    return ((p.rank == 0 ? D : (unsigned long long)((1u << 20) - n)) << 20) | r;
}

// the eight words of root r as frontier k of grid b
__device__ __forceinline__ void fr_write_words(const FrontierParams& p, int b, int k, unsigned r) {
    const int W = p.width;
    const size_t base = (size_t)b * W * p.height;
    int why;
    unsigned long long D = 0;
    (void)fr_sort_key(p, b, r, &why, &D);
    const unsigned long long n = p.count[base + r], sx = p.sums[(base + r) * 2], sy = p.sums[(base + r) * 2 + 1];
    const unsigned cell = (unsigned)(p.rep[base + r] & 0xFFFFFu);
    int* w = p.words + ((size_t)b * PP_FRONTIER_MAX + k) * 8;
    w[0] = (int)(cell % (unsigned)W); w[1] = (int)(cell / (unsigned)W);
    w[2] = (int)((2 * sx + n) / (2 * n)); w[3] = (int)((2 * sy + n) / (2 * n));
    w[4] = (int)n; w[5] = (int)r; w[6] = (int)(unsigned)D; w[7] = (int)(unsigned)(D >> 32);
}

__global__ __launch_bounds__(FR_BLOCK) void k_frontier_select(FrontierParams p) {
    __shared__ unsigned long long s_key[FR_CACHE];
    __shared__ unsigned long long s_red[FR_BLOCK / 64];
    __shared__ int s_cnt[2];
    const int b = blockIdx.x, tid = threadIdx.x, cells = p.width * p.height;
    int* info = p.info + (size_t)b * FR_INFO_WORDS;
    int* words = p.words + (size_t)b * PP_FRONTIER_MAX * 8;
    const unsigned* roots = p.roots + (size_t)b * cells;
    const int nroots = min(info[FR_CLUSTERS], cells);
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    int returned = 0;
    if (nroots <= FR_BLOCK) {
        // a root per lane: the keys are distinct, so a key's place in the order is the number of keys below it
        int why = 0;
        const unsigned r = tid < nroots ? roots[tid] : 0u;
        const unsigned long long key = tid < nroots ? fr_sort_key(p, b, r, &why, nullptr) : FR_NOKEY;
        s_key[tid] = key;
        if (why) atomicAdd(&s_cnt[why - 1], 1);
        __syncthreads();
        int place = 0;
        for (int j = 0; j < nroots; ++j) place += s_key[j] < key;
        if (key != FR_NOKEY && place < p.max_frontiers) fr_write_words(p, b, place, r);
        returned = min(nroots - s_cnt[0] - s_cnt[1], p.max_frontiers);
    } else {
        // max_frontiers passes, each the least key above the last; entry j of s_key is written and read by lane
        // j % FR_BLOCK alone
        unsigned long long last = 0;
        for (int k = 0; k < p.max_frontiers; ++k) {
            unsigned long long best = FR_NOKEY;
            int small = 0, unreached = 0;
            for (int j = tid; j < nroots; j += FR_BLOCK) {
                unsigned long long key;
                if (k > 0 && j < FR_CACHE) key = s_key[j];
                else {
                    int why;
                    key = fr_sort_key(p, b, roots[j], &why, nullptr);
                    small += why == 1;
                    unreached += why == 2;
                    if (j < FR_CACHE) s_key[j] = key;
                }
                if ((k == 0 || key > last) && key < best) best = key;
            }
            if (k == 0) {
                if (small) atomicAdd(&s_cnt[0], small);
                if (unreached) atomicAdd(&s_cnt[1], unreached);
            }
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const unsigned long long o = __shfl_xor(best, s);
                best = o < best ? o : best;
            }
            if ((tid & 63) == 0) s_red[tid >> 6] = best;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < FR_BLOCK / 64; ++w) best = s_red[w] < best ? s_red[w] : best;
            __syncthreads();                             // (s_red is written again in the next pass)
            if (best == FR_NOKEY) break;                 // (the same answer in every lane)
            if (tid == 0) fr_write_words(p, b, k, (unsigned)(best & 0xFFFFFu));
            last = best;
            ++returned;
        }
    }
    // (s_cnt was last added to before a barrier every lane has passed)
    for (int j = returned * 8 + tid; j < PP_FRONTIER_MAX * 8; j += FR_BLOCK) words[j] = 0;
    if (tid == 0) {
        info[FR_SMALL] = s_cnt[0];
        info[FR_UNREACHED] = s_cnt[1];
        info[FR_KEPT] = nroots - s_cnt[0] - s_cnt[1];
        info[FR_RETURNED] = returned;
    }
}

}  // namespace

void launch_frontier_select(const FrontierParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    PP_LAUNCH("k_frontier_select", k_frontier_select, dim3(p.batch), dim3(FR_BLOCK), 0, s, p);
}

void launch_frontier(const FrontierParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    const int W = p.width, H = p.height, cells = W * H;
    const int quads = (W + 3) / 4 * H;
    const int tiles = ((W + FR_TW - 1) / FR_TW) * ((H + FR_TH - 1) / FR_TH);
    const dim3 per_cell((cells + FR_BLOCK - 1) / FR_BLOCK, p.batch);
    PP_LAUNCH("k_frontier_mark", k_frontier_mark, dim3((quads + FR_BLOCK - 1) / FR_BLOCK, p.batch), dim3(FR_BLOCK), 0, s, p);
    PP_LAUNCH("k_frontier_label", k_frontier_label, dim3(tiles, p.batch), dim3(FR_BLOCK), 0, s, p);
    PP_LAUNCH("k_frontier_stats", k_frontier_stats, per_cell, dim3(FR_BLOCK), 0, s, p);
    PP_LAUNCH("k_frontier_rep", k_frontier_rep, per_cell, dim3(FR_BLOCK), 0, s, p);
    launch_frontier_select(p, s);
}
