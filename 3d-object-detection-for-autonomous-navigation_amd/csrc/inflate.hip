// Obstacle inflation of an int8 OccupancyGrid (pp_set_inflation / pp_inflate_async / pp_inflate_grids; inflation.py states
// the rule).  One launch whatever the batch (grid y = stream / grid index); a workgroup owns a tile of 64 columns x 32 rows:
//   rows     for every row of the tile and of the R rows above and below it, a wave turns its 64 cells, and the 64 to either
//            side, into three 64-bit obstacle words by ballot; a cell's distance to the nearest obstacle of its own row is
//            then a count of trailing / leading zeros on those words, capped at R + 1 ("none"), one byte in LDS
//   columns  a lane per column of a wave's 8 tile rows: the minimum over dy of h[y + dy][x]^2 + dy^2 for each of them from
//            8 + 2R LDS bytes -- the exact squared Euclidean distance in cells, O(R) per cell -- then the cost through
//            the table and the compose
// A row outside the grid, and a cell right of its width (the padding of a pitched row), holds no obstacle.  Everything is
// integer arithmetic; the table comes from the host.  The two counts per grid are integer atomics of per-wave sums, so the
// same input gives the same bytes on every run.
#include "pp_common.h"

namespace {

constexpr int INFL_TW = 64, INFL_TH = 32, INFL_BLOCK = 256, INFL_WAVES = INFL_BLOCK / 64;
constexpr int INFL_UNROLL = 4;          // rows a wave loads before it ballots
constexpr int INFL_RPW = INFL_TH / INFL_WAVES;      // tile rows per wave in the column pass
constexpr int INFL_TABLE = PP_INFLATE_MAX_RADIUS * PP_INFLATE_MAX_RADIUS + 1;
static_assert(PP_INFLATE_MAX_RADIUS <= 64, "a row's nearest obstacle within R is looked for in three 64-bit words");
static_assert(PP_INFLATE_MAX_RADIUS + 1 <= 255, "a row distance is one byte");

__global__ __launch_bounds__(INFL_BLOCK) void k_inflate(InflParams p) {
    __shared__ unsigned char s_h[(INFL_TH + 2 * PP_INFLATE_MAX_RADIUS) * INFL_TW];      // 10 KiB
    __shared__ int8_t s_table[(INFL_TABLE + 3) & ~3];                                   // 4 KiB
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = p.width, H = p.height, R = p.R, R2 = R * R;
    const int tiles_x = (W + INFL_TW - 1) / INFL_TW;
    const int x0 = ((int)blockIdx.x % tiles_x) * INFL_TW, y0 = ((int)blockIdx.x / tiles_x) * INFL_TH;
    const int8_t* in = p.in[p.occ_call ? 1 - p.occ_call[b].src : 0] + (size_t)b * p.in_stride;
    const int x = x0 + lane;
    for (int i = tid; i <= R2; i += INFL_BLOCK) s_table[i] = p.table[i];

    // rows: h = distance in cells to the nearest obstacle of the cell's own row, R + 1 where there is none within R
    // A wave takes INFL_UNROLL rows at a time and loads their cells before the first ballot, so the loads of a group are
    // in flight together (a ballot waits for its load: row by row, a wave would pay one memory round trip per row).
    const int rows = INFL_TH + 2 * R;
    for (int r0 = wave * INFL_UNROLL; r0 < rows; r0 += INFL_WAVES * INFL_UNROLL) {      // (r0 is the same in every lane of a wave)
        int v0[INFL_UNROLL], vp[INFL_UNROLL], vn[INFL_UNROLL];
#pragma unroll
        for (int u = 0; u < INFL_UNROLL; ++u) {
            const int gy = y0 - R + r0 + u;
            const bool inside = r0 + u < rows && gy >= 0 && gy < H;
            const int8_t* row = in + (size_t)(inside ? gy : 0) * p.in_pitch;
            v0[u] = inside && x < W ? row[x] : -1;
            vp[u] = inside && x >= INFL_TW ? row[x - INFL_TW] : -1;               // (x - 64 < x0 < W)
            vn[u] = inside && x + INFL_TW < W ? row[x + INFL_TW] : -1;
        }
#pragma unroll
        for (int u = 0; u < INFL_UNROLL; ++u) {
            if (r0 + u >= rows) break;
            const unsigned long long cur = __ballot(v0[u] >= p.lethal), prev = __ballot(vp[u] >= p.lethal),
                                     next = __ballot(vn[u] >= p.lethal);
            const unsigned long long right = cur >> lane, left = cur << (63 - lane);
            int dr = R + 1, dl = R + 1;
            if (right) dr = __builtin_ctzll(right);
            else if (next) dr = 64 - lane + __builtin_ctzll(next);
            if (left) dl = __builtin_clzll(left);
            else if (prev) dl = lane + 1 + __builtin_clzll(prev);
            s_h[(r0 + u) * INFL_TW + lane] = (unsigned char)min(min(dl, dr), R + 1);
        }
    }
    __syncthreads();

    // columns: a wave owns INFL_RPW consecutive tile rows and a lane one column of them.  Tile row t reads LDS rows
    // t .. t + 2R (dy = -R .. R); the lane walks the INFL_RPW + 2R rows of its wave once and feeds every byte to all of its
    // INFL_RPW minima.  Neither "none" nor a row further than R needs a test: (R + 1)^2 > R^2, so such a term never
    // lowers a minimum that starts at R^2 + 1.
    const int t0 = wave * INFL_RPW;
    int g[INFL_RPW], best[INFL_RPW];
#pragma unroll
    for (int j = 0; j < INFL_RPW; ++j) {
        const int gy = y0 + t0 + j;
        g[j] = x < W && gy < H ? in[(size_t)gy * p.in_pitch + x] : 0;
        best[j] = R2 + 1;
    }
    const unsigned char* col = s_h + t0 * INFL_TW + lane;
    for (int k = 0; k < INFL_RPW + 2 * R; ++k) {
        const int hv = col[k * INFL_TW], hv2 = hv * hv;
#pragma unroll
        for (int j = 0; j < INFL_RPW; ++j) {
            const int dy = k - R - j;
            best[j] = min(best[j], hv2 + dy * dy);
        }
    }
    int n_lethal = 0, n_raised = 0;
#pragma unroll
    for (int j = 0; j < INFL_RPW; ++j) {
        const int gy = y0 + t0 + j;
        const bool valid = x < W && gy < H;
        int o = g[j];
        if (valid) {
            const int cost = best[j] > R2 ? 0 : (int)s_table[best[j]];
            o = g[j] >= 0 ? max(g[j], cost) : (cost >= p.unknown_min ? cost : -1);
            const size_t at = (size_t)b * p.out_stride + (size_t)gy * p.out_pitch + x;
            p.out[at] = (int8_t)o;
            if (p.dist2) p.dist2[at] = (uint16_t)best[j];
        }
        n_lethal += __popcll(__ballot(valid && g[j] >= p.lethal));
        n_raised += __popcll(__ballot(valid && o != g[j]));
    }
    if (lane == 0) {
        if (n_lethal) atomicAdd(p.counts + 2 * b, n_lethal);
        if (n_raised) atomicAdd(p.counts + 2 * b + 1, n_raised);
    }
}

}  // namespace

void launch_inflate(const InflParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    const int tiles = ((p.width + INFL_TW - 1) / INFL_TW) * ((p.height + INFL_TH - 1) / INFL_TH);
    PP_LAUNCH("k_inflate", k_inflate, dim3(tiles, p.batch), dim3(INFL_BLOCK), 0, s, p);
}
