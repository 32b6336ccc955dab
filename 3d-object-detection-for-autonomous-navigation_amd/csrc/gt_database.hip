// Building the ground-truth object database from the resident frames: the reference's
// create_groundtruth_database (create_data.py:365-551) and _calculate_num_points_in_gt (:28-93) -- every point of a
// frame against every labelled box of that frame, counted, cut out in the frame's order and centred on the box --
// restated in gt_database.py (build_objects_np).  Membership is decided in float64 in the reference's operation order
// (box_planes3; the build has -ffp-contract=off): inside iff ((x n0 + y n1) + z n2) + d < 0 for all six faces.
//
// k_gdb_planes   a thread per box: its six plane equations.
// k_gdb_members  <false>: the count pass.  A workgroup per chunk of kChunk consecutive points of a frame, a point per
//                lane.  The frame's boxes pass through LDS in tiles of kTile (planes + centres, 12.5 KB: the 48 KB of all
//                256 boxes would leave three workgroups per CU); every lane tests its point against every box of the
//                tile, a ballot + popcount per wave gives the (wave, box) counts, their sum the (chunk, box) count.
//                The cloud is read once per frame, whatever the number of boxes.
// k_gdb_chunks   a workgroup per frame, a thread per box: the exclusive scan of the box's chunk counts (in place: each
//                chunk's base inside its object) and the box's total (num_points_in_gt).
// k_gdb_offsets  one workgroup: the objects' offsets over (frame, box), an exclusive scan of the totals (DPP wave scans).
// k_gdb_members  <true>: the gather pass.  The same tests again (the lane keeps its 64 results of a tile in a bit mask);
//                a member point goes to offsets[object] + chunk base + (members of the earlier waves) + (members among
//                the lower lanes), so the points of an object keep the frame's order and no slot is claimed with an
//                atomic: the output is the same bytes on every run.  x y z are stored as (float)((double)p - centre).
#include <math.h>

#include <algorithm>

#include "pp_common.h"
#include "pp_geom.h"

namespace {

constexpr int kChunk = PP_GDB_CHUNK;
constexpr int kWaves = kChunk / PP_WAVE;
constexpr int kTile = 64;            // boxes per LDS tile: one bit each in a lane's 64-bit result mask

static_assert(PP_MAX_GT_PER_FRAME % kTile == 0 && PP_MAX_GT_PER_FRAME <= kChunk, "k_gdb_chunks: a thread per box");

__global__ __launch_bounds__(256) void k_gdb_planes(GdbParams p, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    GtsPlane& pl = p.planes[i];
    box_planes3(p.boxes + (size_t)i * 7, pl.n, pl.d);
}

template <bool GATHER>
__global__ __launch_bounds__(kChunk) void k_gdb_members(GdbParams p) {
    __shared__ double s_pl[kTile][24];        // n[6][3], d[6]
    __shared__ double s_c[kTile][3];
    __shared__ int s_wc[kWaves][kTile];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const int o0 = p.offsets[b];
    const int n = p.offsets[b + 1] - o0;
    if (chunk * kChunk >= n) return;           // uniform across the workgroup
    const int G = p.box_cnt[b], g0 = p.box_off[b];
    const int i = chunk * kChunk + tid;
    const bool live = i < n;
    const int wave = tid / PP_WAVE, lane = tid & (PP_WAVE - 1);
    const float* in = p.pts + ((size_t)o0 + (live ? i : 0)) * p.F;
    double x = 0.0, y = 0.0, z = 0.0;
    if (live) { x = in[0]; y = in[1]; z = in[2]; }
    int* cc = p.chunk_cnt + ((size_t)b * p.chunk_stride + chunk) * PP_MAX_GT_PER_FRAME;
    for (int t0 = 0; t0 < G; t0 += kTile) {
        const int nt = min(kTile, G - t0);
        __syncthreads();                       // the tile before has been consumed
        for (int k = tid; k < nt * 24; k += kChunk) {
            const int j = k / 24, q = k - j * 24;
            s_pl[j][q] = ((const double*)&p.planes[g0 + t0 + j])[q];
        }
        if (GATHER)
            for (int k = tid; k < nt * 3; k += kChunk) s_c[k / 3][k % 3] = p.boxes[(size_t)(g0 + t0 + k / 3) * 7 + k % 3];
        __syncthreads();
        unsigned long long mine = 0ull;
        for (int j = 0; j < nt; ++j) {
            const double* pl = s_pl[j];
            bool inside = live;
            for (int f = 0; f < 6 && inside; ++f)
                if (((x * pl[f * 3 + 0] + y * pl[f * 3 + 1]) + z * pl[f * 3 + 2]) + pl[18 + f] >= 0.0) inside = false;
            const unsigned long long m = __ballot(inside);
            if (lane == 0) s_wc[wave][j] = __popcll(m);
            if (inside) mine |= 1ull << j;
        }
        __syncthreads();
        if (!GATHER) {
            if (tid < nt) {
                int c = 0;
                for (int w = 0; w < kWaves; ++w) c += s_wc[w][tid];
                cc[t0 + tid] = c;
            }
            continue;
        }
        if (__ballot(mine != 0ull) == 0ull) continue;      // no member of this tile in the wave
        for (int j = 0; j < nt; ++j) {
            const bool member = (mine >> j) & 1ull;
            const unsigned long long m = __ballot(member);
            if (m == 0ull) continue;                        // uniform across the wave
            if (!member) continue;
            int rank = __popcll(m & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) rank += s_wc[w][j];
            const long long row = p.obj_off[g0 + t0 + j] + cc[t0 + j] + rank;
            float* out = p.out + (size_t)row * p.F;
            // a float32 array -= float64 centre: the difference in float64, rounded once
            out[0] = (float)(x - s_c[j][0]);
            out[1] = (float)(y - s_c[j][1]);
            out[2] = (float)(z - s_c[j][2]);
            for (int f = 3; f < p.F; ++f) out[f] = in[f];
        }
    }
}

__global__ __launch_bounds__(PP_MAX_GT_PER_FRAME) void k_gdb_chunks(GdbParams p) {
    const int b = blockIdx.x, j = threadIdx.x;
    if (j >= p.box_cnt[b]) return;
    const int n = p.offsets[b + 1] - p.offsets[b];
    const int nch = (n + kChunk - 1) / kChunk;
    int* cc = p.chunk_cnt + (size_t)b * p.chunk_stride * PP_MAX_GT_PER_FRAME + j;
    int run = 0;
    for (int c = 0; c < nch; ++c) {
        const int v = cc[(size_t)c * PP_MAX_GT_PER_FRAME];
        cc[(size_t)c * PP_MAX_GT_PER_FRAME] = run;
        run += v;
    }
    p.totals[p.box_off[b] + j] = run;
}

__global__ __launch_bounds__(256) void k_gdb_offsets(GdbParams p, int total) {
    __shared__ long long s_wave[4];
    const int tid = threadIdx.x;
    const int per = (total + 255) / 256;
    const int i0 = min(tid * per, total), i1 = min(i0 + per, total);
    int sum = 0;                                // a thread's run: <= 32 objects of <= max_points_per_frame points
    for (int i = i0; i < i1; ++i) sum += p.totals[i];
    // the 256 partial sums: 32-bit DPP scans inside the waves (a frame's objects hold <= 256 x its points, a wave of
    // partials <= 64 x 32 objects: the caller refuses batches whose bound leaves 31 bits), 64 bits across them
    const int incl = wave_inclusive_scan(sum);
    if ((tid & (PP_WAVE - 1)) == PP_WAVE - 1) s_wave[tid / PP_WAVE] = incl;
    __syncthreads();
    long long base = (long long)(incl - sum);
    for (int w = 0; w < tid / PP_WAVE; ++w) base += s_wave[w];
    for (int i = i0; i < i1; ++i) {
        p.obj_off[i] = base;
        base += p.totals[i];
    }
    if (tid == 255) p.obj_off[total] = base;
}

}  // namespace

void launch_gtdb_count(const GdbParams& p, int total_boxes, int max_n, hipStream_t s) {
    if (p.batch <= 0) return;
    if (total_boxes > 0)
        PP_LAUNCH("k_gdb_planes", k_gdb_planes, dim3((unsigned)((total_boxes + 255) / 256)), dim3(256), 0, s, p, total_boxes);
    if (total_boxes > 0 && max_n > 0)
        PP_LAUNCH("k_gdb_count", k_gdb_members<false>, dim3((unsigned)((max_n + kChunk - 1) / kChunk), (unsigned)p.batch),
                  dim3(kChunk), 0, s, p);
    if (total_boxes > 0)
        PP_LAUNCH("k_gdb_chunks", k_gdb_chunks, dim3((unsigned)p.batch), dim3(PP_MAX_GT_PER_FRAME), 0, s, p);
    PP_LAUNCH("k_gdb_offsets", k_gdb_offsets, dim3(1), dim3(256), 0, s, p, total_boxes);
}

void launch_gtdb_gather(const GdbParams& p, int max_n, hipStream_t s) {
    if (p.batch <= 0 || max_n <= 0) return;
    PP_LAUNCH("k_gdb_gather", k_gdb_members<true>, dim3((unsigned)((max_n + kChunk - 1) / kChunk), (unsigned)p.batch),
              dim3(kChunk), 0, s, p);
}
