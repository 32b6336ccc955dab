// Multi-sweep accumulation (pp_sweeps_accumulate*): the resident frames [n_b, F] -> the resident frames plus their
// streams' stored sweeps, carried into the current sensor frame under the ego poses; then the original current frame is
// stored in its stream's ring.  sweeps.py states the rule and this file mirrors it operation for operation:
//
//   used sweeps: the stored ones, newest first, with 0 < stamp_c - stamp_s <= max_age (float64);
//   M = R_c^T R_s, every entry ((a0 b0 + a1 b1) + a2 b2); d = t_s - t_c; u = R_c^T d in the same order;
//   a stored row becomes x' = (float)(((M00 x + M01 y) + M02 z) + u0) on the widened float32 coordinates, column
//   time_feature = (float)(stamp_c - stamp_s) (0.0f in the current rows), every other column bitwise;
//   an output frame is cut at nmax rows; the push takes rows 0, j, 2j ... of the ORIGINAL frame, cut at capacity.
//
// Two launches, ordered by the stream alone (no atomics, no workgroup waits for another: the same calls give the same
// bytes):
//   k_sweep_plan  one workgroup.  A thread per frame selects the used slots and forms the counts and the truncation;
//                 wave 0 scans them into the packed output offsets and the frames' chunk bases; a thread per frame
//                 forms M, u and the frame's segments (current rows, each used sweep, the ring push) and writes the
//                 pushed slot's pose, stamp and row count; 16 lanes per segment cut it into chunks of SWEEP_CHUNK rows.
//   k_sweep_move  one chunk per workgroup, one row per lane: current rows, transformed history rows and the ring push
//                 are entries of the same table.  The grid is the HOST's bound on the chunk count (the frames' sizes
//                 are device values); workgroups past the device-side count exit.
// Bandwidth-bound: every row is read once and written once (the current rows twice: output and ring).  A chunk's table
// entry and its transform are read through wave-uniform addresses (scalar loads: they sit in SGPRs).
#include "pp_common.h"

namespace {

constexpr int PLAN_THREADS = 1024;

__device__ __forceinline__ int chunks_of(int n) { return (n + SWEEP_CHUNK - 1) / SWEEP_CHUNK; }

// the used sweeps of stream b, newest first
struct SweepSel {
    int n;
    int slot[PP_SWEEP_MAX], rows[PP_SWEEP_MAX];
    double dt[PP_SWEEP_MAX];
};

__device__ SweepSel sweep_select(const SweepParams& p, int b) {
#pragma clang fp contract(off)
    const int slots = p.history + 1;
    const int head = p.head[b];
    const double stamp_c = p.call[(size_t)b * 13 + 12];
    // every slot's record is loaded before any is judged: independent loads, one round trip instead of one per slot
    int valid[PP_SWEEP_MAX], cnt[PP_SWEEP_MAX];
    double stamp[PP_SWEEP_MAX];
#pragma unroll
    for (int k = 0; k < PP_SWEEP_MAX; ++k) {
        int sl = head - 1 - k;
        if (sl < 0) sl += slots;
        const size_t i = (size_t)b * slots + (k < p.history ? sl : 0);
        valid[k] = k < p.history ? p.slot_valid[i] : 0;
        cnt[k] = p.slot_cnt[i];
        stamp[k] = p.slot_stamp[i];
    }
    SweepSel s;
    s.n = 0;
#pragma unroll
    for (int k = 0; k < PP_SWEEP_MAX; ++k) {
        int sl = head - 1 - k;
        if (sl < 0) sl += slots;
        const double dt = stamp_c - stamp[k];
        if (valid[k] && dt > 0.0 && dt <= p.max_age) {
            s.slot[s.n] = sl;
            s.rows[s.n] = min(max(cnt[k], 0), p.capacity);
            s.dt[s.n] = dt;
            ++s.n;
        }
    }
    return s;
}

__device__ __forceinline__ int frame_rows(const SweepParams& p, int b) {
    return min(max(p.offsets_in[b + 1] - p.offsets_in[b], 0), p.nmax);
}

__device__ void sweep_transform(const double* __restrict__ c, const double* __restrict__ s, double dt, SweepXf* x) {
#pragma clang fp contract(off)
    double d[3];
    for (int k = 0; k < 3; ++k) d[k] = s[k * 4 + 3] - c[k * 4 + 3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) x->m[i * 3 + j] = (c[i] * s[j] + c[4 + i] * s[4 + j]) + c[8 + i] * s[8 + j];
        x->u[i] = (c[i] * d[0] + c[4 + i] * d[1]) + c[8 + i] * d[2];
    }
    x->dt = (float)dt;
    x->pad = 0;
}

__global__ __launch_bounds__(PLAN_THREADS) void k_sweep_plan(const SweepParams p) {
    const int tid = threadIdx.x, lane = tid & (PP_WAVE - 1), wave = tid >> 6;
    const int slots = p.history + 1, nseg = p.history + 2;
    const size_t Fr = (size_t)p.F;
    // counts
    for (int b = tid; b < p.batch; b += PLAN_THREADS) {
        const SweepSel s = sweep_select(p, b);
        const int n_cur = frame_rows(p, b);
        long long total = n_cur;
        int room = p.nmax - n_cur, chunks = chunks_of(n_cur);
        for (int k = 0; k < s.n; ++k) {
            const int take = min(s.rows[k], room);
            total += s.rows[k];
            room -= take;
            chunks += chunks_of(take);
        }
        const int out_n = p.nmax - room;
        const int n_full = (n_cur + p.decimate - 1) / p.decimate, n_push = min(n_full, p.capacity);
        chunks += chunks_of(n_push);
        p.count[b] = out_n;
        p.used[b] = s.n;
        p.truncated[b] = (int)(total - out_n);
        p.push_truncated[b] = n_full - n_push;
        p.frame_chunks[b] = chunks;
    }
    __threadfence_block();
    __syncthreads();
    if (wave == 0) {                                   // (whole: wave_inclusive_scan wants all 64 lanes)
        int off = 0, c = 0;
        for (int b0 = 0; b0 < p.batch; b0 += PP_WAVE) {
            const int b = b0 + lane;
            const int n = b < p.batch ? p.count[b] : 0, t = b < p.batch ? p.frame_chunks[b] : 0;
            const int n_incl = wave_inclusive_scan(n), t_incl = wave_inclusive_scan(t);
            if (b < p.batch) {
                p.offsets_out[b + 1] = off + n_incl;
                p.frame_chunks[b] = c + t_incl - t;
            }
            off += __builtin_amdgcn_readlane(n_incl, PP_WAVE - 1);
            c += __builtin_amdgcn_readlane(t_incl, PP_WAVE - 1);
        }
        if (lane == 0) {
            p.offsets_out[0] = 0;
            p.frame_chunks[p.batch] = c;
            *p.nchunks = min(c, p.chunk_cap);
        }
    }
    __threadfence_block();
    __syncthreads();
    // segments, transforms, the pushed slot's record
    for (int b = tid; b < p.batch; b += PLAN_THREADS) {
        const SweepSel s = sweep_select(p, b);
        const int n_cur = frame_rows(p, b);
        const double* call = p.call + (size_t)b * 13;
        const float* src_cur = p.in + (size_t)p.offsets_in[b] * Fr;
        float* dst = p.out + (size_t)p.offsets_out[b] * Fr;
        SweepChunk* seg = p.segs + (size_t)b * nseg;
        int* c0 = p.seg_chunk0 + (size_t)b * nseg;
        int c = p.frame_chunks[b];
        seg[0] = SweepChunk{src_cur, dst, n_cur, SWEEP_XF_CUR, 1, 0};
        c0[0] = c;
        c += chunks_of(n_cur);
        int room = p.nmax - n_cur, row = n_cur;
        for (int k = 0; k < p.history; ++k) {
            int take = 0, xi = 0;
            const float* src = nullptr;
            if (k < s.n) {
                const size_t i = (size_t)b * slots + s.slot[k];
                take = min(s.rows[k], room);
                xi = b * p.history + k;
                sweep_transform(call, p.slot_pose + i * 12, s.dt[k], p.xf + xi);
                src = p.ring + i * (size_t)p.capacity * Fr;
            }
            seg[1 + k] = SweepChunk{src, dst + (size_t)row * Fr, take, xi, 1, 0};
            c0[1 + k] = c;
            c += chunks_of(take);
            room -= take;
            row += take;
        }
        const int head = p.head[b];
        const size_t w = (size_t)b * slots + head;
        const int n_push = min((n_cur + p.decimate - 1) / p.decimate, p.capacity);
        seg[1 + p.history] = SweepChunk{src_cur, p.ring + w * (size_t)p.capacity * Fr, n_push, SWEEP_XF_PUSH, p.decimate, 0};
        c0[1 + p.history] = c;
        p.slot_cnt[w] = n_push;
        p.slot_valid[w] = 1;
        for (int k = 0; k < 12; ++k) p.slot_pose[w * 12 + k] = call[k];
        p.slot_stamp[w] = call[12];
        p.head[b] = head + 1 == slots ? 0 : head + 1;
    }
    __threadfence_block();
    __syncthreads();
    // chunks: 16 lanes per segment (64 segments at a time), a lane per chunk
    const int total_seg = p.batch * nseg;
    for (int g = tid >> 4; g < total_seg; g += PLAN_THREADS / 16) {
        const SweepChunk sg = p.segs[g];
        const int first = p.seg_chunk0[g], nc = chunks_of(sg.rows);
        for (int c = tid & 15; c < nc; c += 16) {
            if (first + c >= p.chunk_cap) break;          // (never: the host sized the table for its bounds)
            SweepChunk ch = sg;
            ch.src = sg.src + (size_t)c * SWEEP_CHUNK * sg.stride * Fr;
            ch.dst = sg.dst + (size_t)c * SWEEP_CHUNK * Fr;
            ch.rows = min(SWEEP_CHUNK, sg.rows - c * SWEEP_CHUNK);
            p.chunks[first + c] = ch;
        }
    }
}

// A row of FT floats moved with the widest access its width allows, as the frustum crop does: one 16-byte access for
// FT == 4 (every buffer sits on 16 bytes), one 12-byte access for FT == 3 (lanes back to back: the wave's rows are one
// contiguous run); FT == 0: any width F, a float at a time.
struct __attribute__((aligned(4))) SweepRow3 { float v[3]; };
constexpr int SWEEP_MAX_F = 16;

template <int FT>
__global__ __launch_bounds__(SWEEP_CHUNK) void k_sweep_move(const SweepChunk* __restrict__ chunks,
                                                            const int* __restrict__ nchunks,
                                                            const SweepXf* __restrict__ xf, int F, int tf) {
#pragma clang fp contract(off)
    if ((int)blockIdx.x >= *nchunks) return;
    const SweepChunk ch = chunks[blockIdx.x];
    const int r = threadIdx.x;
    if (r >= ch.rows) return;
    const int Fr = FT ? FT : F;
    constexpr int NR = FT ? FT : SWEEP_MAX_F;
    const float* src = ch.src + (size_t)r * ch.stride * Fr;
    float* dst = ch.dst + (size_t)r * Fr;
    float v[NR];
    if (FT == 4) {
        const float4 q = *reinterpret_cast<const float4*>(src);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else if (FT == 3) {
        const SweepRow3 q = *reinterpret_cast<const SweepRow3*>(src);
        v[0] = q.v[0]; v[1] = q.v[1]; v[2] = q.v[2];
    } else {
#pragma unroll
        for (int j = 0; j < NR; ++j) if (j < Fr) v[j] = src[j];
    }
    if (ch.xf != SWEEP_XF_PUSH) {
        float t = 0.f;
        if (ch.xf >= 0) {
            const SweepXf& X = xf[ch.xf];
            const double x = (double)v[0], y = (double)v[1], z = (double)v[2];
            v[0] = (float)(((X.m[0] * x + X.m[1] * y) + X.m[2] * z) + X.u[0]);
            v[1] = (float)(((X.m[3] * x + X.m[4] * y) + X.m[5] * z) + X.u[1]);
            v[2] = (float)(((X.m[6] * x + X.m[7] * y) + X.m[8] * z) + X.u[2]);
            t = X.dt;
        }
        if (tf >= 0) {
            if (FT == 4) v[3] = t;                  // (3 is the only spare column of a 4-float row)
            else {
#pragma unroll
                for (int j = 3; j < NR; ++j) if (j == tf) v[j] = t;
            }
        }
    }
    if (FT == 4) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else if (FT == 3) {
        SweepRow3 q;
        q.v[0] = v[0]; q.v[1] = v[1]; q.v[2] = v[2];
        *reinterpret_cast<SweepRow3*>(dst) = q;
    } else {
#pragma unroll
        for (int j = 0; j < NR; ++j) if (j < Fr) dst[j] = v[j];
    }
}

}  // namespace

int sweep_chunks(int n) { return (n + SWEEP_CHUNK - 1) / SWEEP_CHUNK; }

void launch_sweeps(const SweepParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    PP_LAUNCH("k_sweep_plan", k_sweep_plan, dim3(1), dim3(PLAN_THREADS), 0, s, p);
    if (p.chunk_bound <= 0) return;
    const dim3 grid(p.chunk_bound), block(SWEEP_CHUNK);
    const bool vec = (((uintptr_t)p.in | (uintptr_t)p.out | (uintptr_t)p.ring) & 15) == 0;
    if (p.F == 4 && vec)
        PP_LAUNCH("k_sweep_move", k_sweep_move<4>, grid, block, 0, s, p.chunks, p.nchunks, p.xf, p.F, p.time_feature);
    else if (p.F == 3)
        PP_LAUNCH("k_sweep_move", k_sweep_move<3>, grid, block, 0, s, p.chunks, p.nchunks, p.xf, p.F, p.time_feature);
    else
        PP_LAUNCH("k_sweep_move", k_sweep_move<0>, grid, block, 0, s, p.chunks, p.nchunks, p.xf, p.F, p.time_feature);
}
