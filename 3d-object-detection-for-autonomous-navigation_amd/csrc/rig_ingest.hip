// Camera-rig ingest (pp_ingest_rig_*): S sources -- depth images, or PointCloud2 messages -- into B frames, each source
// under its own selection (first, decimate) and its own camera -> lidar transform.  The resident points of a frame are
// the kept points of its sources in source order, back to back; per source the rule is ingest.hip's / depth_ingest.hip's,
// restarted: validity, rank, selection, the float64 transform and the single rounding (ingest_dev.h holds the per-record
// functions all three translation units share).  Restates ingest.rig_depth_ingest_np / rig_ingest_np.
//
// Three launches whatever S is, ordered by the stream alone (no workgroup waits for another):
//   k_rig_count    grid (chunks, source): one wave per chunk of ING_CHUNK records -> chunk counts [S][stride]
//   k_rig_scan     one workgroup: a wave per source scans its chunk counts -> chunk bases, the source's finite and kept
//                  counts (its own first / decimate); then one thread walks the S sources and B frames once: out_base[s]
//                  = kept of the earlier sources of its frame, offsets[b] = kept of all sources in front of frame b, and the
//                  frames' sums for pp_ingest_info
//   k_rig_scatter  grid (chunks, source): a kept record of source s goes to row offsets[frame(s)] + out_base[s] +
//                  (rank - first) / decimate, transformed by the source's own matrices (read from the source table: S x 168
//                  bytes do not fit a kernel argument)
//
// pp_ingest_rig_pointcloud2_fields* (rows of F > 3 floats): the same count and scan, and k_rig_scatter_f<F>, which writes
// x y z and the source's F - 3 feature columns (ingest_dev.h: ing_feature) as one row, one 16-byte store for F = 4.
#include "pp_common.h"
#include "ingest_dev.h"

namespace {

// what the kernels need of either record type: records in all, validity (+ what the point is computed from), the point
__device__ __forceinline__ int rig_records(const IngFrame& f) { return f.n_rec; }
__device__ __forceinline__ int rig_records(const DepthFrame& f) { return f.n_pix; }
__device__ __forceinline__ bool rig_probe(const uint8_t* base, const IngFrame& f, int i, double p[3]) {
    return ing_read(base, f, i, p);
}
__device__ __forceinline__ bool rig_probe(const uint8_t* base, const DepthFrame& f, int i, double p[3]) {
    float z = 0.0f;
    const bool ok = dep_read(base, f, i, z);
    p[2] = (double)z;                              // (exact; rig_point narrows it back)
    return ok;
}
__device__ __forceinline__ void rig_point(const IngFrame&, int, double[3]) {}
__device__ __forceinline__ void rig_point(const DepthFrame& f, int i, double p[3]) { dep_deproject(f, i, (float)p[2], p); }

template <typename Frame>
__global__ __launch_bounds__(PP_WAVE * ING_WAVES) void k_rig_count(const uint8_t* __restrict__ raw,
                                                                  const Frame* __restrict__ frames, int stride,
                                                                  int* __restrict__ chunk_cnt) {
    const int s = blockIdx.y;
    const Frame f = frames[s];
    const int lane = threadIdx.x & (PP_WAVE - 1);
    const int c = blockIdx.x * ING_WAVES + (threadIdx.x >> 6);
    if (c >= f.nchunks) return;                    // (the same for every lane of the wave)
    const uint8_t* base = raw + f.byte_off;
    const int n = rig_records(f);
    int cnt = 0;
#pragma unroll 2
    for (int k = 0; k < ING_ITER; ++k) {
        const int i = c * ING_CHUNK + k * PP_WAVE + lane;
        double p[3];
        const bool ok = i < n && rig_probe(base, f, i, p);
        cnt += __popcll(__ballot(ok));
    }
    if (lane == 0) chunk_cnt[(size_t)s * stride + c] = cnt;
}

// One workgroup of 16 waves; wave w scans sources w, w + 16, ...; thread 0 then walks the sources and the frames once
// (S + B steps: S <= PP_RIG_MAX_SOURCES * max_batch).
template <typename Frame>
__global__ __launch_bounds__(1024) void k_rig_scan(const Frame* __restrict__ frames, const RigSource* __restrict__ src,
                                                   int sources, int batch, int stride, const int* __restrict__ chunk_cnt,
                                                   int* __restrict__ chunk_base, int* __restrict__ src_finite,
                                                   int* __restrict__ src_kept, int* __restrict__ out_base,
                                                   int* __restrict__ finite, int* __restrict__ kept,
                                                   int* __restrict__ offsets) {
    const int lane = threadIdx.x & (PP_WAVE - 1), wave = threadIdx.x >> 6;
    for (int s = wave; s < sources; s += 16) {
        const int nchunks = frames[s].nchunks;
        int carry = 0;
        for (int c0 = 0; c0 < nchunks; c0 += PP_WAVE) {
            const int c = c0 + lane;
            const int v = c < nchunks ? chunk_cnt[(size_t)s * stride + c] : 0;
            const int incl = wave_inclusive_scan(v);
            if (c < nchunks) chunk_base[(size_t)s * stride + c] = carry + incl - v;
            carry += __builtin_amdgcn_readlane(incl, PP_WAVE - 1);
        }
        if (lane == 0) {
            const int first = src[s].first, decimate = src[s].decimate;
            src_finite[s] = carry;
            src_kept[s] = carry > first ? (carry - first + decimate - 1) / decimate : 0;
        }
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        // (the host checked the frame map: it starts at 0, never decreases, skips no frame and ends at batch - 1)
        int off = 0, s = 0;
        for (int b = 0; b < batch; ++b) {
            offsets[b] = off;
            int base = 0, fin = 0;
            for (; s < sources && src[s].frame == b; ++s) {
                out_base[s] = base;
                base += src_kept[s];
                fin += src_finite[s];
            }
            finite[b] = fin;
            kept[b] = base;
            off += base;
        }
        offsets[batch] = off;
    }
}

template <typename Frame>
__global__ __launch_bounds__(PP_WAVE * ING_WAVES) void k_rig_scatter(const uint8_t* __restrict__ raw,
                                                                    const Frame* __restrict__ frames,
                                                                    const RigSource* __restrict__ src, int batch, int stride,
                                                                    const int* __restrict__ chunk_base,
                                                                    const int* __restrict__ out_base,
                                                                    const int* __restrict__ offsets,
                                                                    float* __restrict__ out, long long out_rows) {
    const int s = blockIdx.y;
    const Frame f = frames[s];
    const int lane = threadIdx.x & (PP_WAVE - 1);
    const int c = blockIdx.x * ING_WAVES + (threadIdx.x >> 6);
    if (c >= f.nchunks) return;
    const RigSource& g = src[s];
    const int frame = g.frame, first = g.first, decimate = g.decimate;
    if (frame < 0 || frame >= batch) return;       // (never: the host checked the frame map)
    IngXform xf;
#pragma unroll
    for (int k = 0; k < 9; ++k) { xf.r[k] = g.r[k]; xf.r2[k] = g.r2[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) xf.lift[k] = g.lift[k];
    const uint8_t* base = raw + f.byte_off;
    const int n = rig_records(f);
    const long long row0 = (long long)offsets[frame] + out_base[s];
    int run = chunk_base[(size_t)s * stride + c];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k = 0; k < ING_ITER; ++k) {
        const int i = c * ING_CHUNK + k * PP_WAVE + lane;
        double p[3];
        const bool ok = i < n && rig_probe(base, f, i, p);
        const unsigned long long m = __ballot(ok);
        const int r = run + __popcll(m & below) - first;
        run += __popcll(m);
        if (ok && r >= 0 && r % decimate == 0) {
            const long long row = row0 + r / decimate;
            if (row >= 0 && row < out_rows) {      // (always: the host sized the call from the sources' bounds)
                float o[3];
                rig_point(f, i, p);
                ing_transform(p, xf, o);
                out[row * 3 + 0] = o[0];
                out[row * 3 + 1] = o[1];
                out[row * 3 + 2] = o[2];
            }
        }
    }
}

// k_rig_scatter<IngFrame> for rows of F floats: columns 3 ... F - 1 are the source's feature columns feats[s][0 ... F - 4]
template <int F>
__global__ __launch_bounds__(PP_WAVE * ING_WAVES) void k_rig_scatter_f(const uint8_t* __restrict__ raw,
                                                                      const IngFrame* __restrict__ frames,
                                                                      const RigSource* __restrict__ src,
                                                                      const IngFeat* __restrict__ feats, int batch, int stride,
                                                                      const int* __restrict__ chunk_base,
                                                                      const int* __restrict__ out_base,
                                                                      const int* __restrict__ offsets,
                                                                      float* __restrict__ out, long long out_rows) {
    const int s = blockIdx.y;
    const IngFrame f = frames[s];
    const int lane = threadIdx.x & (PP_WAVE - 1);
    const int c = blockIdx.x * ING_WAVES + (threadIdx.x >> 6);
    if (c >= f.nchunks) return;
    const RigSource& g = src[s];
    const int frame = g.frame, first = g.first, decimate = g.decimate;
    if (frame < 0 || frame >= batch) return;       // (never: the host checked the frame map)
    IngXform xf;
#pragma unroll
    for (int k = 0; k < 9; ++k) { xf.r[k] = g.r[k]; xf.r2[k] = g.r2[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) xf.lift[k] = g.lift[k];
    IngFeat ft[F - 3];
#pragma unroll
    for (int j = 0; j < F - 3; ++j) ft[j] = feats[(size_t)s * (F - 3) + j];
    const uint8_t* base = raw + f.byte_off;
    const long long row0 = (long long)offsets[frame] + out_base[s];
    int run = chunk_base[(size_t)s * stride + c];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k = 0; k < ING_ITER; ++k) {
        const int i = c * ING_CHUNK + k * PP_WAVE + lane;
        double p[3];
        const bool ok = i < f.n_rec && ing_read(base, f, i, p);
        const unsigned long long m = __ballot(ok);
        const int r = run + __popcll(m & below) - first;
        run += __popcll(m);
        if (ok && r >= 0 && r % decimate == 0) {
            const long long row = row0 + r / decimate;
            if (row >= 0 && row < out_rows) {      // (always: the host sized the call from the sources' bounds)
                float o[F];
                ing_transform(p, xf, o);
                const uint8_t* rec = ing_record(base, f, i);
#pragma unroll
                for (int j = 0; j < F - 3; ++j) o[3 + j] = ing_feature(rec, ft[j], f.big_endian != 0);
                ing_store_row<F>(out, row, o);
            }
        }
    }
}

inline void launch_rig_scatter_f(const RigParamsT<DepthFrame>&, hipStream_t, dim3, dim3) {}    // (an image has no field)
inline void launch_rig_scatter_f(const RigParamsT<IngFrame>& p, hipStream_t s, dim3 grid, dim3 block) {
    // (nfeat == 1: the C-ABI holds nfeat to F - 3 and pp_create F to 3 or 4)
    PP_LAUNCH("k_rig_scatter_f<4>", k_rig_scatter_f<4>, grid, block, 0, s, p.raw, p.frames, p.src, p.feats, p.batch, p.stride,
              p.chunk_base, p.out_base, p.offsets, p.out, p.out_rows);
}

template <typename Frame>
void launch_rig(const RigParamsT<Frame>& p, hipStream_t s, const char* n_count, const char* n_scan, const char* n_scatter) {
    if (p.batch <= 0 || p.sources <= 0) return;
    const dim3 grid((p.stride + ING_WAVES - 1) / ING_WAVES, p.sources), block(PP_WAVE * ING_WAVES);
    if (p.stride > 0)
        PP_LAUNCH(n_count, k_rig_count<Frame>, grid, block, 0, s, p.raw, p.frames, p.stride, p.chunk_cnt);
    PP_LAUNCH(n_scan, k_rig_scan<Frame>, dim3(1), dim3(1024), 0, s, p.frames, p.src, p.sources, p.batch, p.stride, p.chunk_cnt,
              p.chunk_base, p.src_finite, p.src_kept, p.out_base, p.finite, p.kept, p.offsets);
    if (p.stride > 0 && p.nfeat > 0)
        launch_rig_scatter_f(p, s, grid, block);
    else if (p.stride > 0)
        PP_LAUNCH(n_scatter, k_rig_scatter<Frame>, grid, block, 0, s, p.raw, p.frames, p.src, p.batch, p.stride, p.chunk_base,
                  p.out_base, p.offsets, p.out, p.out_rows);
}

}  // namespace

void launch_rig_ingest(const RigParamsT<IngFrame>& p, hipStream_t s) {
    launch_rig(p, s, "k_rig_count<pc2>", "k_rig_scan<pc2>", "k_rig_scatter<pc2>");
}

void launch_rig_ingest(const RigParamsT<DepthFrame>& p, hipStream_t s) {
    launch_rig(p, s, "k_rig_count<depth>", "k_rig_scan<depth>", "k_rig_scatter<depth>");
}
