// Live-camera ingest (pp_ingest_pointcloud2*): raw sensor_msgs/PointCloud2 bytes -> the float32 [sum n_b, 3] lidar-frame
// points and the frame offsets the voxeliser reads, without the host touching a point.  Restates
// ingest.pointcloud2_to_xyz(...)[first::decimate] followed by ingest.realsense_to_lidar (load_data.py:2433-2443):
//
//   record i = row * width + col of a frame sits at row * row_step + col * point_step; x y z are read at their field
//   offsets (FLOAT32 or FLOAT64, either byte order, no alignment assumed);
//   a record is finite when its three coordinates are; rank = finite records before it in message order;
//   it is kept when finite, rank >= first and (rank - first) % decimate == 0, as output row (rank - first) / decimate;
//   a kept point becomes ((p . r) . r2) + lift in float64 -- every 3-term dot product summed left to right, no fused
//   multiply-add, which is what numpy's dot computes for these shapes -- and is rounded to float32 once.
//
// Three launches, ordered by the stream alone (no workgroup waits for another):
//   k_ingest_count    one wave per chunk of ING_CHUNK records: ballot + popcount of the finite flags -> chunk counts
//   k_ingest_scan     one workgroup: a wave per frame scans its chunk counts -> chunk bases, the frame's finite and kept
//                     counts; then the frame offsets
//   k_ingest_scatter  re-reads the chunks; a finite record's rank is its chunk's base + the finite lanes below it
//
// pp_ingest_pointcloud2_fields* (rows of F > 3 floats): the count and the scan are the same launches -- validity is x y z's
// alone --, and k_ingest_scatter_f<F> writes x y z and the frame's F - 3 feature columns (ingest_dev.h: ing_feature) as one
// row, one 16-byte store for F = 4.
#include "pp_common.h"
#include "ingest_dev.h"

namespace {

// (the chunking and the per-record decode / validity functions: ingest_dev.h, shared with rig_ingest.hip)
__global__ __launch_bounds__(PP_WAVE * ING_WAVES) void k_ingest_count(const uint8_t* __restrict__ raw,
                                                                     const IngFrame* __restrict__ frames, int stride,
                                                                     int* __restrict__ chunk_cnt) {
    const int b = blockIdx.y;
    const IngFrame f = frames[b];
    const int lane = threadIdx.x & (PP_WAVE - 1);
    const int c = blockIdx.x * ING_WAVES + (threadIdx.x >> 6);
    if (c >= f.nchunks) return;                    // (the same for every lane of the wave)
    const uint8_t* base = raw + f.byte_off;
    int cnt = 0;
#pragma unroll 2
    for (int k = 0; k < ING_ITER; ++k) {
        const int i = c * ING_CHUNK + k * PP_WAVE + lane;
        double p[3];
        const bool fin = i < f.n_rec && ing_read(base, f, i, p);
        cnt += __popcll(__ballot(fin));
    }
    if (lane == 0) chunk_cnt[(size_t)b * stride + c] = cnt;
}

// One workgroup of 16 waves; wave w scans frames w, w + 16, ...; thread 0 then sums the kept counts into the offsets
// (ingest_dev.h: the depth-image ingest runs the same scan).
__global__ __launch_bounds__(1024) void k_ingest_scan(const IngFrame* __restrict__ frames, int batch, int stride,
                                                      int first, int decimate, const int* __restrict__ chunk_cnt,
                                                      int* __restrict__ chunk_base, int* __restrict__ finite,
                                                      int* __restrict__ kept, int* __restrict__ offsets) {
    ingest_scan_frames(frames, batch, stride, first, decimate, chunk_cnt, chunk_base, finite, kept, offsets);
}

__global__ __launch_bounds__(PP_WAVE * ING_WAVES) void k_ingest_scatter(const uint8_t* __restrict__ raw,
                                                                       const IngFrame* __restrict__ frames, int stride,
                                                                       int first, int decimate, IngXform xf,
                                                                       const int* __restrict__ chunk_base,
                                                                       const int* __restrict__ offsets,
                                                                       float* __restrict__ out, long long out_rows) {
    const int b = blockIdx.y;
    const IngFrame f = frames[b];
    const int lane = threadIdx.x & (PP_WAVE - 1);
    const int c = blockIdx.x * ING_WAVES + (threadIdx.x >> 6);
    if (c >= f.nchunks) return;
    const uint8_t* base = raw + f.byte_off;
    const long long row0 = offsets[b];
    int run = chunk_base[(size_t)b * stride + c];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k = 0; k < ING_ITER; ++k) {
        const int i = c * ING_CHUNK + k * PP_WAVE + lane;
        double p[3];
        const bool fin = i < f.n_rec && ing_read(base, f, i, p);
        const unsigned long long m = __ballot(fin);
        const int r = run + __popcll(m & below) - first;
        run += __popcll(m);
        if (fin && r >= 0 && r % decimate == 0) {
            const long long row = row0 + r / decimate;
            if (row < out_rows) {                  // (always: the host sized the call from the frames' bounds)
                float o[3];
                ing_transform(p, xf, o);
                out[row * 3 + 0] = o[0];
                out[row * 3 + 1] = o[1];
                out[row * 3 + 2] = o[2];
            }
        }
    }
}

// k_ingest_scatter for rows of F floats: columns 3 ... F - 1 are the frame's feature columns feats[b][0 ... F - 4]
template <int F>
__global__ __launch_bounds__(PP_WAVE * ING_WAVES) void k_ingest_scatter_f(const uint8_t* __restrict__ raw,
                                                                         const IngFrame* __restrict__ frames,
                                                                         const IngFeat* __restrict__ feats, int stride,
                                                                         int first, int decimate, IngXform xf,
                                                                         const int* __restrict__ chunk_base,
                                                                         const int* __restrict__ offsets,
                                                                         float* __restrict__ out, long long out_rows) {
    const int b = blockIdx.y;
    const IngFrame f = frames[b];
    const int lane = threadIdx.x & (PP_WAVE - 1);
    const int c = blockIdx.x * ING_WAVES + (threadIdx.x >> 6);
    if (c >= f.nchunks) return;
    IngFeat ft[F - 3];
#pragma unroll
    for (int j = 0; j < F - 3; ++j) ft[j] = feats[(size_t)b * (F - 3) + j];
    const uint8_t* base = raw + f.byte_off;
    const long long row0 = offsets[b];
    int run = chunk_base[(size_t)b * stride + c];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k = 0; k < ING_ITER; ++k) {
        const int i = c * ING_CHUNK + k * PP_WAVE + lane;
        double p[3];
        const bool fin = i < f.n_rec && ing_read(base, f, i, p);
        const unsigned long long m = __ballot(fin);
        const int r = run + __popcll(m & below) - first;
        run += __popcll(m);
        if (fin && r >= 0 && r % decimate == 0) {
            const long long row = row0 + r / decimate;
            if (row < out_rows) {                  // (always: the host sized the call from the frames' bounds)
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

}  // namespace

int ingest_chunks(int n_rec) { return (n_rec + ING_CHUNK - 1) / ING_CHUNK; }

void launch_ingest(const IngestParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    const dim3 grid((p.stride + ING_WAVES - 1) / ING_WAVES, p.batch), block(PP_WAVE * ING_WAVES);
    if (p.stride > 0)
        PP_LAUNCH("k_ingest_count", k_ingest_count, grid, block, 0, s, p.raw, p.frames, p.stride, p.chunk_cnt);
    PP_LAUNCH("k_ingest_scan", k_ingest_scan, dim3(1), dim3(1024), 0, s, p.frames, p.batch, p.stride, p.first, p.decimate,
              p.chunk_cnt, p.chunk_base, p.finite, p.kept, p.offsets);
    if (p.stride > 0) {
        const IngXform xf = ing_xform_of(p);
        if (p.nfeat == 0)
            PP_LAUNCH("k_ingest_scatter", k_ingest_scatter, grid, block, 0, s, p.raw, p.frames, p.stride, p.first, p.decimate,
                      xf, p.chunk_base, p.offsets, p.out, p.out_rows);
        else            // (nfeat == 1: the C-ABI holds nfeat to F - 3 and pp_create F to 3 or 4)
            PP_LAUNCH("k_ingest_scatter_f<4>", k_ingest_scatter_f<4>, grid, block, 0, s, p.raw, p.frames, p.feats, p.stride,
                      p.first, p.decimate, xf, p.chunk_base, p.offsets, p.out, p.out_rows);
    }
}
