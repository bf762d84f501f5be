// BEV rasteriser: point_cloud_2_top (lib/utils/read_lidar.py:10-115 == tools/read_lidar.py:10-115, ranges
// tools/read_lidar.py:121-123) for `num_frames` Velodyne clouds back to back -> (num_frames, H, W, C) maps behind three launches --
// clear, scatter, resolve -- whatever the batch.  The single-cloud entries are this body with one frame and no offsets.
// The reference assigns top[y, x, i] = z - height_range[0] and top[y, x, z_max] = reflectance slice by slice with numpy fancy
// indexing: among the points that hit the same (cell, slice) the LAST one in point order wins, and for the reflectance channel the
// last slice then the last point.  Deterministic here via atomicMax on keys written into the output buffer itself (as u32) until the
// resolve replaces them by values:
//   channels < z_max : key = index + 1
//   channel z_max    : key = slice << 27 | (index + 1)         (at most 32 slices)
// (a height written to channel z_max -- possible when (h1 - h0) / zres is not an integer -- is always overwritten by the same
// iteration's reflectance, read_lidar.py:109-112, so that channel only ever shows the reflectance).
// HBM-bound: one clear of the maps, P scattered atomics, one read of the maps and a write of the vectors a point fell into.
//   frames   frame b owns rows offsets[b] .. offsets[b + 1] of the concatenated clouds; frame_rows.h has the rule, and a row that
//            belongs to no frame is skipped.  Frame b of the output equals, bit for bit, the map of that frame's rows alone.
//   index    the key holds the row's index WITHIN ITS FRAME, p - offsets[b], so the order is per frame and the 27 bits bound a
//            frame (2^27 - 2 rows: a row further into its frame than that is skipped), not the batch: total_points goes to INT_MAX.
//   resolve  turns a key back into the global row offsets[b] + index.  A key is only ever written by a row p that passed
//            offsets[b] <= p < offsets[b + 1] and p < total_points in the scatter of the SAME call, which stored index = p - offsets[b]
//            below 2^27, so neither key form can carry into the other's bits; the resolve reads the same offsets[b] (nothing on the
//            stream writes them in between) and recovers exactly that p.  So every row it reads is below total_points whatever the
//            offsets hold, and every cell the scatter touches is frame lo < num_frames, cell < H * W: nothing in offsets_dev can
//            make the call read or write out of bounds.
//   traffic  an empty key is already the bit pattern of 0.0f, so the resolve stores only where a key is not zero (at 120 000 points
//            at most 240 000 of 3 250 809 elements), at the granularity it loads at: a 16-byte vector of four keys is stored whole when
//            any of the four is set and not at all otherwise -- 13 MB less written per frame than a resolve that stores every element.
//            DENSE stores every vector and gives the same bits; measured with the output buffers traded between the two it is
//            1.5 - 3 % slower.  It is exported as mv3d_point_cloud_2_top_batch_dense for tools/bev_batch_bench.py
//            alone, which times the two against each other.
//   layout   one frame of the MV3D map is 13 003 236 bytes = 4 mod 16, so inside a batch only every fourth frame starts on a
//            16-byte boundary.  Clear and resolve therefore run over the FLAT range of num_frames * H * W * C elements: `head` scalar
//            elements up to the first 16-byte boundary of top_dev, 16-byte vectors, `tail` scalar elements.  The body needs 4-byte
//            alignment of top_dev only.  All element indices are 64-bit (1024 frames x 3 250 809 elements > 2^31).
#include "bev_cell.h"       // BevParams, bev_params, and the cell / slice rule shared with bev_paper.hip
#include "common.h"
#include "frame_rows.h"

// zero keys: a workgroup clears 16 KB contiguous, four 16-byte stores per thread; workgroup 0 also clears the head / tail elements
// (at most 3 each) and the status word
__global__ __launch_bounds__(256) void bevb_clear_kernel(float *top, int head, long long nvec, int tail, int *status)
{
    float4 *body = reinterpret_cast<float4 *>(top + head);
    const long long base = (long long)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long long v = base + u * 256;
        if (v < nvec) body[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (blockIdx.x == 0) {
        const int t = threadIdx.x;
        if (t < head) top[t] = 0.0f;
        if (t < tail) top[head + 4 * nvec + t] = 0.0f;
        if (status && t == 0) *status = 0;
    }
}

// One thread per row of the concatenated clouds; n = H * W * C elements per frame.
__global__ __launch_bounds__(256) void bevb_scatter_kernel(const float *__restrict__ pts, const int *__restrict__ offsets, int nf, int P,
                                                           unsigned *keys, long long n, const BevParams q, int *status)
{
    __shared__ int s_off[MV3D_FV_MAX_FRAMES + 1];
    frame_rows_stage(s_off, offsets, nf, P);
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (unsigned)P) return;
    int lo;
    if (!frame_of_row(s_off, nf, p, lo)) return;
    const unsigned idx = p - (unsigned)s_off[lo];
    if (idx > BEVB_MAX_INDEX) return;
    const float4 v = reinterpret_cast<const float4 *>(pts)[p];
    long long pixel;
    bool out;
    if (!bev_cell_of(v, q, pixel, out)) return;                  // the range tests and the cell: bev_cell.h
    const double z = (double)v.z;
    unsigned *cell = keys + (long long)lo * n + pixel * q.Cd;
    for (int i = 0; i < q.nslice; ++i) {
        if (bev_in_slice(z, i, q)) {
            if (out) { if (status) atomicOr(status, 1); return; }
            if (i < q.zmax) atomicMax(&cell[i], idx + 1u);
            atomicMax(&cell[q.zmax], ((unsigned)i << 27) | (idx + 1u));
        }
    }
}

// flat element e (frame e / n, channel e % C because C divides n) with key `key` != 0 -> its value
__device__ __forceinline__ float bevb_value(const float *__restrict__ pts, const int *__restrict__ offsets, unsigned key, long long e,
                                            long long n, const BevParams &q)
{
    const int c = (int)((unsigned long long)e % (unsigned)q.Cd);
    const long long first = offsets ? (long long)offsets[(unsigned long long)e / (unsigned long long)n] : 0;
    const long long row = first + (long long)((c == q.zmax ? (key & 0x7FFFFFFu) : key) - 1u);
    return (c == q.zmax) ? pts[4 * row + 3] : (pts[4 * row + 2] - q.h0f);          // z - height_range[0] in f32 (:106)
}

// Two 16-byte key loads per thread (a workgroup reads 8 KB contiguous), each stored back as one 16-byte vector of values: DENSE stores
// every vector (the bench tool's yardstick), otherwise only those that hold a key (an empty key IS 0.0f; the entry).  Workgroup 0 also
// resolves the head / tail elements.
template <bool DENSE>
__global__ __launch_bounds__(256) void bevb_resolve_kernel(const float *__restrict__ pts, const int *__restrict__ offsets, float *top, int head,
                                                           long long nvec, int tail, long long n, const BevParams q)
{
    uint4 *body = reinterpret_cast<uint4 *>(top + head);
    const long long base = (long long)blockIdx.x * 512 + threadIdx.x;
    uint4 k[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const long long v = base + u * 256;
        k[u] = v < nvec ? body[v] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const long long v = base + u * 256;
        if (v >= nvec) continue;
        const unsigned key[4] = {k[u].x, k[u].y, k[u].z, k[u].w};
        if (!DENSE && !(key[0] | key[1] | key[2] | key[3])) continue;      // (four empty keys are the four zeros the map wants)
        const long long e = head + 4 * v;
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = key[j] ? bevb_value(pts, offsets, key[j], e + j, n, q) : 0.0f;
        reinterpret_cast<float4 *>(body)[v] = make_float4(o[0], o[1], o[2], o[3]);
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < head + tail) {
        const long long e = (int)threadIdx.x < head ? (long long)threadIdx.x : 4 * nvec + threadIdx.x;      // (head + 4 nvec + (t - head))
        const unsigned key = reinterpret_cast<const unsigned *>(top)[e];
        if (key) top[e] = bevb_value(pts, offsets, key, e, n, q);
    }
}

static int bevb_launch(const float *points_dev, const int32_t *offsets_dev, int num_frames, int total_points, const double *r,
                       float *top_dev, int32_t *status_dev, hipStream_t s, bool dense)
{
    if (num_frames < 0 || num_frames > MV3D_FV_MAX_FRAMES || total_points < 0) return MV3D_ERR_INVALID_ARG;
    if (num_frames == 0) return MV3D_OK;
    BevParams q;
    if (r) {
        if (!status_dev || !bev_params8(r, q)) return MV3D_ERR_INVALID_ARG;
    } else {
        bev_params_mv3d(q);                                              // tools/read_lidar.py:121-133 -> (601, 601, 9); no cell can fall outside
        status_dev = nullptr;
    }
    if ((!offsets_dev && num_frames != 1) || !top_dev || (total_points > 0 && !points_dev)) return MV3D_ERR_INVALID_ARG;
    if (((uintptr_t)points_dev & 15) != 0 || ((uintptr_t)top_dev & 3) != 0 || ((uintptr_t)offsets_dev & 3) != 0 || ((uintptr_t)status_dev & 3) != 0)
        return MV3D_ERR_INVALID_ARG;
    const long long n = (long long)q.Hd * q.Wd * q.Cd, total = n * num_frames;
    int head, tail;
    long long nvec;
    bev_flat_split(top_dev, total, head, nvec, tail);
    const long long clear_groups = nvec / 1024 + 1, resolve_groups = nvec / 512 + 1;
    if (resolve_groups > 0x7FFFFFFFll) return MV3D_ERR_INVALID_ARG;
    hipLaunchKernelGGL(bevb_clear_kernel, dim3((unsigned)clear_groups), dim3(256), 0, s, top_dev, head, nvec, tail, status_dev);
    if (total_points > 0) {
        hipLaunchKernelGGL(bevb_scatter_kernel, dim3(((unsigned)total_points + 255u) / 256u), dim3(256), 0, s, points_dev, offsets_dev,
                           num_frames, total_points, reinterpret_cast<unsigned *>(top_dev), n, q, status_dev);
        if (dense)
            hipLaunchKernelGGL(bevb_resolve_kernel<true>, dim3((unsigned)resolve_groups), dim3(256), 0, s, points_dev, offsets_dev, top_dev,
                               head, nvec, tail, n, q);
        else
            hipLaunchKernelGGL(bevb_resolve_kernel<false>, dim3((unsigned)resolve_groups), dim3(256), 0, s, points_dev, offsets_dev, top_dev,
                               head, nvec, tail, n, q);
    }
    return mv3d_launch_status();
}

extern "C" int mv3d_point_cloud_2_top_batch(const float *points_dev, const int32_t *offsets_dev, int num_frames, int total_points,
                                            const double *ranges8_host, float *top_dev, int32_t *status_dev, void *stream)
{
    return bevb_launch(points_dev, offsets_dev, num_frames, total_points, ranges8_host, top_dev, status_dev, (hipStream_t)stream, false);
}

extern "C" int mv3d_point_cloud_2_top_batch_dense(const float *points_dev, const int32_t *offsets_dev, int num_frames, int total_points,
                                                  const double *ranges8_host, float *top_dev, int32_t *status_dev, void *stream)
{
    return bevb_launch(points_dev, offsets_dev, num_frames, total_points, ranges8_host, top_dev, status_dev, (hipStream_t)stream, true);
}

// The single-cloud entries: the body above on ONE frame of num_points rows, no offsets.  What they refuse beyond it is their own
// contract (include/mv3d_hip.h), decided here before any launch: a cloud of 2^27 rows or more (the body would skip the rows behind
// 2^27 - 2), and a map that is not 16-byte aligned.
static int bev_single(const float *points_dev, int num_points, const double *r, float *top_dev, int *status_dev, void *stream)
{
    if (num_points < 0 || num_points >= (1 << 27) || ((uintptr_t)top_dev & 15) != 0) return MV3D_ERR_INVALID_ARG;
    return bevb_launch(points_dev, nullptr, 1, num_points, r, top_dev, status_dev, (hipStream_t)stream, false);
}

extern "C" int mv3d_point_cloud_2_top(const float *points_dev, int num_points, float *top_dev, void *stream)
{
    return bev_single(points_dev, num_points, nullptr, top_dev, nullptr, stream);
}

extern "C" int mv3d_point_cloud_2_top_shape(double res, double zres, double side_lo, double side_hi, double fwd_lo, double fwd_hi,
                                            double height_lo, double height_hi, int *dims)
{
    BevParams q;
    if (!dims || !bev_params(res, zres, side_lo, side_hi, fwd_lo, fwd_hi, height_lo, height_hi, q)) return MV3D_ERR_INVALID_ARG;
    dims[0] = q.Hd; dims[1] = q.Wd; dims[2] = q.Cd;
    return MV3D_OK;
}

extern "C" int mv3d_point_cloud_2_top_ranges(const float *points_dev, int num_points, double res, double zres, double side_lo, double side_hi,
                                             double fwd_lo, double fwd_hi, double height_lo, double height_hi, float *top_dev,
                                             int *status_dev, void *stream)
{
    const double r[8] = {res, zres, side_lo, side_hi, fwd_lo, fwd_hi, height_lo, height_hi};
    return bev_single(points_dev, num_points, r, top_dev, status_dev, stream);
}
