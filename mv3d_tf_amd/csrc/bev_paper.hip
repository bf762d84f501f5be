// The MV3D paper's bird's-eye-view encoding (section 3.1 of the paper) from `num_frames` Velodyne clouds back to
// back -> (num_frames, H, W, M + 2) maps behind three launches -- clear, scatter, resolve -- whatever the batch.  PARITY UNPINNED:
// the reference has no such raster (bev_raster.hip restates the one it has); the definition is this repository's, stated in plain
// Python in tests/bev_paper_restatement.py.
// Which rows are kept, their cell and their height slices are bev_raster.hip's, through the same functions (bev_cell.h): a row
// passes the two f32 range tests, falls into cell (yi, xi), and into the slice set S = { i < M : z in [height_i, height_i + zres) }
// (f64).  A row with empty S is dropped (NaN, +-inf, z outside the height range); a row with non-empty S whose cell lies outside
// the map sets *status and is dropped.  With M = nslice = ceil((h1 - h0) / zres):
//   channel i < M   max of z over the kept rows with i in S, stored as z - (float)h0
//   channel M       the reflectance, bit for bit, of the cell's winner: the kept row with the largest z (-0.0 == +0.0), among equal
//                   z the largest row index within the frame (the "last" rule of both other rasters)
//   channel M + 1   T[min(N, 63)], N = the kept rows of the cell, T[n] = (float)fmin(1, log(n + 1) / log(64)) computed on the HOST
//                   with libm (mv3d_bev_density_table) and handed to the resolve by value
// An empty cell is all zeros.  Maxima, a count and a tie rule on the row index: the map depends neither on the order of the rows
// nor on scheduling.
//   keys     the scatter writes into the output buffer itself (as u32) and the resolve replaces keys by values, as bev_raster.hip:
//            channel i < M: atomicMax of K(z) = mv3d_score_key(z), the order-preserving u32 image of a finite f32 with both zeros on
//            one key; K >= 0x00800000 for every finite z, so 0 means empty.  Channel M + 1: atomicAdd of 1, the count.  Channel M
//            stays 0 until the resolve.  The winner is ONE 64-bit atomicMax per row on K(z) << 32 | (index + 1) in the caller's
//            workspace, 8 bytes per cell and frame (601 x 601: 2.9 MB a frame): larger z first, then the larger index.
//   index    the row's index WITHIN ITS FRAME, at most 2^27 - 2 (BEVB_MAX_INDEX: a row further into its frame is skipped), the bound
//            bev_raster.hip has, so that a frame's rows are the same set under both encodings.
//   bounds   the scatter touches frame lo < num_frames (frame_rows.h) and, unless `out`, cell < H * W, of output and workspace.  The
//            resolve reads workspace word e / C for element e < num_frames * H * W * C, i.e. below num_frames * H * W.  A non-zero
//            winner word was written by a row p that passed offsets[lo] <= p < offsets[lo + 1] and p < total_points in the scatter
//            of the SAME call (the clear zeroed the whole workspace before it, so nothing stale survives), with index = p -
//            offsets[lo]; the resolve reads the same offsets[lo] (nothing on the stream writes them in between) and recovers that
//            p < total_points.  So nothing in offsets_dev can make the call read or write outside its buffers.
//   traffic  one clear of maps and workspace, three or more atomics per kept row (one per slice hit, the count, the winner), one
//            read of the maps plus the workspace words of channel M, and a 16-byte store of each vector a point fell into (an empty
//            key IS 0.0f).  One frame is 14 448 040 bytes = 8 mod 16, so inside a batch every second frame starts off a 16-byte
//            boundary: clear and resolve walk the FLAT element range as head / vectors / tail (bev_cell.h), top_dev needs 4-byte
//            alignment only, and all element indices are 64-bit.
#include "bev_cell.h"
#include "common.h"
#include "frame_rows.h"

struct BevDensity { float t[64]; };

// T[n] = (float)fmin(1, log(n + 1) / log(64)), n = 0 .. 63, libm on the host
extern "C" int mv3d_bev_density_table(float *out64)
{
    if (!out64) return MV3D_ERR_INVALID_ARG;
    for (int n = 0; n < 64; ++n) out64[n] = (float)fmin(1.0, log((double)(n + 1)) / log(64.0));
    return MV3D_OK;
}

// zero keys and winners: workgroups [0, top_groups) clear 16 KB of the maps each (four 16-byte stores per thread), the rest 16 KB of
// the workspace each; workgroup 0 also clears the maps' head / tail elements, the workspace's odd last word and the status word
__global__ __launch_bounds__(256) void bevp_clear_kernel(float *top, int head, long long nvec, int tail, unsigned top_groups,
                                                         unsigned long long *ws, long long nws, int *status)
{
    if (blockIdx.x < top_groups) {
        float4 *body = reinterpret_cast<float4 *>(top + head);
        const long long base = (long long)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long v = base + u * 256;
            if (v < nvec) body[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        ulonglong2 *body = reinterpret_cast<ulonglong2 *>(ws);
        const long long base = (long long)(blockIdx.x - top_groups) * 1024 + threadIdx.x;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long v = base + u * 256;
            if (v < nws / 2) body[v] = make_ulonglong2(0ull, 0ull);
        }
    }
    if (blockIdx.x == 0) {
        const int t = threadIdx.x;
        if (t < head) top[t] = 0.0f;
        if (t < tail) top[head + 4 * nvec + t] = 0.0f;
        if (t == 0 && (nws & 1)) ws[nws - 1] = 0ull;
        if (status && t == 0) *status = 0;
    }
}

// One thread per row of the concatenated clouds; n = H * W * C elements and hw = H * W winner words per frame, C = M + 2.
__global__ __launch_bounds__(256) void bevp_scatter_kernel(const float *__restrict__ pts, const int *__restrict__ offsets, int nf, int P,
                                                           unsigned *keys, unsigned long long *ws, long long n, long long hw,
                                                           const BevParams q, int *status)
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
    const int M = q.nslice;
    unsigned *cell = keys + (long long)lo * n + pixel * (M + 2);
    unsigned key = 0u;                                           // K(z) once the row is known to be kept (z is finite then)
    for (int i = 0; i < M; ++i) {
        if (bev_in_slice(z, i, q)) {
            if (out) { if (status) atomicOr(status, 1); return; }
            key = mv3d_score_key(v.z);
            atomicMax(&cell[i], key);
        }
    }
    if (!key) return;                                            // empty S: dropped, not counted
    atomicAdd(&cell[M + 1], 1u);
    atomicMax(&ws[(long long)lo * hw + pixel], ((unsigned long long)key << 32) | (unsigned long long)(idx + 1u));
}

// K(z) -> z (the zeros come back as +0.0f)
__device__ __forceinline__ float bevp_unkey(unsigned key)
{
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// flat element e = (frame * H * W + pixel) * C + c, given as cellw = e / C and c = e % C, with the word `key` the scatter left there
// (0 in channel M) -> its value; 0.0f for an empty one
__device__ __forceinline__ float bevp_value(const float *__restrict__ pts, const int *__restrict__ offsets, const unsigned long long *__restrict__ ws,
                                            unsigned key, long long cellw, int c, long long hw, const BevParams &q, const float *tab)
{
    const int M = q.nslice;
    if (c < M) return key ? bevp_unkey(key) - q.h0f : 0.0f;                          // max z - height_range[0], one f32 subtraction
    if (c == M + 1) return key ? tab[key < 63u ? key : 63u] : 0.0f;                  // the count -> T[min(N, 63)]
    const unsigned long long w = ws[cellw];
    if (!w) return 0.0f;
    const long long first = offsets ? (long long)offsets[(unsigned long long)cellw / (unsigned long long)hw] : 0;
    const long long row = first + (long long)((unsigned)(w & 0xFFFFFFFFull) - 1u);
    return pts[4 * row + 3];
}

// Two 16-byte key loads per thread (a workgroup reads 8 KB contiguous), each stored back as one 16-byte vector of values where one
// of the four holds a key or a value.  Workgroup 0 also resolves the head / tail elements.
__global__ __launch_bounds__(256) void bevp_resolve_kernel(const float *__restrict__ pts, const int *__restrict__ offsets,
                                                           const unsigned long long *__restrict__ ws, float *top, int head, long long nvec,
                                                           int tail, long long hw, const BevParams q, const BevDensity dens)
{
    __shared__ float s_tab[64];
    if (threadIdx.x < 64) s_tab[threadIdx.x] = dens.t[threadIdx.x];
    __syncthreads();
    const unsigned C = (unsigned)(q.nslice + 2);
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
        const unsigned long long e = (unsigned long long)(head + 4 * v);
        long long cellw = (long long)(e / C);
        int c = (int)(e % C);
        float o[4];
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = bevp_value(pts, offsets, ws, key[j], cellw, c, hw, q, s_tab);
            any |= (key[j] | __float_as_uint(o[j])) != 0u;           // (a key whose value is 0.0f -- z == height_lo -- is still replaced)
            if (++c == (int)C) { c = 0; ++cellw; }
        }
        if (any) reinterpret_cast<float4 *>(body)[v] = make_float4(o[0], o[1], o[2], o[3]);
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < head + tail) {
        const long long e = (int)threadIdx.x < head ? (long long)threadIdx.x : 4 * nvec + threadIdx.x;      // (head + 4 nvec + (t - head))
        const unsigned key = reinterpret_cast<const unsigned *>(top)[e];
        const float o = bevp_value(pts, offsets, ws, key, (long long)((unsigned long long)e / C), (int)((unsigned long long)e % C), hw, q, s_tab);
        if ((key | __float_as_uint(o)) != 0u) top[e] = o;
    }
}

// ranges8_host (NULL = the call MV3D makes) -> parameters; false for ranges mv3d_point_cloud_2_top_shape refuses
static bool bevp_params(const double *r, BevParams &q)
{
    if (r) return bev_params8(r, q);
    bev_params_mv3d(q);
    return true;
}

extern "C" int mv3d_point_cloud_2_top_paper_shape(double res, double zres, double side_lo, double side_hi, double fwd_lo, double fwd_hi,
                                                  double height_lo, double height_hi, int *dims)
{
    BevParams q;
    if (!dims || !bev_params(res, zres, side_lo, side_hi, fwd_lo, fwd_hi, height_lo, height_hi, q)) return MV3D_ERR_INVALID_ARG;
    dims[0] = q.Hd; dims[1] = q.Wd; dims[2] = q.nslice + 2;
    return MV3D_OK;
}

extern "C" size_t mv3d_point_cloud_2_top_paper_workspace(int num_frames, const double *ranges8_host)
{
    BevParams q;
    if (num_frames < 1 || num_frames > MV3D_FV_MAX_FRAMES || !bevp_params(ranges8_host, q)) return 0;
    return (size_t)num_frames * (size_t)q.Hd * (size_t)q.Wd * sizeof(unsigned long long);
}

extern "C" int mv3d_point_cloud_2_top_paper_batch(const float *points_dev, const int32_t *offsets_dev, int num_frames, int total_points,
                                                  const double *ranges8_host, float *top_dev, void *workspace_dev, int32_t *status_dev,
                                                  void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (num_frames < 0 || num_frames > MV3D_FV_MAX_FRAMES || total_points < 0) return MV3D_ERR_INVALID_ARG;
    if (num_frames == 0) return MV3D_OK;
    BevParams q;
    if (!bevp_params(ranges8_host, q) || (ranges8_host && !status_dev)) return MV3D_ERR_INVALID_ARG;
    if (!ranges8_host) status_dev = nullptr;                     // (no cell of MV3D's map can fall outside)
    if ((!offsets_dev && num_frames != 1) || !top_dev || !workspace_dev || (total_points > 0 && !points_dev)) return MV3D_ERR_INVALID_ARG;
    if (((uintptr_t)points_dev & 15) != 0 || ((uintptr_t)top_dev & 3) != 0 || ((uintptr_t)offsets_dev & 3) != 0 ||
        ((uintptr_t)status_dev & 3) != 0 || ((uintptr_t)workspace_dev & 15) != 0)
        return MV3D_ERR_INVALID_ARG;
    const long long hw = (long long)q.Hd * q.Wd, n = hw * (q.nslice + 2), total = n * num_frames, nws = hw * num_frames;
    int head, tail;
    long long nvec;
    bev_flat_split(top_dev, total, head, nvec, tail);
    const long long top_groups = nvec / 1024 + 1, ws_groups = (nws / 2) / 1024 + 1, resolve_groups = nvec / 512 + 1;
    if (resolve_groups > 0x7FFFFFFFll || top_groups + ws_groups > 0x7FFFFFFFll) return MV3D_ERR_INVALID_ARG;
    unsigned long long *ws = reinterpret_cast<unsigned long long *>(workspace_dev);
    hipLaunchKernelGGL(bevp_clear_kernel, dim3((unsigned)(top_groups + ws_groups)), dim3(256), 0, s, top_dev, head, nvec, tail,
                       (unsigned)top_groups, ws, nws, status_dev);
    if (total_points > 0) {
        BevDensity dens;
        mv3d_bev_density_table(dens.t);
        hipLaunchKernelGGL(bevp_scatter_kernel, dim3(((unsigned)total_points + 255u) / 256u), dim3(256), 0, s, points_dev, offsets_dev,
                           num_frames, total_points, reinterpret_cast<unsigned *>(top_dev), ws, n, hw, q, status_dev);
        hipLaunchKernelGGL(bevp_resolve_kernel, dim3((unsigned)resolve_groups), dim3(256), 0, s, points_dev, offsets_dev, ws, top_dev, head,
                           nvec, tail, hw, q, dens);
    }
    return mv3d_launch_status();
}
