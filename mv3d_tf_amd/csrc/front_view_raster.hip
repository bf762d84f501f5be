// Front-view rasteriser: Velodyne points -> the 64 x 512 x 3 cylindrical map [height, distance, intensity] that the third
// trunk reads as `lidar_fv_data` (MV3D paper, Chen et al., CVPR 2017, §3.1), for a batch of frames behind three launches.
//
// PARITY UNPINNED BY CONSTRUCTION, like front_view.hip: the reference has no front view (lib/networks/network.py:293-315 is a
// TODO).  The definition is this repository's, written so that a point lands on the pixel rois_3d_to_fv
// computes for its position -- both go through fv_point of front_view.h:
//   pixel     (col, row) = fv_point((double)x, (double)y, (double)z)
//   dropped   x, y or z not finite; x == 0 && y == 0 (the zero rows of padded clouds); col outside [0, 512) or row outside
//             [0, 64) -- nothing is clipped into the window; the reflectance takes no part
//   distance  d = (float)sqrt(fma(z, z, fma(x, x, y * y))), f64 rounded once; every kept point has d > 0
//   winner    smallest d (a depth buffer: the nearest return occludes), among equal d the LAST point in point order
//   values    [z, d, reflectance] of the winner, z and reflectance copied bit for bit; an empty pixel is [0, 0, 0]
// Every step is an IEEE basic operation, so tests/front_view_raster_restatement.py agrees bit for bit.
//
// The winner is one 64-bit atomicMin per point on  bits(d) << 32 | (0xFFFFFFFF - point index) : d > 0, so its bit pattern
// orders like its value, and the complemented index makes the later point the smaller key.  The minimum of a set does not
// depend on the order of arrival, so the map does not depend on scheduling.  Keys live in the caller's workspace (one per
// pixel and frame, 256 KB a frame); 0xFFFF... (a NaN distance, which no point has) marks an empty pixel.
#include "front_view.h"
#include "frame_rows.h"

#define FV_PIXELS (FV_H * FV_W)
#define FV_EMPTY 0xFFFFFFFFFFFFFFFFull

// a workgroup sets 2048 keys = 16 KB contiguous, four 16-byte stores per thread (the key count is a multiple of 2048)
__global__ __launch_bounds__(256) void fv_clear_kernel(unsigned long long *keys)
{
    ulonglong2 *k2 = reinterpret_cast<ulonglong2 *>(keys) + (size_t)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
    for (int u = 0; u < 4; ++u) k2[u * 256] = make_ulonglong2(FV_EMPTY, FV_EMPTY);
}

// One thread per point of the concatenated clouds; a point that belongs to no frame (frame_rows.h) is skipped: whatever the offsets
// hold, p stays below P and the key index inside the workspace.
__global__ __launch_bounds__(256) void fv_scatter_kernel(const float *__restrict__ pts, const int *__restrict__ offsets, int nf, int P,
                                                         unsigned long long *keys)
{
    __shared__ int s_off[MV3D_FV_MAX_FRAMES + 1];
    frame_rows_stage(s_off, offsets, nf, P);
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (unsigned)P) return;
    const float4 v = reinterpret_cast<const float4 *>(pts)[p];
    int lo;
    if (!frame_of_row(s_off, nf, p, lo)) return;
    if (!(fabsf(v.x) <= 3.402823466e+38f && fabsf(v.y) <= 3.402823466e+38f && fabsf(v.z) <= 3.402823466e+38f)) return;   // NaN, +-inf
    if (v.x == 0.0f && v.y == 0.0f) return;
    const double x = (double)v.x, y = (double)v.y, z = (double)v.z;
    double col, row;
    fv_point(x, y, z, col, row);
    if (!(col >= 0.0 && col < (double)FV_W && row >= 0.0 && row < (double)FV_H)) return;
    const float d = (float)__dsqrt_rn(fma(z, z, fma(x, x, y * y)));
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(0xFFFFFFFFu - p);
    unsigned long long *cell = keys + (size_t)lo * FV_PIXELS + (int)row * FV_W + (int)col;
    // (every kept point issues its atomic, which returns nothing: DESIGN.md §3.21 on same-pixel contention)
    atomicMin(cell, key);
}

// Four neighbouring pixels of a row per thread: two 16-byte key loads, the winners' [z, reflectance] as 8-byte loads, three 16-byte
// stores (4 pixels x 3 channels = 48 contiguous bytes).
__global__ __launch_bounds__(256) void fv_resolve_kernel(const float *__restrict__ pts, const unsigned long long *__restrict__ keys,
                                                         float *__restrict__ fv)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;                 // quad index; the grid covers the quads exactly
    const ulonglong2 k01 = reinterpret_cast<const ulonglong2 *>(keys)[2 * q], k23 = reinterpret_cast<const ulonglong2 *>(keys)[2 * q + 1];
    const unsigned long long k[4] = {k01.x, k01.y, k23.x, k23.y};
    float o[12];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        o[3 * u] = o[3 * u + 1] = o[3 * u + 2] = 0.0f;
        if (k[u] != FV_EMPTY) {
            const unsigned p = 0xFFFFFFFFu - (unsigned)k[u];
            const float2 zr = *reinterpret_cast<const float2 *>(pts + 4 * (size_t)p + 2);
            o[3 * u] = zr.x; o[3 * u + 1] = __uint_as_float((unsigned)(k[u] >> 32)); o[3 * u + 2] = zr.y;
        }
    }
    float4 *out = reinterpret_cast<float4 *>(fv) + 3 * q;
    out[0] = make_float4(o[0], o[1], o[2], o[3]);
    out[1] = make_float4(o[4], o[5], o[6], o[7]);
    out[2] = make_float4(o[8], o[9], o[10], o[11]);
}

extern "C" size_t mv3d_point_cloud_2_front_workspace(int num_frames)
{
    if (num_frames <= 0 || num_frames > MV3D_FV_MAX_FRAMES) return 0;
    return (size_t)num_frames * FV_PIXELS * sizeof(unsigned long long);
}

extern "C" int mv3d_point_cloud_2_front(const float *points_dev, const int32_t *offsets_dev, int num_frames, int total_points,
                                        float *fv_dev, void *workspace_dev, void *stream)
{
    if (num_frames < 0 || num_frames > MV3D_FV_MAX_FRAMES || total_points < 0) return MV3D_ERR_INVALID_ARG;
    if (num_frames == 0) return MV3D_OK;
    if ((!offsets_dev && num_frames != 1) || !fv_dev || !workspace_dev || (total_points > 0 && !points_dev)) return MV3D_ERR_INVALID_ARG;
    if (((uintptr_t)points_dev & 15) != 0 || ((uintptr_t)fv_dev & 15) != 0 || ((uintptr_t)workspace_dev & 15) != 0 ||
        ((uintptr_t)offsets_dev & 3) != 0)
        return MV3D_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(workspace_dev);
    const unsigned quads = (unsigned)num_frames * (FV_PIXELS / 4);
    hipLaunchKernelGGL(fv_clear_kernel, dim3((unsigned)num_frames * (FV_PIXELS / 2048)), dim3(256), 0, s, keys);
    if (total_points > 0)
        hipLaunchKernelGGL(fv_scatter_kernel, dim3(((unsigned)total_points + 255u) / 256u), dim3(256), 0, s, points_dev, offsets_dev,
                           num_frames, total_points, keys);
    hipLaunchKernelGGL(fv_resolve_kernel, dim3(quads / 256), dim3(256), 0, s, points_dev, keys, fv_dev);   // (no point: every key is empty)
    return mv3d_launch_status();
}
