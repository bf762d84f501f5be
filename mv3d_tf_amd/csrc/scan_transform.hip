// Scan augmentation: a similarity transform A = [s R(theta) | t] per frame on `num_frames` Velodyne clouds laid back
// to back, in front of the crop (scan_crop.hip) and the rasterisers (bev_raster.hip, bev_paper.hip, front_view_raster.hip), which take
// the result as they take any other (points, offsets) batch.  PARITY UNPINNED: the reference trains from stored maps and has no such
// code; tests/scan_augment_restatement.py states the rule.
//   a row     [x, y, z, r] of frame b with finite x, y, z becomes, with A = xform[b] (3x4 f64, row-major),
//                 c'_i = (float)fma(A[i][3], 1, fma(A[i][2], z, fma(A[i][1], y, fma(A[i][0], x, 0))))      in f64, i = 0, 1, 2
//             -- scan_image_point's chain (geometry.h) on an f64 matrix -- and r is copied bit for bit.  A row with a non-finite
//             coordinate and a row that no frame owns (frame_rows.h) are copied bit for bit, all 16 bytes.
//   launch    one, one thread per row, 256 rows a workgroup; one 16-byte load and one 16-byte store per row, so out == in works: no
//             thread reads a row another one writes.
//   matrices  a workgroup stages the matrices of the frame of its first row and the SCAN_XF_STAGED - 1 frames behind it in LDS
//             (768 bytes; all MV3D_FV_MAX_FRAMES of them would be 96 KB and cost the occupancy); 256 consecutive rows touch more
//             frames than that only under frames of a few rows, and such a row reads its twelve values from the table.
//   bounds    rows p < P only; the frame comes from frame_of_row, which answers "none" or a frame in [0, nf) whatever offsets_dev
//             holds, and indexes xform alone; the matrix' values enter arithmetic only, never an address.  So nothing in offsets_dev
//             or xform_dev can make the call read or write out of bounds.
// HBM-bound by construction: 16 P bytes read, 16 P written, 12 f64 fmas a row.
#include "common.h"
#include "frame_rows.h"

#pragma clang fp contract(off)       // (the build's -ffp-contract=off, restated where it matters: only the written fmas are fused)

#define SCAN_XF_STAGED 8             // frames whose matrix a workgroup stages in LDS: the frame of its first row and the 7 behind it

__device__ __forceinline__ float4 scan_transform_row(float4 v, const double *A)
{
    const unsigned inf = 0x7f800000u;
    if ((__float_as_uint(v.x) & inf) == inf || (__float_as_uint(v.y) & inf) == inf || (__float_as_uint(v.z) & inf) == inf) return v;
    const double cx = (double)v.x, cy = (double)v.y, cz = (double)v.z;
    float c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double acc = 0.0;
        acc = fma(A[i * 4 + 0], cx, acc);
        acc = fma(A[i * 4 + 1], cy, acc);
        acc = fma(A[i * 4 + 2], cz, acc);
        acc = fma(A[i * 4 + 3], 1.0, acc);
        c[i] = (float)acc;
    }
    return make_float4(c[0], c[1], c[2], v.w);
}

// pts and out may be one buffer: neither is __restrict__
__global__ __launch_bounds__(256) void scan_transform_kernel(const float *pts, const int *__restrict__ offsets, int nf, int P,
                                                             const double *__restrict__ xform, float *out)
{
    __shared__ int s_off[MV3D_FV_MAX_FRAMES + 1];
    __shared__ double s_A[SCAN_XF_STAGED][12];
    frame_rows_stage(s_off, offsets, nf, P);
    const unsigned first = blockIdx.x * 256u;
    int f0;
    frame_of_row(s_off, nf, first, f0);                                  // (a frame in [0, nf) whether or not it owns the row)
    if (threadIdx.x < SCAN_XF_STAGED * 12) {
        const int j = threadIdx.x / 12, e = threadIdx.x % 12;
        if (f0 + j < nf) s_A[j][e] = xform[12 * (size_t)(f0 + j) + e];
    }
    __syncthreads();
    const unsigned p = first + threadIdx.x;
    if (p >= (unsigned)P) return;
    float4 v = reinterpret_cast<const float4 *>(pts)[p];
    int f;
    if (frame_of_row(s_off, nf, p, f)) {
        const unsigned j = (unsigned)(f - f0);
        if (j < SCAN_XF_STAGED) {
            v = scan_transform_row(v, s_A[j]);
        } else {                                                         // more than 8 frames in 256 rows: the matrix from the table
            double A[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) A[e] = xform[12 * (size_t)f + e];
            v = scan_transform_row(v, A);
        }
    }
    reinterpret_cast<float4 *>(out)[p] = v;
}

extern "C" int mv3d_scan_transform(const float *points_dev, const int32_t *offsets_dev, int num_frames, int total_points,
                                   const double *xform_dev, float *points_out_dev, void *stream)
{
    if (num_frames < 0 || num_frames > MV3D_FV_MAX_FRAMES || total_points < 0) return MV3D_ERR_INVALID_ARG;
    if (num_frames == 0) return MV3D_OK;
    if ((!offsets_dev && num_frames != 1) || !xform_dev) return MV3D_ERR_INVALID_ARG;
    if (total_points > 0 && (!points_dev || !points_out_dev)) return MV3D_ERR_INVALID_ARG;
    if (((uintptr_t)points_dev & 15) != 0 || ((uintptr_t)points_out_dev & 15) != 0 || ((uintptr_t)offsets_dev & 3) != 0 ||
        ((uintptr_t)xform_dev & 7) != 0)
        return MV3D_ERR_INVALID_ARG;
    const uintptr_t in = (uintptr_t)points_dev, out = (uintptr_t)points_out_dev, bytes = (uintptr_t)total_points * 16;
    if (in != out && in < out + bytes && out < in + bytes) return MV3D_ERR_INVALID_ARG;    // (in place, or no byte in common)
    if (total_points == 0) return MV3D_OK;
    hipLaunchKernelGGL(scan_transform_kernel, dim3((unsigned)(((long long)total_points + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       points_dev, offsets_dev, num_frames, total_points, xform_dev, points_out_dev);
    return mv3d_launch_status();
}
