// The BEV rasterisers' one statement of "which cell and which height slices does a row fall into": the parameters (host
// arithmetic) and the two device functions that bevb_scatter_kernel (bev_raster.hip, the reference's encoding) and
// bevp_scatter_kernel (bev_paper.hip, the MV3D paper's) both call.  point_cloud_2_top (lib/utils/read_lidar.py:10-115 ==
// tools/read_lidar.py:10-115) is what is restated; the dtypes numpy gives every step (f32 range tests against Python floats, f64
// slice tests against np.arange's values, which are h0, h0 + zres, h0 + i * ((h0 + zres) - h0), ...) are spelled out in
// oracle/mv3d_oracle.c:mv3d_ref_point_cloud_2_top_ranges.
#pragma once
#include "common.h"

// The rasterisers' parameters; the kernels take the struct by value.  Cd = z_max + 1 is the REFERENCE encoding's channel count;
// the paper's is nslice + 2 (bev_paper.hip).
struct BevParams {
    float fwd0f, fwd1f, ylo, yhi, resf, h0f;
    double h0, next, delta, zres;
    int xoff, yoff, Hd, Wd, Cd, nslice, zmax;
};

static bool bev_params(double res, double zres, double side0, double side1, double fwd0, double fwd1, double h0, double h1, BevParams &q)
{
    if (!(res > 0.0) || !(zres > 0.0) || !(side1 > side0) || !(fwd1 > fwd0) || !(h1 >= h0)) return false;
    const double nx = (side1 - side0) / res, ny = (fwd1 - fwd0) / res, nz = (h1 - h0) / zres;
    if (!(nx < 32768.0) || !(ny < 32768.0) || !(nz < 31.0)) return false;       // (the key of the last channel holds 5 bits of slice)
    const int x_max = (int)nx, y_max = (int)ny, z_max = (int)nz;                 // read_lidar.py:49-51
    q.Wd = x_max + 1; q.Hd = y_max + 1; q.Cd = z_max + 1; q.zmax = z_max;
    q.xoff = (int)floor(side0 / res); q.yoff = (int)floor(fwd1 / res);
    q.nslice = (int)ceil(nz);
    q.h0 = h0; q.next = h0 + zres; q.delta = q.next - h0; q.zres = zres;
    q.fwd0f = (float)fwd0; q.fwd1f = (float)fwd1; q.ylo = (float)(-side1); q.yhi = (float)(-side0); q.resf = (float)res; q.h0f = (float)h0;
    return true;
}

static bool bev_params8(const double *r, BevParams &q) { return bev_params(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], q); }

// tools/read_lidar.py:121-133 -> 601 x 601 cells, 8 slices; no cell can fall outside
static void bev_params_mv3d(BevParams &q) { bev_params(0.1, 0.3, -30.0, 30.0, 0.0, 60.0, -2.0, 0.4, q); }

#define BEVB_MAX_INDEX ((1u << 27) - 2u)       // largest index within a frame: index + 1 stays below 2^27, as mv3d_point_cloud_2_top requires

// A run of `total` f32 elements at a 4-byte aligned `top`, as clear and resolve walk it: `head` scalar elements up to the first
// 16-byte boundary, `nvec` 16-byte vectors, `tail` scalar elements (head, tail <= 3).
static void bev_flat_split(const float *top, long long total, int &head, long long &nvec, int &tail)
{
    const long long to_boundary = (long long)(((16u - (unsigned)((uintptr_t)top & 15u)) & 15u) / 4u);      // 0 .. 3 elements
    head = (int)(to_boundary < total ? to_boundary : total);
    nvec = (total - head) / 4;
    tail = (int)(total - head - 4 * nvec);
}

// The cell of row v = [x, y, z, r].  false: the row fails a range test and is dropped.  true: `pixel` = yi * W + xi, and `out`
// says that (yi, xi) lies outside the map after numpy's wrap of negative indices (its IndexError); `pixel` is then no answer.
__device__ __forceinline__ bool bev_cell_of(const float4 &v, const BevParams &q, long long &pixel, bool &out)
{
    if (!(v.x > q.fwd0f && v.x < q.fwd1f)) return false;        // f_filt (read_lidar.py:58-59): f32 against the f32-rounded bounds
    if (!(v.y > q.ylo && v.y < q.yhi)) return false;            // s_filt (:60-61)
    int xi = (int)(-v.y / q.resf), yi = (int)(-v.x / q.resf);   // f32 divide, astype(int32) truncates (:96-97)
    xi -= q.xoff;                                                // int(np.floor(side_range[0] / res)) (:102)
    yi += q.yoff;                                                // int(np.floor(fwd_range[1] / res))  (:103)
    if (xi < 0) xi += q.Wd;                                      // numpy: a negative index counts from the end ...
    if (yi < 0) yi += q.Hd;
    out = xi < 0 || xi >= q.Wd || yi < 0 || yi >= q.Hd;          // ... anything else outside the map is its IndexError
    pixel = (long long)yi * q.Wd + xi;
    return true;
}

// is z inside height slice i < nslice?  np.arange(h0, h1, zres) (:80), compared in f64 (:82-83).  NaN and +-inf are in no slice.
__device__ __forceinline__ bool bev_in_slice(double z, int i, const BevParams &q)
{
    const double height = i == 0 ? q.h0 : (i == 1 ? q.next : q.h0 + (double)i * q.delta);
    return z >= height && z < height + q.zres;
}
