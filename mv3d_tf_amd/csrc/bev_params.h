// The BEV rasteriser's parameters (point_cloud_2_top, lib/utils/read_lidar.py:10-115), host arithmetic shared by the single-cloud
// kernels of next_rows.hip and the batched ones of bev_raster_batch.hip: both take the struct by value.
// The dtypes numpy gives every step (f32 range tests against Python floats, f64 slice tests against np.arange's values, which are
// h0, h0 + zres, h0 + i * ((h0 + zres) - h0), ...) are spelled out in oracle/mv3d_oracle.c:mv3d_ref_point_cloud_2_top_ranges.
#pragma once
#include <math.h>

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
