// Rounded ROI geometry shared by the RoiPool kernels (roi_pool.hip, roi_grad_tiles.hip).
#pragma once
#include "common.h"

struct RoiGeom { int rsw, rsh, rew, reh; };

// roi_pooling_op.cc:139-143: round() (half away from zero) of the f32 product
__device__ __forceinline__ RoiGeom roi_geom(const float *roi, float scale)
{
    RoiGeom g;
    g.rsw = (int)roundf(__fmul_rn(roi[1], scale));
    g.rsh = (int)roundf(__fmul_rn(roi[2], scale));
    g.rew = (int)roundf(__fmul_rn(roi[3], scale));
    g.reh = (int)roundf(__fmul_rn(roi[4], scale));
    return g;
}

// The view of a multi-view launch that workgroup `blk` belongs to: the last of the n views whose first workgroup, first(j), is <= blk
// (view 0 starts at workgroup 0).  `first` reads wherever the launch's pack keeps the first workgroups.
template <typename First>
__device__ __forceinline__ int roi_view_of(const unsigned blk, const int n, const First &first)
{
    int k = 0;
#pragma unroll
    for (int j = 1; j < MV3D_MAX_ROI_VIEWS; ++j)
        if (j < n && blk >= first(j)) k = j;
    return k;
}
