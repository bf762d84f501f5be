// Rounded ROI geometry shared by the RoiPool kernels (roi_pool.hip, roi_grad_tiles.hip): the reference's rounding, bin and pixel rules
// (roi_pooling_op.cc:139-162, :392-431), each stated once.  Operand order, __fmul_rn and the f32 divides are the reference's: bits count.
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

// :146-147: a ROI's extent along one axis, forced to at least 1; an axis' bin size is (float)roi_extent / (float)P (:148-151)
__device__ __forceinline__ int roi_extent(const int rs, const int re) { return max(re - rs + 1, 1); }

struct RoiSpan { int s, e; };        // [s, e)

// The FORWARD rule for one axis (:153-162): the map pixels of pooled index p, [floor(p * bin), ceil((p + 1) * bin)) offset by the rounded
// ROI start and clamped to the map [0, limit].  p0, p1: the float forms of p and p + 1 (a caller may hoist them).
__device__ __forceinline__ RoiSpan roi_bin_span(const float p0, const float p1, const float bin, const int start, const int limit)
{
    return {min(max((int)floorf(__fmul_rn(p0, bin)) + start, 0), limit), min(max((int)ceilf(__fmul_rn(p1, bin)) + start, 0), limit)};
}

// The BACKWARD rule for one axis (:423-431, identical to the CUDA form roi_pooling_op_gpu.cu.cc:169-172): the pooled indices that may
// hold map pixel x, [floor((x - start) / bin), ceil((x - start + 1) / bin)) clamped to [0, P].
__device__ __forceinline__ RoiSpan roi_pixel_bins(const int x, const int start, const float bin, const int P)
{
    return {min(max((int)floorf((float)(x - start) / bin), 0), P), min(max((int)ceilf((float)(x - start + 1) / bin), 0), P)};
}

// The forward rectangle of bin (ph, pw) of the ROI row rr[5] (:139-162), 32 bytes (one wide LDS store).  base: the ROI's frame, < 0
// when nothing is pooled (an empty rectangle or a batch index outside [0, B)): the output is 0 / -1 then.
struct BinGeom { int hs, he, ws, we; int base; int pad0, pad1, pad2; };
__device__ __forceinline__ BinGeom roi_bin_rect(const float rr[5], const int ph, const int pw, const float scale, const int B, const int H, const int W,
                                                const int PH, const int PW)
{
    const int bi = (int)rr[0];
    const RoiGeom q = roi_geom(rr, scale);
    const float bh = (float)roi_extent(q.rsh, q.reh) / (float)PH, bw = (float)roi_extent(q.rsw, q.rew) / (float)PW;
    const RoiSpan h = roi_bin_span((float)ph, (float)(ph + 1), bh, q.rsh, H), w = roi_bin_span((float)pw, (float)(pw + 1), bw, q.rsw, W);
    const bool empty = (h.e <= h.s) || (w.e <= w.s) || bi < 0 || bi >= B;
    return {h.s, h.e, w.s, w.e, empty ? -1 : bi, 0, 0, 0};
}

// The pair's compact argmax codes (roi_pool.hip, COMPACT) are scan positions inside the bin's rectangle: a rectangle of more than 255
// pixels takes 16-bit codes in the escape plane, every other bin one byte.  THE contract between the pair's forward, its gradient
// and the decode: all three ask here.  rows, cols: of a non-empty rectangle.
__device__ __forceinline__ bool roi_rect_wide(const int rows, const int cols) { return rows * cols > 255; }
__device__ __forceinline__ bool roi_bin_wide(const BinGeom &g) { return g.base >= 0 && roi_rect_wide(g.he - g.hs, g.we - g.ws); }

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
