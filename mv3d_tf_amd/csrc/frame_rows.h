// Which frame owns a row of `num_frames` clouds laid back to back: the one statement of the rule for every scatter kernel that takes
// (points, offsets) -- fv_scatter_kernel (front_view_raster.hip), bevb_scatter_kernel (bev_raster.hip) and bevp_scatter_kernel (bev_paper.hip).
// Frame b owns rows offsets[b] .. offsets[b + 1].  The frame of row p is the LAST b with offsets[b] <= p (a binary search over the
// offsets staged in LDS; equal neighbours = an empty frame, skipped by that rule).  A row outside [offsets[b], offsets[b + 1]) -- in
// front of offsets[0], behind offsets[num_frames], or anything under offsets that do not ascend -- belongs to NO frame and is skipped.
// Bounds: the answer is "none" or a frame in [0, nf) with offsets[frame] <= p < offsets[frame + 1], so whatever offsets_dev holds a
// caller that has tested p < P stays below P in the points, inside frame `frame` of its keys, and 0 <= p - offsets[frame] (DESIGN.md
// §3.21, §3.22 rest on this).
#pragma once
#include "common.h"

// Stage offsets[0 .. nf] in s_off (MV3D_FV_MAX_FRAMES + 1 ints of LDS); every thread of the 256-wide workgroup calls it, and none may
// have left before.
__device__ __forceinline__ void frame_rows_stage(int *s_off, const int *offsets, int nf, int P)
{
    for (int i = threadIdx.x; i <= nf; i += 256) s_off[i] = offsets ? offsets[i] : i * P;      // (no offsets: ONE frame of P rows)
    __syncthreads();
}

// frame = the frame that owns row p; false when none does (frame is then no answer)
__device__ __forceinline__ bool frame_of_row(const int *s_off, int nf, unsigned p, int &frame)
{
    int lo = 0, hi = nf - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_off[mid] <= (int)p) lo = mid; else hi = mid - 1;
    }
    frame = lo;
    return s_off[lo] <= (int)p && (int)p < s_off[lo + 1];
}
