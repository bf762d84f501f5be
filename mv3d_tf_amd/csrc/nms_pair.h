// The IoU predicate of the greedy NMS, shared by every kernel that suppresses boxes (nms.hip, detect_post.hip).
#pragma once
#include "common.h"

// lib/nms/cpu_nms.pyx:55-65 for one (kept box i, later box j) pair.  f32, separate IEEE
// ops.  Cython emits ((xx2 - xx1) + 1.0) with a double literal and narrows to f32; for
// f32 operands that equals the f32 add (the f64 sum is exact or rounds identically), so
// the f32 form below is bit-identical.  `tf` is ceil_f32(thresh): (double)ovr >= thresh
// <=> ovr >= tf.  The CUDA rule `ovr > thresh` (nms_kernel.cu:71) is served by the same
// compare with tf = nextafter(thresh, +inf).
__device__ __forceinline__ bool pair_suppresses(float ix1, float iy1, float ix2, float iy2, float iarea,
                                                float jx1, float jy1, float jx2, float jy2, float jarea,
                                                float tf, bool &zero_den)
{
    const float xx1 = cy_max(ix1, jx1);
    const float yy1 = cy_max(iy1, jy1);
    const float xx2 = cy_min(ix2, jx2);
    const float yy2 = cy_min(iy2, jy2);
    const float w = cy_max(0.0f, (xx2 - xx1) + 1.0f);
    const float h = cy_max(0.0f, (yy2 - yy1) + 1.0f);
    const float inter = w * h;
    const float den = (iarea + jarea) - inter;
    zero_den = (den == 0.0f);
    const float ovr = inter / den;
    return ovr >= tf;
}
