// The test-time tail of box_detect (lib/fast_rcnn/test_mv.py:240-261; SURVEY §8(f) "next" rows, rank 2): lidar_3d_to_corners,
// bbox_transform_inv_cnr (lib/fast_rcnn/bbox_transform.py:157-176), corners_to_bv (lib/utils/transform.py:342-366)
#include <math.h>
#include "geometry.h"

// numpy npy_divmodf -> floor_divide in f32: corners_to_bv runs _lidar_to_bv_coord on f32 arrays, so
// RES = 0.1 becomes the f32 0.1 and the whole floor-division is single precision.
__device__ __forceinline__ float np_floor_dividef(float a, float b)
{
    if (b == 0.0f) return a / b;
    float mod = fmodf(a, b);
    float div = (a - mod) / b;
    if (mod != 0.0f) {
        if ((b < 0) != (mod < 0)) { mod += b; div -= 1.0f; }
    }
    float fd;
    if (div != 0.0f) {
        fd = floorf(div);
        if (div - fd > 0.5f) fd += 1.0f;
    } else {
        fd = copysignf(0.0f, a / b);
    }
    return fd;
}

__device__ __forceinline__ void corners_to_bv_one(const float *c, float *out)
{
    float xmin = c[0], xmax = c[0], ymin = c[8], ymax = c[8];
    bool nx = c[0] != c[0], ny = c[8] != c[8];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        if (c[k] < xmin) xmin = c[k];
        if (c[k] > xmax) xmax = c[k];
        if (c[8 + k] < ymin) ymin = c[8 + k];
        if (c[8 + k] > ymax) ymax = c[8 + k];
        nx |= c[k] != c[k]; ny |= c[8 + k] != c[8 + k];
    }
    if (nx) xmin = xmax = NAN;
    if (ny) ymin = ymax = NAN;
    const float res = (float)BV_RES;
    out[0] = (float)BV_YN - np_floor_dividef(ymax - (float)TOP_Y_MIN_D, res);     // transform.py:17-18, 352-355
    out[1] = (float)BV_XN - np_floor_dividef(xmax - (float)TOP_X_MIN_D, res);
    out[2] = (float)BV_YN - np_floor_dividef(ymin - (float)TOP_Y_MIN_D, res);
    out[3] = (float)BV_XN - np_floor_dividef(xmin - (float)TOP_X_MIN_D, res);
}

__global__ __launch_bounds__(128) void box_tail_kernel(const float *__restrict__ rois_3d, const float *__restrict__ deltas,
                                                       int R, int nc, float *corners, float *pred_cnr_r, float *bv, float *bv_r)
{
    const int i = blockIdx.x * 128 + threadIdx.x;
    if (i >= R) return;
    const float *P = rois_3d + 7 * (long long)i + 1;            // rois[2][:, 1:7] (test_mv.py:240)
    const float hl = P[3] / 2.0f, hw = P[4] / 2.0f, hh = P[5] / 2.0f;
    float c[24];
#pragma unroll
    for (int k = 0; k < 8; ++k) {                                // transform.py:296-313
        c[k] = ((k & 2) ? -hl : hl) + P[0];
        c[8 + k] = (((k + 1) & 2) ? -hw : hw) + P[1];
        c[16 + k] = ((k & 4) ? hh : -hh) + P[2];
    }
    for (int j = 0; j < 24; ++j) corners[24 * (long long)i + j] = c[j];
    // bbox_transform.py:162-176: diag = ||p0 - p6|| in f32 (sqrt((d0^2 + d1^2) + d2^2)), deltas * diag + boxes
    const float d0 = c[0] - c[6], d1 = c[8] - c[14], d2 = c[16] - c[22];
    float ss = __fmul_rn(d0, d0);
    ss = __fadd_rn(ss, __fmul_rn(d1, d1));
    ss = __fadd_rn(ss, __fmul_rn(d2, d2));
    const float diag = sqrtf(ss);
    for (int k = 0; k < nc; ++k) {
        float pr[24];
        const float *dl = deltas + ((long long)i * nc + k) * 24;
#pragma unroll
        for (int j = 0; j < 24; ++j) pr[j] = __fadd_rn(__fmul_rn(dl[j], diag), c[j]);
        for (int j = 0; j < 24; ++j) pred_cnr_r[((long long)i * nc + k) * 24 + j] = pr[j];
        corners_to_bv_one(c, bv + ((long long)i * nc + k) * 4);                   // hstack((cnr, cnr)) (:250)
        corners_to_bv_one(pr, bv_r + ((long long)i * nc + k) * 4);
    }
}

extern "C" int mv3d_box_detect_tail(const float *rois_3d_dev, const float *bbox_pred_dev, int num_rois, int num_classes,
                                    float *corners_dev, float *pred_cnr_r_dev, float *pred_bv_dev, float *pred_bv_r_dev,
                                    void *stream)
{
    if (num_rois < 0 || num_classes <= 0) return MV3D_ERR_INVALID_ARG;
    if (num_rois == 0) return MV3D_OK;
    if (!rois_3d_dev || !bbox_pred_dev || !corners_dev || !pred_cnr_r_dev || !pred_bv_dev || !pred_bv_r_dev)
        return MV3D_ERR_INVALID_ARG;
    hipLaunchKernelGGL(box_tail_kernel, dim3((num_rois + 127) / 128), dim3(128), 0, (hipStream_t)stream, rois_3d_dev,
                       bbox_pred_dev, num_rois, num_classes, corners_dev, pred_cnr_r_dev, pred_bv_dev, pred_bv_r_dev);
    return mv3d_launch_status();
}
