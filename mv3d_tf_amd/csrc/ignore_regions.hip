// Ignore regions in training (not in the reference): sampled BACKGROUND anchors and sampled background ROIs
// that lie on an ignore region (a Van, a DontCare box, ...) get label -1, which both losses skip.  The relabelling runs after the
// target layers have drawn their samples, out of place, in ONE launch for both candidate kinds and all frames.
//
//   IoA(c, q)  = intersection over the CANDIDATE's area, f64, +1 pixel convention of bbox_overlap_f64:
//                iw = min(c2, q2) - max(c0, q0) + 1, ih likewise, both > 0 or the result is 0; iw * ih / ((c2 - c0 + 1)(c3 - c1 + 1));
//                0 when the candidate's area is not > 0; a NaN among the eight numbers gives 0.
//   relabel    label == 0 and (max_k IoA(c_bv, ignore_bv[b][k]) >= T or max_m IoA(c_img, ignore_img[b][m]) >= T)  ->  -1;
//                every other label passes through bit for bit.
//   anchors    c_bv = grid_anchor(n, W, stride) (not clipped), c_img = image_box(proj_matrix(calib[b]), anchor_to_lidar(c_bv)): the
//                statements of geometry.h the proposal decode uses; four int32, converted to f64.
//   ROIs       c_bv = rois_bv[r, 1:5], c_img = rois_img[r, 1:5], frame = rois_bv[r, 0].
//
// Launch shape: grid (batch, 2), 1024 threads.  Workgroup (b, 0) owns frame b's anchors, (b, 1) the ROI rows whose frame is b (rows
// whose frame column names no frame are written through by workgroup (0, 1)).  After subsampling almost every anchor label is -1: a
// thread reads its label first and writes it through unless it is 0; the few hundred labelled candidates are queued in LDS and then
// processed one per thread, so only they project a box and walk the lists.  A frame's ignore boxes are staged in LDS, IGN_STAGE boxes
// at a time.  The work is bound by the launch and two dependent passes, not by bandwidth.
#include "common.h"
#include "geometry.h"

#define IGN_THREADS 1024
#define IGN_STAGE 256                       // ignore boxes staged at a time: one float per thread
#define IGN_QUEUE 8192                      // queued candidates; a pass adds at most IGN_TILE
#define IGN_TILE (4 * IGN_THREADS)

struct IgnoreDev {
    const float *rpn_labels;    // (B, N)
    const int32_t *roi_labels;  // (S)
    const float *rois_bv;       // (S, 5)
    const float *rois_img;      // (S, 5)
    const float *calib;         // (B, 4, 12)
    const float *ign[2];        // packed (rows, 4): BEV, image
    const int32_t *off[2];      // (B + 1) each
    int rows[2];
    int B, N, S, W, stride;
    double T;
    float *rpn_out;
    int32_t *roi_out;
    int32_t *counts;            // (B, 2) or NULL
    int32_t *status;            // (B) or NULL
};

struct IgnCand {
    double bv[4], img[4];
    double area_bv, area_img;   // 0 where the candidate cannot be ignored on that side (area not > 0, or a NaN)
};

__device__ __forceinline__ double ign_area(const double c[4])
{
    if (c[0] != c[0] || c[1] != c[1] || c[2] != c[2] || c[3] != c[3]) return 0.0;
    const double a = (c[2] - c[0] + 1) * (c[3] - c[1] + 1);
    return a > 0 ? a : 0.0;
}

// IoA(c, q) >= T for a candidate with area > 0 and no NaN
__device__ __forceinline__ bool ign_hit(const double c[4], double area, float4 qf, double T)
{
    const double q0 = (double)qf.x, q1 = (double)qf.y, q2 = (double)qf.z, q3 = (double)qf.w;
    if (q0 != q0 || q1 != q1 || q2 != q2 || q3 != q3) return false;
    const double iw = fmin(c[2], q2) - fmax(c[0], q0) + 1;
    if (!(iw > 0)) return false;
    const double ih = fmin(c[3], q3) - fmax(c[1], q1) + 1;
    if (!(ih > 0)) return false;
    return iw * ih / area >= T;
}

// Every thread of the workgroup calls it (it synchronises); `live` threads test their candidate against rows [o0, o1) of `rows`.
__device__ __forceinline__ bool ign_walk(const float *__restrict__ rows, int o0, int o1, float *s_box, bool live, const double c[4],
                                         double area, double T)
{
    bool hit = false;
    for (int base = o0; base < o1; base += IGN_STAGE) {
        const int n = min(IGN_STAGE, o1 - base);
        __syncthreads();                                                     // the previous stage has been read
        if ((int)threadIdx.x < 4 * n) s_box[threadIdx.x] = rows[4 * (long long)base + threadIdx.x];
        __syncthreads();
        if (live && !hit)
            for (int k = 0; k < n; ++k)
                if (ign_hit(c, area, reinterpret_cast<const float4 *>(s_box)[k], T)) { hit = true; break; }
    }
    return hit;
}

__global__ __launch_bounds__(IGN_THREADS) void ignore_relabel_kernel(IgnoreDev d)
{
    __shared__ __attribute__((aligned(16))) float s_box[4 * IGN_STAGE];
    __shared__ int s_queue[IGN_QUEUE];
    __shared__ int s_n, s_red[IGN_THREADS / 64];
    __shared__ float s_M[12];
    const int b = blockIdx.x, kind = blockIdx.y, tid = threadIdx.x;
    const int total = kind == 0 ? d.N : d.S;

    // the frame's two row ranges; a frame whose offsets are out of order, out of the lists or too long is written through
    int o0[2], o1[2];
    bool ok = true;
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        o0[l] = d.off[l][b]; o1[l] = d.off[l][b + 1];
        ok = ok && o0[l] >= 0 && o0[l] <= o1[l] && o1[l] <= d.rows[l] && o1[l] - o0[l] <= TARGET_MAX_GT;
    }
    if (tid == 0) {
        s_n = 0;
        if (kind == 0) {
            proj_matrix(d.calib + 48 * (long long)b, s_M);
            if (d.status) d.status[b] = ok ? MV3D_OK : MV3D_ERR_INVALID_ARG;
        }
    }
    __syncthreads();

    int relabelled = 0;
    for (int base = 0; base < total; base += IGN_TILE) {
        // pass 1: labels through; this frame's background candidates into the queue
        for (int i = base + tid; i < min(total, base + IGN_TILE); i += IGN_THREADS) {
            if (kind == 0) {
                const long long at = (long long)b * d.N + i;
                const float lab = d.rpn_labels[at];
                if (ok && lab == 0.0f) s_queue[atomicAdd(&s_n, 1)] = i;
                else d.rpn_out[at] = lab;
            } else {
                const float fr = d.rois_bv[5 * (long long)i];
                const bool framed = fr >= 0.0f && fr < (float)d.B && fr == truncf(fr);
                const bool mine = framed ? fr == (float)b : b == 0;
                if (!mine) continue;
                const int32_t lab = d.roi_labels[i];
                if (ok && framed && lab == 0) s_queue[atomicAdd(&s_n, 1)] = i;
                else d.roi_out[i] = lab;
            }
        }
        __syncthreads();
        const int queued = s_n;
        __syncthreads();                                                     // every thread has read it before the next pass adds
        if (queued + IGN_TILE <= IGN_QUEUE && base + IGN_TILE < total) continue;   // (uniform) room for another tile
        // pass 2: one queued candidate per thread
        for (int c0 = 0; c0 < queued; c0 += IGN_THREADS) {
            const bool live = c0 + tid < queued;
            const int i = live ? s_queue[c0 + tid] : 0;
            IgnCand c = {};
            if (live) {
                if (kind == 0) {
                    int x1, y1, x2, y2;
                    grid_anchor(i, d.W, d.stride, x1, y1, x2, y2);
                    float M[12], P[6];
#pragma unroll
                    for (int j = 0; j < 12; ++j) M[j] = s_M[j];
                    anchor_to_lidar(x1, y1, x2, y2, P);
                    int32_t box[4];
                    image_box(M, P, box);
                    c.bv[0] = (double)x1; c.bv[1] = (double)y1; c.bv[2] = (double)x2; c.bv[3] = (double)y2;
#pragma unroll
                    for (int j = 0; j < 4; ++j) c.img[j] = (double)box[j];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        c.bv[j] = (double)d.rois_bv[5 * (long long)i + 1 + j];
                        c.img[j] = (double)d.rois_img[5 * (long long)i + 1 + j];
                    }
                }
                c.area_bv = ign_area(c.bv);
                c.area_img = ign_area(c.img);
            }
            bool hit = ign_walk(d.ign[0], o0[0], o1[0], s_box, live && c.area_bv > 0, c.bv, c.area_bv, d.T);
            hit = ign_walk(d.ign[1], o0[1], o1[1], s_box, live && !hit && c.area_img > 0, c.img, c.area_img, d.T) || hit;
            if (live) {
                if (kind == 0) d.rpn_out[(long long)b * d.N + i] = hit ? -1.0f : d.rpn_labels[(long long)b * d.N + i];   // (-0.0 stays -0.0)
                else d.roi_out[i] = hit ? -1 : 0;
                relabelled += hit ? 1 : 0;
            }
        }
        __syncthreads();                                                     // the queue has been read
        if (tid == 0) s_n = 0;
        __syncthreads();
    }

    if (!d.counts) return;
    for (int o = 32; o > 0; o >>= 1) relabelled += __shfl_down(relabelled, o);
    if ((tid & 63) == 0) s_red[tid >> 6] = relabelled;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < IGN_THREADS / 64; ++w) t += s_red[w];
        d.counts[2 * b + kind] = t;
    }
}

extern "C" int mv3d_ignore_relabel(const float *rpn_labels_dev, const int32_t *roi_labels_dev, const float *rois_bv_dev,
                                   const float *rois_img_dev, int num_rois, const float *calib_dev, int batch, int H, int W,
                                   int feat_stride, const float *ignore_bv_dev, const int32_t *ignore_bv_off_dev, int ignore_bv_rows,
                                   const float *ignore_img_dev, const int32_t *ignore_img_off_dev, int ignore_img_rows, double overlap,
                                   float *rpn_labels_out_dev, int32_t *roi_labels_out_dev, int32_t *counts_dev, int32_t *status_dev,
                                   void *stream)
{
    if (batch < 1 || batch > 65535 || H < 1 || W < 1 || feat_stride < 1 || num_rois < 0 || ignore_bv_rows < 0 || ignore_img_rows < 0)
        return MV3D_ERR_INVALID_ARG;
    if ((long long)H * W > INT32_MAX / 4) return MV3D_ERR_INVALID_ARG;
    if (((long long)(H > W ? H : W) - 1) * feat_stride + 20 > INT32_MAX) return MV3D_ERR_INVALID_ARG;     // the last anchor leaves int32
    if (!rpn_labels_dev || !rpn_labels_out_dev || !calib_dev || !ignore_bv_off_dev || !ignore_img_off_dev) return MV3D_ERR_INVALID_ARG;
    if (num_rois > 0 && (!roi_labels_dev || !roi_labels_out_dev || !rois_bv_dev || !rois_img_dev)) return MV3D_ERR_INVALID_ARG;
    if ((ignore_bv_rows > 0 && !ignore_bv_dev) || (ignore_img_rows > 0 && !ignore_img_dev)) return MV3D_ERR_INVALID_ARG;
    IgnoreDev d = {};
    d.rpn_labels = rpn_labels_dev; d.roi_labels = roi_labels_dev; d.rois_bv = rois_bv_dev; d.rois_img = rois_img_dev;
    d.calib = calib_dev; d.ign[0] = ignore_bv_dev; d.ign[1] = ignore_img_dev; d.off[0] = ignore_bv_off_dev; d.off[1] = ignore_img_off_dev;
    d.rows[0] = ignore_bv_rows; d.rows[1] = ignore_img_rows;
    d.B = batch; d.N = 4 * H * W; d.S = num_rois; d.W = W; d.stride = feat_stride; d.T = overlap;
    d.rpn_out = rpn_labels_out_dev; d.roi_out = roi_labels_out_dev; d.counts = counts_dev; d.status = status_dev;
    hipLaunchKernelGGL(ignore_relabel_kernel, dim3(batch, 2), dim3(IGN_THREADS), 0, (hipStream_t)stream, d);
    return mv3d_launch_status();
}
