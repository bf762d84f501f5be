// Test-time detection tail of a batch of frames (lib/fast_rcnn/test_mv.py:420-444, 491-501): per-class score cut,
// greedy NMS of the class's BEV boxes, cap of max_per_image over all classes -- for every frame of the serving step
// in two launches, without leaving the device.
//
//  detect_post_nms_kernel  grid (num_classes, batch), 1024 threads: ONE workgroup per (frame, class), everything in LDS.
//      1. keys      thread p reads cls_prob[row p, class j]; a candidate (score > score_thresh, in f32) gets the 64-bit
//                   key (mv3d_score_key(score) << 32 | p), everything else 0.
//      2. sort      bitonic sort of the keys, descending: larger score first, equal scores by larger row index (the low
//                   word) -- the library's tie rule; all keys of candidates are distinct, so the sort is exact and
//                   deterministic.  Non-candidates sink to the end; nc = position of the first 0.
//      3. boxes     s_box[p] / s_area[p] = BEV box and area (cpu_nms.pyx:24) of the candidate at sorted position p.
//      4. greedy    blocks of 64 sorted positions, in order.  Thread t owns positions t and t + 1024 and keeps their
//                   "alive" flags in registers, so block b belongs to wave b % 16.  That wave settles the block's own
//                   64 x 64 triangle serially over its alive boxes (one ballot per KEPT box) and publishes the block's kept
//                   mask; after one barrier every wave that holds later boxes tests them against the block's kept boxes
//                   (LDS broadcasts), in ascending order, and a box stops at its first suppressor.  That is the
//                   reference's order of evaluation, pair for pair, so a zero union is seen exactly where
//                   cpu_nms raises (bit 0 of status[f]; the pair does not suppress, as in nms.hip).
//      5. output    kept positions are compacted (popcounts of the masks) and the rows are written in
//                   descending score order: det_bv, det_cnr, det_cnr_r, det_row, det_count (the count BEFORE the cap).
//  detect_post_cap_kernel  grid (batch), 256 threads, only if max_per_image > 0: if the frame's kept detections number
//      more than max_per_image, every thread takes kept scores v, counts by binary search in each class's (descending)
//      list how many are > v and >= v; the max_per_image-th largest is the v with #(> v) < max_per_image <= #(>= v).
//      Every class then keeps its scores >= that value: a prefix, so only det_count shrinks.
// Steps 1-2 (dp_sort_candidates) and 5 (dp_emit) live in detect_post.h: the oriented tail (detect_post_oriented.hip) runs the same code.
#include "detect_post.h"
#include "nms_pair.h"

__global__ __launch_bounds__(DP_THREADS) void detect_post_nms_kernel(const DetectPostDev d)
{
    __shared__ unsigned long long s_sort[DP_MAX_ROWS];
    __shared__ float4 s_box[DP_MAX_ROWS];
    __shared__ float s_area[DP_MAX_ROWS];
    __shared__ unsigned long long s_kmask[DP_MAX_ROWS / 64];
    __shared__ unsigned short s_kpos[DP_MAX_ROWS];
    __shared__ int s_nc;
    const int j = blockIdx.x, f = blockIdx.y, t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int K = d.K, cap = d.cap;
    if (j == 0) {                                            // background: no detections
        if (t == 0) d.det_count[(long long)f * K] = 0;
        return;
    }
    const long long row0 = (long long)f * cap;

    // 1-2. keys, sort
    const int nc = dp_sort_candidates(d, j, f, s_sort, &s_nc);

    // 3. boxes in processing order
    for (int p = t; p < nc; p += DP_THREADS) {
        const int row = (int)(unsigned)s_sort[p];
        const float *b = d.pred_bv + (row0 + row) * (4 * K) + 4 * j;
        const float4 v = make_float4(b[0], b[1], b[2], b[3]);
        s_box[p] = v;
        s_area[p] = ((v.z - v.x) + 1.0f) * ((v.w - v.y) + 1.0f);     // cpu_nms.pyx:24
    }
    __syncthreads();

    // 4. greedy pass
    const int nblk = (nc + 63) >> 6;
    bool alive[2];
    float4 me[2];
    float marea[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int p = t + DP_THREADS * s;
        alive[s] = p < nc;
        me[s] = s_box[p];                                    // (p < DP_MAX_ROWS: in bounds; unused unless alive)
        marea[s] = s_area[p];
    }
    bool zero = false;
    for (int b = 0; b < nblk; ++b) {
        const int os = b / DP_WAVES;
        if (wave == b % DP_WAVES) {                          // the block's own triangle
            bool a = os ? alive[1] : alive[0];
            const float4 m4 = os ? me[1] : me[0];
            const float ma = os ? marea[1] : marea[0];
            unsigned long long m = __ballot(a), kept = 0ull;
            while (m) {
                const int i = __builtin_ctzll(m);
                kept |= 1ull << i;
                const float4 q = s_box[64 * b + i];
                const float qa = s_area[64 * b + i];
                if (a && lane > i) {
                    bool zd;
                    if (pair_suppresses(q.x, q.y, q.z, q.w, qa, m4.x, m4.y, m4.z, m4.w, ma, d.tf, zd)) a = false;
                    zero |= zd;
                }
                m = __ballot(a) & ~((2ull << i) - 1ull);
            }
            if (lane == 0) s_kmask[b] = kept;
        }
        __syncthreads();
        const unsigned long long km = s_kmask[b];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (wave + DP_WAVES * s <= b) continue;          // this wave's block of slot s is not behind block b
            bool a = alive[s];
            unsigned long long m = km;
            while (m && __any(a)) {
                const int i = __builtin_ctzll(m);
                m &= m - 1ull;
                const float4 q = s_box[64 * b + i];
                const float qa = s_area[64 * b + i];
                if (a) {
                    bool zd;
                    if (pair_suppresses(q.x, q.y, q.z, q.w, qa, me[s].x, me[s].y, me[s].z, me[s].w, marea[s], d.tf, zd)) a = false;
                    zero |= zd;
                }
            }
            alive[s] = a;
        }
    }
    if (__any(zero) && lane == 0) atomicOr(&d.status[f], MV3D_FLAG_ZERO_DIVISION);
    __syncthreads();

    // 5. kept positions, in order; outputs
    dp_emit<DP_THREADS>(d, j, f, nblk, s_kmask, s_kpos, s_sort, s_box);
}

// number of leading scores of a descending list that are > v (GE: >= v)
template <bool GE>
__device__ __forceinline__ int dp_count_before(const float *list, const int len, const float v)
{
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float x = list[5 * mid + 4];
        if (GE ? (x >= v) : (x > v)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void detect_post_cap_kernel(const DetectPostDev d)
{
    __shared__ int s_cnt[DP_MAX_CLASSES];
    __shared__ float s_thr;
    const int f = blockIdx.x, t = threadIdx.x, K = d.K, m = d.max_per_image;
    if (t < K) s_cnt[t] = d.det_count[(long long)f * K + t];
    __syncthreads();
    int total = 0;
    for (int j = 1; j < K; ++j) total += s_cnt[j];
    if (total <= m) return;                                  // test_mv.py:493
    const float *lists = d.det_bv + (long long)f * K * d.cap * 5;
    for (int e = t; e < total; e += 256) {
        int j = 1, s = e;
        while (s >= s_cnt[j]) { s -= s_cnt[j]; ++j; }
        const float v = lists[((long long)j * d.cap + s) * 5 + 4];
        int gt = 0, ge = 0;
        for (int c = 1; c < K; ++c) {
            const float *l = lists + (long long)c * d.cap * 5;
            gt += dp_count_before<false>(l, s_cnt[c], v);
            ge += dp_count_before<true>(l, s_cnt[c], v);
        }
        if (gt < m && m <= ge) s_thr = v;                    // np.sort(image_scores)[-max_per_image]
    }
    __syncthreads();
    const float thr = s_thr;
    if (t >= 1 && t < K)
        d.det_count[(long long)f * K + t] = dp_count_before<true>(lists + (long long)t * d.cap * 5, s_cnt[t], thr);
}

void mv3d_launch_detect_post_cap(const DetectPostDev &d, int batch, hipStream_t stream)
{
    hipLaunchKernelGGL(detect_post_cap_kernel, dim3(batch), dim3(256), 0, stream, d);
}

extern "C" size_t mv3d_detect_post_workspace_bytes(int batch, const mv3d_detect_post_params *p)
{
    (void)batch; (void)p;
    return 0;                                                // everything lives in LDS and in the outputs
}

extern "C" int mv3d_detect_post(const float *cls_prob_dev, const float *pred_bv_dev, const float *corners_dev,
                                const float *pred_cnr_r_dev, const int32_t *num_rois_dev, int batch,
                                const mv3d_detect_post_params *p, float *det_bv_dev, float *det_cnr_dev,
                                float *det_cnr_r_dev, int32_t *det_row_dev, int32_t *det_count_dev, int32_t *status_dev,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    if (!dp_params_ok(batch, p) || !cls_prob_dev || !pred_bv_dev || !corners_dev || !det_bv_dev || !det_cnr_dev ||
        !det_row_dev || !det_count_dev || !status_dev || (pred_cnr_r_dev && !det_cnr_r_dev))
        return MV3D_ERR_INVALID_ARG;
    DetectPostDev d;
    d.cls_prob = cls_prob_dev; d.pred_bv = pred_bv_dev; d.corners = corners_dev; d.pred_cnr_r = pred_cnr_r_dev;
    d.num_rois = num_rois_dev;
    d.det_bv = det_bv_dev; d.det_cnr = det_cnr_dev; d.det_cnr_r = det_cnr_r_dev;
    d.det_row = det_row_dev; d.det_count = det_count_dev; d.status = status_dev;
    d.K = p->num_classes; d.cap = p->rows_per_frame; d.max_per_image = p->max_per_image;
    d.score_thresh = p->score_thresh;
    d.tf = p->nms_strict_gt ? nextafterf((float)p->nms_thresh, INFINITY) : mv3d_ceil_f32(p->nms_thresh);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(detect_post_nms_kernel, dim3(d.K, batch), dim3(DP_THREADS), 0, st, d);
    if (d.max_per_image > 0) mv3d_launch_detect_post_cap(d, batch, st);
    return mv3d_launch_status();
}
