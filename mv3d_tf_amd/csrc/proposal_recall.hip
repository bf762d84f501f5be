// Proposal recall on the device: the greedy matching of lib/datasets/imdb.py:162-196 (evaluate_recall) for every frame of a
// split and every proposal limit in ONE launch.
//
//   proposal_recall_kernel   one 256-lane workgroup per (frame, limit), limits on blockIdx.y.  The frame's objects and their
//                            running (max, argmax, used) live in LDS; lanes stride over the boxes; overlaps are recomputed on
//                            the fly (an R x G f64 block does not fit LDS at R = 2000).
//
// Contract per (frame f, limit l), R = the frame's boxes, G = its objects (tests/recall_restatement.py follows it line by line):
//   n        = limit <= 0 ? R : min(R, limit)                       (boxes[:limit], imdb.py:171-172)
//   R == 0   the frame is skipped (imdb.py:169-170): its G entries are -1.0, nothing is counted, no status.
//   overlap  (lib/utils/bbox.pyx:15 bbox_overlaps, f64 from the f32 inputs, the order of the oracle's mv3d_ref_bbox_overlaps, no fma)
//            qarea = ((q2 - q0) + 1) * ((q3 - q1) + 1)
//            iw = (min(b2, q2) - max(b0, q0)) + 1;  ih = (min(b3, q3) - max(b1, q1)) + 1
//            iw > 0 and ih > 0:  ua = ((((b2 - b0) + 1) * ((b3 - b1) + 1)) + qarea) - iw * ih;  o = (iw * ih) / ua;  else o = 0
//   rounds   j = 0 .. G-1 (imdb.py:178-194); used box rows and used object columns count as -1:
//            per object, the maximum over the boxes and the first index of that maximum     (overlaps.max / argmax(axis=0))
//            gt_ind = the object with the largest maximum, first index on a tie               (max_overlaps.argmax())
//            box_ind = that object's box                                                      (argmax_overlaps[gt_ind])
//            the overlap is recorded at position j of the frame's block, NOT at gt_ind (the reference's _gt_overlaps[j]; the
//            vector is only ever used sorted, but parity is on the raw vector); box_ind and gt_ind are marked used.
//   short    0 < n < G: from round n on every row is used and the reference fails assert(gt_ovr >= 0).  short_mode 0: the
//            frame's status gets MV3D_RECALL_STATUS_SHORT and rounds n .. G-1 record -1.0; short_mode 1 (this library's
//            definition, not the reference's): they record 0.0, no status.
//   finite   R > 0 and any non-finite coordinate among ALL of the frame's R boxes (whatever the limit) or its G objects: status
//            MV3D_RECALL_STATUS_NONFINITE, the frame records 0.0 throughout (the reference's result there hangs on C min / max
//            of NaN and is not a target).
//   counts   counts[l][t] += the number of the frame's G recorded values >= thresholds[t] (skipped frames add nothing).
// An overlap of finite boxes is >= 0, so while an unused box is left a used row (-1) never holds a column's maximum or ties
// with it: the kernel skips used boxes instead of storing -1, and the first-index (value, index) reductions across lanes
// give exactly numpy's argmax.  After a round only the columns whose argmax was the consumed box are recomputed.
#include "common.h"

#define PR_THREADS 256
#define PR_WAVES 4
#define PR_LDS_BOXES 2048     // boxes of one (frame, limit) staged in LDS (f32 x 4: 32 KiB); more are read from global memory
#define PR_MASK_BOXES 16384   // used-box bits kept in LDS (2 KiB); a used box beyond them is looked up in the list of used boxes

struct PrGt {
    double q0, q1, q2, q3, area;
};

__device__ __forceinline__ double pr_overlap(float fb0, float fb1, float fb2, float fb3, const PrGt &q)
{
    const double b0 = fb0, b1 = fb1, b2 = fb2, b3 = fb3;
    const double iw = ((b2 < q.q2 ? b2 : q.q2) - (b0 > q.q0 ? b0 : q.q0)) + 1.0;
    if (!(iw > 0.0)) return 0.0;
    const double ih = ((b3 < q.q3 ? b3 : q.q3) - (b1 > q.q1 ? b1 : q.q1)) + 1.0;
    if (!(ih > 0.0)) return 0.0;
    const double inter = iw * ih;
    const double ua = ((((b2 - b0) + 1.0) * ((b3 - b1) + 1.0)) + q.area) - inter;
    return inter / ua;
}

// (largest key, first index) over the wave's 64 lanes
__device__ __forceinline__ void pr_argmax(double &key, int &idx)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double k2 = __shfl_xor(key, o);
        const int i2 = __shfl_xor(idx, o);
        if (k2 > key || (k2 == key && i2 < idx)) { key = k2; idx = i2; }
    }
}

__global__ __launch_bounds__(PR_THREADS) void proposal_recall_kernel(
    const int32_t *__restrict__ box_off, const int32_t *__restrict__ gt_off, const float *__restrict__ boxes,
    const float *__restrict__ gts, const int32_t *__restrict__ limits, const double *__restrict__ thresholds, int T, int short_mode,
    long long Gtot, double *__restrict__ gt_overlaps, int32_t *__restrict__ counts, int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) float s_box[4 * PR_LDS_BOXES];
    __shared__ PrGt s_gt[MV3D_RECALL_MAX_GT];
    __shared__ double s_max[MV3D_RECALL_MAX_GT];      // per object: the maximum over the unused boxes ...
    __shared__ int s_arg[MV3D_RECALL_MAX_GT];         // ... and the first box that has it
    __shared__ int s_col_used[MV3D_RECALL_MAX_GT];
    __shared__ double s_rec[MV3D_RECALL_MAX_GT];      // the frame's recorded overlaps, round by round
    __shared__ int s_used_box[MV3D_RECALL_MAX_GT];    // the boxes consumed so far, in round order
    __shared__ uint32_t s_mask[PR_MASK_BOXES / 32];
    __shared__ double s_wkey[PR_WAVES];
    __shared__ int s_widx[PR_WAVES];

    const int f = blockIdx.x, l = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = box_off[f], R = box_off[f + 1] - b0, g0 = gt_off[f], G = gt_off[f + 1] - g0;
    const int limit = limits[l];
    const int n = (limit <= 0 || limit > R) ? R : limit;
    double *out = gt_overlaps + (long long)l * Gtot + g0;
    if (R == 0) {                                      // skipped frame
        for (int g = tid; g < G; g += PR_THREADS) out[g] = -1.0;
        return;
    }
    const float *fbox = boxes + 4 * (long long)b0;
    const bool staged = n <= PR_LDS_BOXES;             // (workgroup-uniform)

    bool bad = false;
    for (int p = tid; p < 4 * R; p += PR_THREADS) {
        const float v = fbox[p];
        bad = bad || !isfinite(v);
        if (staged && p < 4 * n) s_box[p] = v;
    }
    for (int g = tid; g < G; g += PR_THREADS) {
        const float *q = gts + 4 * (long long)(g0 + g);
        const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
        bad = bad || !isfinite(q0) || !isfinite(q1) || !isfinite(q2) || !isfinite(q3);
        PrGt t;
        t.q0 = q0; t.q1 = q1; t.q2 = q2; t.q3 = q3;
        t.area = (((double)q2 - (double)q0) + 1.0) * (((double)q3 - (double)q1) + 1.0);
        s_gt[g] = t;
        s_col_used[g] = 0;
    }
    for (int w = tid; w < PR_MASK_BOXES / 32; w += PR_THREADS) s_mask[w] = 0u;
    const int nbad = __syncthreads_or(bad ? 1 : 0);    // (also publishes s_box, s_gt, s_mask)

    const int rounds = G < n ? G : n;
    if (nbad) {
        for (int g = tid; g < G; g += PR_THREADS) s_rec[g] = 0.0;
        if (tid == 0) atomicOr(status + f, MV3D_RECALL_STATUS_NONFINITE);
    } else {
        // the maximum of column g over the unused boxes (`nused` of them consumed so far) and its first index
        auto column = [&](int g, int nused) {
            const PrGt q = s_gt[g];
            double best = -1.0;
            int bi = INT32_MAX;
            for (int i = lane; i < n; i += 64) {
                bool used = false;
                if (nused > 0) {
                    if (i < PR_MASK_BOXES) used = (s_mask[i >> 5] >> (i & 31)) & 1u;
                    else
                        for (int k = 0; k < nused; ++k) used = used || s_used_box[k] == i;
                }
                if (used) continue;
                double o;
                if (staged) {
                    const float4 b = reinterpret_cast<const float4 *>(s_box)[i];
                    o = pr_overlap(b.x, b.y, b.z, b.w, q);
                } else {
                    const float *b = fbox + 4 * (long long)i;
                    o = pr_overlap(b[0], b[1], b[2], b[3], q);
                }
                if (o > best) { best = o; bi = i; }
            }
            pr_argmax(best, bi);
            if (lane == 0) { s_max[g] = best; s_arg[g] = bi; }
        };
        for (int g = wave; g < G; g += PR_WAVES) column(g, 0);
        __syncthreads();
        for (int j = 0; j < rounds; ++j) {
            // max_overlaps.argmax() over the unused columns: lane t holds column t
            double key = -INFINITY;
            int idx = INT32_MAX;
            if (tid < G && !s_col_used[tid]) { key = s_max[tid]; idx = tid; }
            pr_argmax(key, idx);
            if (lane == 0) { s_wkey[wave] = key; s_widx[wave] = idx; }
            __syncthreads();
            key = s_wkey[0]; idx = s_widx[0];
#pragma unroll
            for (int w = 1; w < PR_WAVES; ++w) {
                const double k2 = s_wkey[w];
                const int i2 = s_widx[w];
                if (k2 > key || (k2 == key && i2 < idx)) { key = k2; idx = i2; }
            }
            const int box = s_arg[idx];
            if (tid == 0) {                             // (nothing a lane still reads in this phase)
                s_rec[j] = key;
                s_col_used[idx] = 1;
                s_used_box[j] = box;
                if (box < PR_MASK_BOXES) s_mask[box >> 5] |= 1u << (box & 31);
            }
            __syncthreads();
            if (j + 1 < rounds)
                for (int g = wave; g < G; g += PR_WAVES)
                    if (!s_col_used[g] && s_arg[g] == box) column(g, j + 1);
            __syncthreads();
        }
        if (rounds < G) {                               // short frame: no unused box is left
            for (int j = rounds + tid; j < G; j += PR_THREADS) s_rec[j] = short_mode == MV3D_RECALL_SHORT_ZERO ? 0.0 : -1.0;
            if (tid == 0 && short_mode != MV3D_RECALL_SHORT_ZERO) atomicOr(status + f, MV3D_RECALL_STATUS_SHORT);
        }
    }
    __syncthreads();
    for (int g = tid; g < G; g += PR_THREADS) out[g] = s_rec[g];
    for (int t = wave; t < T; t += PR_WAVES) {
        const double thr = thresholds[t];
        int c = 0;
        for (int g = lane; g < MV3D_RECALL_MAX_GT; g += 64) c += __popcll(__ballot(g < G && s_rec[g] >= thr));
        if (lane == 0 && c) atomicAdd(counts + (long long)l * T + t, c);
    }
}

// ------------------------------------------------------------------ C-ABI
extern "C" int mv3d_proposal_recall(const mv3d_recall_split *s, double *gt_overlaps_dev, int32_t *counts_dev, int32_t *status_dev,
                                    void *stream)
{
    if (!s || s->num_frames < 0 || s->num_gts < 0 || s->num_boxes < 0 || s->num_boxes > INT32_MAX || s->num_limits < 1 ||
        s->num_limits > 65535 || s->num_thresholds < 0 || !s->box_off || !s->gt_off || !s->limits_dev)
        return MV3D_ERR_INVALID_ARG;
    if (s->short_mode != MV3D_RECALL_SHORT_ASSERT && s->short_mode != MV3D_RECALL_SHORT_ZERO) return MV3D_ERR_INVALID_ARG;
    const int F = s->num_frames;
    if (s->box_off[0] != 0 || s->gt_off[0] != 0 || s->box_off[F] != s->num_boxes || s->gt_off[F] != s->num_gts) return MV3D_ERR_INVALID_ARG;
    for (int f = 0; f < F; ++f) {
        const long long R = (long long)s->box_off[f + 1] - s->box_off[f], G = (long long)s->gt_off[f + 1] - s->gt_off[f];
        if (R < 0 || G < 0 || G > MV3D_RECALL_MAX_GT) return MV3D_ERR_INVALID_ARG;
    }
    if (F > 0 && (!s->box_off_dev || !s->gt_off_dev || !status_dev)) return MV3D_ERR_INVALID_ARG;
    if (s->num_boxes > 0 && !s->boxes_dev) return MV3D_ERR_INVALID_ARG;
    if (s->num_gts > 0 && (!s->gt_dev || !gt_overlaps_dev)) return MV3D_ERR_INVALID_ARG;
    if (s->num_thresholds > 0 && (!s->thresholds_dev || !counts_dev)) return MV3D_ERR_INVALID_ARG;
    if (s->num_thresholds > 0)
        MV3D_HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(int32_t) * (size_t)s->num_limits * (size_t)s->num_thresholds, (hipStream_t)stream));
    if (F == 0) return MV3D_OK;
    MV3D_HIP_TRY(hipMemsetAsync(status_dev, 0, sizeof(int32_t) * (size_t)F, (hipStream_t)stream));
    hipLaunchKernelGGL(proposal_recall_kernel, dim3(F, s->num_limits), dim3(PR_THREADS), 0, (hipStream_t)stream, s->box_off_dev,
                       s->gt_off_dev, s->boxes_dev, s->gt_dev, s->limits_dev, s->thresholds_dev, s->num_thresholds, s->short_mode,
                       (long long)s->num_gts, gt_overlaps_dev, counts_dev, status_dev);
    return mv3d_launch_status();
}
