// Proposal recall on the device: the greedy matching of lib/datasets/imdb.py:162-196 (evaluate_recall) for every frame of a
// split and every proposal limit in ONE launch.
//
//   proposal_recall_kernel   one 256-lane workgroup per (frame, limit), limits on blockIdx.y.  The frame's objects and their
//                            running (max, argmax, used) live in LDS; lanes stride over the boxes; overlaps are recomputed on
//                            the fly (an R x G f64 block does not fit LDS at R = 2000).
//
// Contract per (frame f, limit l), R = the frame's boxes, G = its objects (tests/recall_restatement.py follows it line by line):
//   overlap  (lib/utils/bbox.pyx:15 bbox_overlaps, f64 from the f32 inputs, the order of the oracle's mv3d_ref_bbox_overlaps, no fma)
//            qarea = ((q2 - q0) + 1) * ((q3 - q1) + 1)
//            iw = (min(b2, q2) - max(b0, q0)) + 1;  ih = (min(b3, q3) - max(b1, q1)) + 1
//            iw > 0 and ih > 0:  ua = ((((b2 - b0) + 1) * ((b3 - b1) + 1)) + qarea) - iw * ih;  o = (iw * ih) / ua;  else o = 0
//   matching n, R == 0, rounds, short, finite and counts as the header comment of recall_match.h states them, with this overlap;
//            finite is over the 4 coordinates of ALL of the frame's R boxes and of its G objects, and this kernel sets the bit.
#include "recall_match.h"

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

__global__ __launch_bounds__(RM_THREADS) void proposal_recall_kernel(
    const int32_t *__restrict__ box_off, const int32_t *__restrict__ gt_off, const float *__restrict__ boxes,
    const float *__restrict__ gts, const int32_t *__restrict__ limits, const double *__restrict__ thresholds, int T, int short_mode,
    long long Gtot, double *__restrict__ gt_overlaps, int32_t *__restrict__ counts, int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) float s_box[4 * PR_LDS_BOXES];
    __shared__ PrGt s_gt[MV3D_RECALL_MAX_GT];
    __shared__ RmState<PR_MASK_BOXES> s_match;

    const int f = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
    const int b0 = box_off[f], R = box_off[f + 1] - b0, g0 = gt_off[f], G = gt_off[f + 1] - g0;
    const int limit = limits[l];
    const int n = (limit <= 0 || limit > R) ? R : limit;
    double *out = gt_overlaps + (long long)l * Gtot + g0;
    if (R == 0) {                                      // skipped frame
        for (int g = tid; g < G; g += RM_THREADS) out[g] = -1.0;
        return;
    }
    const float *fbox = boxes + 4 * (long long)b0;
    const bool staged = n <= PR_LDS_BOXES;             // (workgroup-uniform)

    bool bad = false;
    for (int p = tid; p < 4 * R; p += RM_THREADS) {
        const float v = fbox[p];
        bad = bad || !isfinite(v);
        if (staged && p < 4 * n) s_box[p] = v;
    }
    for (int g = tid; g < G; g += RM_THREADS) {
        const float *q = gts + 4 * (long long)(g0 + g);
        const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
        bad = bad || !isfinite(q0) || !isfinite(q1) || !isfinite(q2) || !isfinite(q3);
        PrGt t;
        t.q0 = q0; t.q1 = q1; t.q2 = q2; t.q3 = q3;
        t.area = (((double)q2 - (double)q0) + 1.0) * (((double)q3 - (double)q1) + 1.0);
        s_gt[g] = t;
    }
    rm_clear(s_match, G);
    const int nbad = __syncthreads_or(bad ? 1 : 0);    // (also publishes s_box, s_gt, s_match)

    if (nbad && tid == 0) atomicOr(status + f, MV3D_RECALL_STATUS_NONFINITE);
    auto overlap = [&](int g) {
        const PrGt q = s_gt[g];
        return [=](int i) {
            if (staged) {
                const float4 b = reinterpret_cast<const float4 *>(s_box)[i];
                return pr_overlap(b.x, b.y, b.z, b.w, q);
            }
            const float *b = fbox + 4 * (long long)i;
            return pr_overlap(b[0], b[1], b[2], b[3], q);
        };
    };
    rm_match(s_match, G, n, nbad != 0, short_mode, overlap, out, thresholds, T, counts + (long long)l * T, status + f);
}

// ------------------------------------------------------------------ C-ABI
extern "C" int mv3d_proposal_recall(const mv3d_recall_split *s, double *gt_overlaps_dev, int32_t *counts_dev, int32_t *status_dev,
                                    void *stream)
{
    if (rm_validate_split(s) != MV3D_OK) return MV3D_ERR_INVALID_ARG;
    const int F = s->num_frames;
    if ((F > 0 && !status_dev) || (s->num_gts > 0 && (!s->gt_dev || !gt_overlaps_dev)) || (s->num_thresholds > 0 && !counts_dev))
        return MV3D_ERR_INVALID_ARG;
    if (s->num_thresholds > 0)
        MV3D_HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(int32_t) * (size_t)s->num_limits * (size_t)s->num_thresholds, (hipStream_t)stream));
    if (F == 0) return MV3D_OK;
    MV3D_HIP_TRY(hipMemsetAsync(status_dev, 0, sizeof(int32_t) * (size_t)F, (hipStream_t)stream));
    hipLaunchKernelGGL(proposal_recall_kernel, dim3(F, s->num_limits), dim3(RM_THREADS), 0, (hipStream_t)stream, s->box_off_dev,
                       s->gt_off_dev, s->boxes_dev, s->gt_dev, s->limits_dev, s->thresholds_dev, s->num_thresholds, s->short_mode,
                       (long long)s->num_gts, gt_overlaps_dev, counts_dev, status_dev);
    return mv3d_launch_status();
}
