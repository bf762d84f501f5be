// proposal_target_layer_3d for gfx950 (one frame): lib/rpn_msr/proposal_target_layer_tf.py:19-94
// with _sample_rois_3d (:227-298), lib/utils/bbox.pyx:15-55 (f64 IoU), lib/fast_rcnn/
// bbox_transform.py:61-72 (corner targets), _get_bbox_regression_labels_3d (:172-194) and the image
// projection (lib/utils/transform.py:483-500) fused in.
//
//  pt_overlap_kernel  per candidate ROI (proposals followed by the G ground-truth boxes, :38-44):
//                     f64 IoU against the GT staged in LDS, first-argmax / max.
//  pt_compact_kernel  one workgroup: ordered compaction of the fg (max_ov >= FG_THRESH) and bg
//                     (LO <= max_ov < HI) candidate lists + counts.
//  (host)             draws npr.permutation(n_fg) / (n_bg) from the numpy global RNG: draw-for-draw
//                     parity with `npr.choice(inds, size=k, replace=False)`.
//  pt_emit_kernel     eight lanes per sampled ROI (one per corner): gathers the ROI, its 8 corners (f32), corner
//                     targets (gt - roi) / ||gt_p0 - gt_p6|| in f32, class-slot expansion, image box and, for the
//                     batched entry, the third view's ROI (front_view.hip) of the same 3D box.
#include <math.h>
#include "proposal_target.h"

__global__ __launch_bounds__(256) void pt_overlap_kernel(PtBatch bt)
{
    const PtDev &d = bt.f[blockIdx.y].d;
    __shared__ float s_gt[TARGET_MAX_GT * 4];
    stage_gt_bv(d.gt_bv, d.G, s_gt);
    __syncthreads();
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int R = pt_num_rois(d);
    if (r >= R + d.G) return;
    float b[5];
    cand_bv(d, R, r, b);
    const double b0 = b[1], b1 = b[2], b2 = b[3], b3 = b[4];
    double mx = 0.0;
    int am = 0;
    // bbox.pyx:33-54; overlaps.argmax(axis=1) = first maximum, overlaps.max(axis=1) (:233-237)
    for (int g = 0; g < d.G; ++g) {
        const double o = bbox_overlap_f64(b0, b1, b2, b3, s_gt[4 * g], s_gt[4 * g + 1], s_gt[4 * g + 2], s_gt[4 * g + 3]);
        if (g == 0 || o > mx) { mx = o; am = g; }
    }
    d.max_ov[r] = mx;
    d.assign[r] = am;
}

__global__ __launch_bounds__(1024) void pt_compact_kernel(PtBatch bt, PtMirror m)
{
    const PtDev &d = bt.f[blockIdx.y].d;
    int32_t *counts = bt.f[blockIdx.y].counts;
    if (m.h_report) {                                            // the frame's reports for the host (PtMirror): the head of the anchor report
        const int f = blockIdx.y;
        const uint4 *src = reinterpret_cast<const uint4 *>(m.report + (size_t)f * m.report_row);
        uint4 *dst = reinterpret_cast<uint4 *>(m.h_report + (size_t)f * m.h_row);
        for (size_t j = threadIdx.x; j < m.h_row / 16; j += 1024) dst[j] = src[j];
        if (threadIdx.x < 2) m.h_num_proposals[threadIdx.x * m.batch + f] = m.num_proposals[threadIdx.x * m.batch + f];
    }
    const int n = pt_num_rois(d) + d.G;
    int tot[2];
    mv3d_block_compact<2>(
        n,
        [&](int r, bool f[2]) {
            const double mx = d.max_ov[r];
            f[0] = (mx >= d.fg_thresh);                          // :246
            f[1] = (mx < d.bg_hi) && (mx >= d.bg_lo);            // :259-260
        },
        [&](int k, int pos, int r) { (k == 0 ? d.fg_list : d.bg_list)[pos] = r; },
        tot);
    if (threadIdx.x == 0) { counts[0] = n; counts[1] = tot[0]; counts[2] = tot[1]; counts[3] = 0; }
    if (m.h_report && threadIdx.x < 4)                            // (the totals are every thread's)
        m.h_pt_counts[4 * blockIdx.y + threadIdx.x] = threadIdx.x == 0 ? n : threadIdx.x == 1 ? tot[0] : threadIdx.x == 2 ? tot[1] : 0;
}

// (bodies: proposal_target.h)
__global__ __launch_bounds__(PT_EMIT_THREADS) void pt_emit_kernel(PtBatch bt) { pt_emit_body(pt_emit_frame(bt.f[blockIdx.y]), blockIdx.x); }

extern "C" size_t mv3d_proposal_target_workspace_bytes(int num_rois, int G)
{
    PtLayout L;
    return pt_layout(num_rois, G, L) ? L.total : 0;
}

static int pt_stage1_batch(int batch, const float *const *rois_bv_dev, const float *const *rois_3d_dev, const int *num_rois,
                           const int32_t *const *num_rois_dev, const float *const *gt_bv_dev, const float *const *gt_3d_dev,
                           const int *G, const mv3d_proposal_target_params *p, int32_t *const *counts_dev,
                           void *const *workspace, const size_t *workspace_bytes, void *stream, const PtMirror &mirror = PtMirror{})
{
    if (batch <= 0 || batch > PT_MAX_BATCH || !p || !rois_bv_dev || !rois_3d_dev || !num_rois || !gt_bv_dev || !gt_3d_dev || !G ||
        !counts_dev || !workspace || !workspace_bytes)
        return MV3D_ERR_INVALID_ARG;
    PtBatch bt = {};
    int most = 0;
    for (int b = 0; b < batch; ++b) {
        PtLayout L;
        if (!pt_layout(num_rois[b], G[b], L) || !gt_bv_dev[b] || !gt_3d_dev[b] || !counts_dev[b] ||
            (num_rois[b] > 0 && (!rois_bv_dev[b] || !rois_3d_dev[b])))
            return MV3D_ERR_INVALID_ARG;
        if (!workspace[b] || workspace_bytes[b] < L.total || ((uintptr_t)workspace[b] % MV3D_ALIGN)) return MV3D_ERR_WORKSPACE;
        pt_fill(bt.f[b].d, L, (char *)workspace[b], rois_bv_dev[b], rois_3d_dev[b], num_rois[b], gt_bv_dev[b], gt_3d_dev[b], G[b], &p[b]);
        bt.f[b].d.R_dev = num_rois_dev ? num_rois_dev[b] : nullptr;
        bt.f[b].counts = counts_dev[b];
        if (num_rois[b] + G[b] > most) most = num_rois[b] + G[b];
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pt_overlap_kernel, dim3((most + 255) / 256, batch), dim3(256), 0, s, bt);
    hipLaunchKernelGGL(pt_compact_kernel, dim3(1, batch), dim3(1024), 0, s, bt, mirror);
    return mv3d_launch_status();
}

extern "C" int mv3d_proposal_target_stage1_batch(int batch, const float *const *rois_bv_dev, const float *const *rois_3d_dev,
                                                 const int *num_rois, const float *const *gt_bv_dev, const float *const *gt_3d_dev,
                                                 const int *G, const mv3d_proposal_target_params *p, int32_t *const *counts_dev,
                                                 void *const *workspace, const size_t *workspace_bytes, void *stream)
{
    return pt_stage1_batch(batch, rois_bv_dev, rois_3d_dev, num_rois, nullptr, gt_bv_dev, gt_3d_dev, G, p, counts_dev, workspace,
                           workspace_bytes, stream);
}

extern "C" int mv3d_proposal_target_stage1_batch_devn(int batch, const float *const *rois_bv_dev, const float *const *rois_3d_dev,
                                                      const int *num_rois_cap, const int32_t *const *num_rois_dev,
                                                      const float *const *gt_bv_dev, const float *const *gt_3d_dev, const int *G,
                                                      const mv3d_proposal_target_params *p, int32_t *const *counts_dev,
                                                      void *const *workspace, const size_t *workspace_bytes, void *stream)
{
    if (!num_rois_dev) return MV3D_ERR_INVALID_ARG;
    for (int b = 0; b < batch && b < PT_MAX_BATCH; ++b) if (!num_rois_dev[b]) return MV3D_ERR_INVALID_ARG;
    return pt_stage1_batch(batch, rois_bv_dev, rois_3d_dev, num_rois_cap, num_rois_dev, gt_bv_dev, gt_3d_dev, G, p, counts_dev,
                           workspace, workspace_bytes, stream);
}

int mv3d_pt_stage1_batch_mirrored(int batch, const float *const *rois_bv_dev, const float *const *rois_3d_dev, const int *num_rois_cap,
                                  const int32_t *const *num_rois_dev, const float *const *gt_bv_dev, const float *const *gt_3d_dev,
                                  const int *G, const mv3d_proposal_target_params *p, int32_t *const *counts_dev, void *const *workspace,
                                  const size_t *workspace_bytes, const PtMirror &mirror, void *stream)
{
    if (!num_rois_dev || mirror.batch != batch) return MV3D_ERR_INVALID_ARG;
    if (mirror.h_report && (!mirror.report || !mirror.h_pt_counts || !mirror.num_proposals || !mirror.h_num_proposals || mirror.h_row % 16 ||
                            mirror.h_row > mirror.report_row || mirror.report_row % 16 || (uintptr_t)mirror.report % 16 ||
                            (uintptr_t)mirror.h_report % 16))
        return MV3D_ERR_INVALID_ARG;
    for (int b = 0; b < batch && b < PT_MAX_BATCH; ++b) if (!num_rois_dev[b]) return MV3D_ERR_INVALID_ARG;
    return pt_stage1_batch(batch, rois_bv_dev, rois_3d_dev, num_rois_cap, num_rois_dev, gt_bv_dev, gt_3d_dev, G, p, counts_dev, workspace,
                           workspace_bytes, stream, mirror);
}

extern "C" int mv3d_proposal_target_stage1(const float *rois_bv_dev, const float *rois_3d_dev, int num_rois,
                                           const float *gt_bv_dev, const float *gt_3d_dev, int G,
                                           const mv3d_proposal_target_params *p, int32_t *counts_dev, void *workspace,
                                           size_t workspace_bytes, void *stream)
{
    return mv3d_proposal_target_stage1_batch(1, &rois_bv_dev, &rois_3d_dev, &num_rois, &gt_bv_dev, &gt_3d_dev, &G, p, &counts_dev,
                                             &workspace, &workspace_bytes, stream);
}

static int pt_stage2_batch(int batch, const float *const *rois_bv_dev, const float *const *rois_3d_dev,
                                                 const int *num_rois, const int32_t *const *num_rois_dev, const float *const *gt_bv_dev, const float *const *gt_3d_dev,
                                                 const float *const *gt_corners_dev, const int *G, const float *const *calib_dev,
                                                 const mv3d_proposal_target_params *p, const int32_t *const *fg_pick_dev,
                                                 const int *n_fg, const int32_t *const *bg_pick_dev, const int *n_bg,
                                                 float *const *rois_bv_out, float *const *rois_img_out, int32_t *const *labels_out,
                                                 float *const *bbox_targets_out, float *const *rois_3d_out,
                                                 float *const *rois_fv_out, void *const *workspace,
                                                 const size_t *workspace_bytes, void *stream)
{
    PtBatch bt;
    int most;
    const int rc = pt_stage2_args(batch, rois_bv_dev, rois_3d_dev, num_rois, num_rois_dev, gt_bv_dev, gt_3d_dev, gt_corners_dev, G, calib_dev, p,
                                  fg_pick_dev, n_fg, bg_pick_dev, n_bg, rois_bv_out, rois_img_out, labels_out, bbox_targets_out, rois_3d_out,
                                  rois_fv_out, workspace, workspace_bytes, bt, most);
    if (rc != MV3D_OK) return rc;
    if (most == 0) return MV3D_OK;
    hipLaunchKernelGGL(pt_emit_kernel, dim3(pt_emit_workgroups(most), batch), dim3(PT_EMIT_THREADS), 0,
                       (hipStream_t)stream, bt);
    return mv3d_launch_status();
}

#define PT_S2_ARGS gt_bv_dev, gt_3d_dev, gt_corners_dev, G, calib_dev, p, fg_pick_dev, n_fg, bg_pick_dev, n_bg, rois_bv_out, rois_img_out, \
                   labels_out, bbox_targets_out, rois_3d_out, rois_fv_out, workspace, workspace_bytes, stream
extern "C" int mv3d_proposal_target_stage2_batch(int batch, const float *const *rois_bv_dev, const float *const *rois_3d_dev,
                                                 const int *num_rois, const float *const *gt_bv_dev, const float *const *gt_3d_dev,
                                                 const float *const *gt_corners_dev, const int *G, const float *const *calib_dev,
                                                 const mv3d_proposal_target_params *p, const int32_t *const *fg_pick_dev,
                                                 const int *n_fg, const int32_t *const *bg_pick_dev, const int *n_bg,
                                                 float *const *rois_bv_out, float *const *rois_img_out, int32_t *const *labels_out,
                                                 float *const *bbox_targets_out, float *const *rois_3d_out,
                                                 float *const *rois_fv_out, void *const *workspace,
                                                 const size_t *workspace_bytes, void *stream)
{
    return pt_stage2_batch(batch, rois_bv_dev, rois_3d_dev, num_rois, nullptr, PT_S2_ARGS);
}

extern "C" int mv3d_proposal_target_stage2_batch_devn(int batch, const float *const *rois_bv_dev, const float *const *rois_3d_dev,
                                                      const int *num_rois_cap, const int32_t *const *num_rois_dev,
                                                      const float *const *gt_bv_dev, const float *const *gt_3d_dev,
                                                      const float *const *gt_corners_dev, const int *G, const float *const *calib_dev,
                                                      const mv3d_proposal_target_params *p, const int32_t *const *fg_pick_dev,
                                                      const int *n_fg, const int32_t *const *bg_pick_dev, const int *n_bg,
                                                      float *const *rois_bv_out, float *const *rois_img_out, int32_t *const *labels_out,
                                                      float *const *bbox_targets_out, float *const *rois_3d_out,
                                                      float *const *rois_fv_out, void *const *workspace,
                                                      const size_t *workspace_bytes, void *stream)
{
    if (!num_rois_dev) return MV3D_ERR_INVALID_ARG;
    return pt_stage2_batch(batch, rois_bv_dev, rois_3d_dev, num_rois_cap, num_rois_dev, PT_S2_ARGS);
}
#undef PT_S2_ARGS

extern "C" int mv3d_proposal_target_stage2(const float *rois_bv_dev, const float *rois_3d_dev, int num_rois,
                                           const float *gt_bv_dev, const float *gt_3d_dev,
                                           const float *gt_corners_dev, int G, const float *calib_dev,
                                           const mv3d_proposal_target_params *p, const int32_t *fg_pick_dev, int n_fg,
                                           const int32_t *bg_pick_dev, int n_bg, float *rois_bv_out, float *rois_img_out,
                                           int32_t *labels_out, float *bbox_targets_out, float *rois_3d_out,
                                           void *workspace, size_t workspace_bytes, void *stream)
{
    if (!p) return MV3D_ERR_INVALID_ARG;
    return mv3d_proposal_target_stage2_batch(1, &rois_bv_dev, &rois_3d_dev, &num_rois, &gt_bv_dev, &gt_3d_dev, &gt_corners_dev, &G,
                                             &calib_dev, p, &fg_pick_dev, &n_fg, &bg_pick_dev, &n_bg, &rois_bv_out, &rois_img_out,
                                             &labels_out, &bbox_targets_out, &rois_3d_out, nullptr, &workspace, &workspace_bytes, stream);
}
