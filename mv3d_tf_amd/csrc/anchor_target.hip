// anchor_target_layer for gfx950 (one frame): lib/rpn_msr/anchor_target_layer_tf.py:21-250
// with lib/utils/bbox.pyx:15-55 (IoU, f64) and lib/fast_rcnn/bbox_transform.py:32-58 fused in;
// the N x G overlap matrix is never materialised.  The anchor grid, the BEV -> 3D anchor arithmetic,
// the overlap and the ground-truth staging are geometry.h's (shared with proposal.hip / proposal_target.hip).
//
//  at_overlap_kernel   per anchor: inside test, f64 IoU against the G ground-truth boxes staged
//                      in LDS, first-argmax / max per anchor, per-GT column maximum of the workgroup's
//                      256 anchors (u64 atomicMax in LDS on the bit pattern of the non-negative f64),
//                      stored as one partial per (GT, workgroup): no global atomics, so nothing in the
//                      workspace has to be zero on entry (the look-back words of the two compactions
//                      are cleared by this launch as well) -- stage 1 is three launches and no memset.
//  at_label_kernel     labels before any random subsampling (incl. the "every anchor tying a
//                      GT's column max" flood) and the 6-d targets, written straight
//                      into the full-grid (unmapped) outputs: -1 / 0 fill for outside anchors.
//  at_compact_kernel   one workgroup: ordered (ascending anchor index) compaction of the three
//                      lists the reference subsamples from + their counts.
//  stage 2             applies the host-drawn permutations (numpy MT19937 draws stay on the host:
//                      draw-for-draw parity) and emits the debug anchor lists.
#include <math.h>
#include "anchor_target.h"

// Stage 1 (bodies: anchor_target.h)
__global__ __launch_bounds__(256) void at_overlap_kernel(AtBatch bt) { at_overlap_body(bt.f[blockIdx.y], bt.n_agg1, bt.n_agg2, blockIdx.x); }
__global__ __launch_bounds__(256) void at_label_kernel(AtBatch bt) { at_label_body(bt.f[blockIdx.y], blockIdx.x); }
__global__ __launch_bounds__(256) void at_compact_kernel(AtBatch bt) { at_compact_body(bt.f[blockIdx.y], blockIdx.x, gridDim.x); }

// Stage 2 (bodies: anchor_target.h)
__global__ __launch_bounds__(256) void at_disable_all_kernel(AtBatch bt) { at_disable_all_body(bt.f[blockIdx.y], blockIdx.x, gridDim.x); }

__global__ __launch_bounds__(256) void at_emit_relabel_kernel(AtBatch bt)
{
    const AtFrame &F = bt.f[blockIdx.y];
    at_emit_relabel_body(at_emit_frame(F), at_emit_grid(F, bt.cap), blockIdx.x, gridDim.x);
}

// ------------------------------------------------------------------------ workspace / C-ABI
extern "C" size_t mv3d_anchor_target_workspace_bytes(int H, int W, int G)
{
    AtLayout L;
    return at_layout(H, W, G, L) ? L.total : 0;
}

extern "C" int mv3d_anchor_target_stage1_batch_masked(int batch, int H, int W, const float *im_info_dev,
                                                      const float *const *gt_bv_dev, const float *const *gt_3d_dev, const int *G,
                                                      const mv3d_anchor_target_params *p, const uint8_t *const *anchor_mask_dev,
                                                      float *labels_dev, float *targets_dev, int32_t *const *counts_dev,
                                                      uint8_t *const *fg_hi_dev, void *const *workspace, size_t workspace_bytes,
                                                      void *stream)
{
    AtBatch bt;
    AtLayout L;
    const int rc = at_stage1_args(batch, H, W, im_info_dev, gt_bv_dev, gt_3d_dev, G, p, anchor_mask_dev, labels_dev, targets_dev, counts_dev,
                                  fg_hi_dev, workspace, workspace_bytes, bt, L);
    if (rc != MV3D_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = L.nblk;
    hipLaunchKernelGGL(at_overlap_kernel, dim3(blocks, batch), dim3(256), 0, s, bt);
    hipLaunchKernelGGL(at_label_kernel, dim3(blocks, batch), dim3(256), 0, s, bt);
    hipLaunchKernelGGL(at_compact_kernel, dim3(L.ncwg, batch), dim3(256), 0, s, bt);
    return mv3d_launch_status();
}

extern "C" int mv3d_anchor_target_stage1_batch(int batch, int H, int W, const float *im_info_dev, const float *const *gt_bv_dev,
                                               const float *const *gt_3d_dev, const int *G, const mv3d_anchor_target_params *p,
                                               float *labels_dev, float *targets_dev, int32_t *const *counts_dev,
                                               uint8_t *const *fg_hi_dev, void *const *workspace, size_t workspace_bytes,
                                               void *stream)
{
    return mv3d_anchor_target_stage1_batch_masked(batch, H, W, im_info_dev, gt_bv_dev, gt_3d_dev, G, p, nullptr, labels_dev, targets_dev,
                                                  counts_dev, fg_hi_dev, workspace, workspace_bytes, stream);
}

extern "C" int mv3d_anchor_target_stage1(int H, int W, const float *im_info_dev, const float *gt_bv_dev,
                                         const float *gt_3d_dev, int G, const mv3d_anchor_target_params *p,
                                         float *labels_dev, float *targets_dev, int32_t *counts_dev, uint8_t *fg_hi_dev,
                                         void *workspace, size_t workspace_bytes, void *stream)
{
    return mv3d_anchor_target_stage1_batch(1, H, W, im_info_dev, &gt_bv_dev, &gt_3d_dev, &G, p, labels_dev, targets_dev,
                                           &counts_dev, &fg_hi_dev, &workspace, workspace_bytes, stream);
}

extern "C" int mv3d_anchor_target_stage2_batch(int batch, int H, int W, const mv3d_anchor_target_params *p,
                                               const int32_t *const *disable_fg_dev, const int *n_dis_fg,
                                               const int32_t *const *disable_bg1_dev, const int *n_dis_bg1,
                                               const int32_t *const *disable_bg2_dev, const int *n_dis_bg2, float *labels_dev,
                                               float *anchors_dev, float *anchors_3d_dev, int32_t *n_anchors_dev,
                                               int anchors_cap, void *const *workspace, size_t workspace_bytes, void *stream)
{
    AtBatch bt;
    AtLayout L;
    int most;
    const int rc = at_stage2_args(batch, H, W, p, disable_fg_dev, n_dis_fg, disable_bg1_dev, n_dis_bg1, disable_bg2_dev, n_dis_bg2, labels_dev,
                                  anchors_dev, anchors_3d_dev, n_anchors_dev, anchors_cap, workspace, workspace_bytes, bt, L, most);
    if (rc != MV3D_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (most > 0) hipLaunchKernelGGL(at_disable_all_kernel, dim3((most + 255) / 256, batch), dim3(256), 0, s, bt);
    hipLaunchKernelGGL(at_emit_relabel_kernel, dim3(L.ncwg, batch), dim3(256), 0, s, bt);
    return mv3d_launch_status();
}

extern "C" int mv3d_anchor_target_stage2(int H, int W, const mv3d_anchor_target_params *p,
                                         const int32_t *disable_fg_dev, int n_dis_fg, const int32_t *disable_bg1_dev,
                                         int n_dis_bg1, const int32_t *disable_bg2_dev, int n_dis_bg2, float *labels_dev,
                                         float *anchors_dev, float *anchors_3d_dev, int32_t *n_anchors_dev,
                                         int anchors_cap, void *workspace, size_t workspace_bytes, void *stream)
{
    return mv3d_anchor_target_stage2_batch(1, H, W, p, &disable_fg_dev, &n_dis_fg, &disable_bg1_dev, &n_dis_bg1, &disable_bg2_dev,
                                           &n_dis_bg2, labels_dev, anchors_dev, anchors_3d_dev, n_anchors_dev, anchors_cap,
                                           &workspace, workspace_bytes, stream);
}
