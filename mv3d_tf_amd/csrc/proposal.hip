// proposal_layer_3d for gfx950: lib/rpn_msr/proposal_layer_tf.py:25-202 behind one C-ABI call.
//
//   proposal_decode_kernel  one thread per anchor (h,w,a): anchor -> 3D anchor (f64,
//        lib/utils/transform.py:89-111) -> decoded 3D box (f32, numpy's f32 exp restated;
//        lib/fast_rcnn/bbox_transform.py:108-155) -> BEV pixel box (f64 floor-divide,
//        transform.py:113-142) -> 8 corners (transform.py:290-315) -> image box (f32 matrix,
//        f64 product, trunc to i32; transform.py:483-500,369-386) -> clip + both filters
//        (bbox_transform.py:178-191, proposal_layer_tf.py:336-352).  Nothing but the final
//        candidate record (BEV box, image box, 3D box, score key) is written: the ~25 numpy
//        temporaries of the reference never exist.  Reads are the two NHWC head tensors,
//        consecutive anchors = consecutive addresses.
//   rank_kernel (rank.hip)   argsort()[::-1][:pre_nms_topN]
//   nms_mask/reduce (nms.hip) greedy NMS on the sorted candidates, capped at post_nms_topN
//   (ROI blobs)              gathered by the tail of the NMS reduce kernel, unused rows zero-filled.
//
// All shapes are static given (H, W, params); data-dependent counts stay on the device, so
// the whole call is capturable in a hipGraph.
#include "proposal.h"

__global__ __launch_bounds__(DEC_THREADS) void proposal_decode_kernel(ProposalDev d) { proposal_decode_body(d, blockIdx.y, blockIdx.x, gridDim.x); }

extern "C" int mv3d_proposal_3d_capacity(int H, int W, const mv3d_proposal_params *p)
{
    ProposalLayout L;
    return proposal_layout(1, H, W, p, L) ? L.cap : -1;
}

extern "C" size_t mv3d_proposal_3d_workspace_bytes(int batch, int H, int W, const mv3d_proposal_params *p)
{
    ProposalLayout L;
    return proposal_layout(batch, H, W, p, L) ? L.total : 0;
}

extern "C" int mv3d_proposal_3d_masked(const float *prob_dev, const float *pred_dev, int batch, int H, int W,
                                       const float *im_info_dev, const float *calib_dev, const mv3d_proposal_params *p,
                                       const uint8_t *anchor_mask_dev, float *blob_bv_dev, float *blob_img_dev,
                                       float *blob_3d_dev, int32_t *num_out_dev, int32_t *status_dev, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    ProposalLayout L;
    if (!proposal_layout(batch, H, W, p, L)) return MV3D_ERR_INVALID_ARG;
    if (!prob_dev || !pred_dev || !im_info_dev || !calib_dev || !blob_bv_dev || !blob_img_dev || !blob_3d_dev ||
        !num_out_dev || p->feat_stride <= 0)
        return MV3D_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < L.total || ((uintptr_t)workspace % MV3D_ALIGN)) return MV3D_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    ProposalDev d;
    NmsLaunch nl;
    proposal_launch_args(L, prob_dev, pred_dev, batch, H, W, im_info_dev, calib_dev, p, anchor_mask_dev, blob_bv_dev, blob_img_dev, blob_3d_dev,
                         num_out_dev, status_dev, ws, d, nl);
    hipLaunchKernelGGL(proposal_decode_kernel, dim3(L.n_blocks, batch), dim3(DEC_THREADS), 0, s, d);
    int rc = mv3d_launch_rank(d.key, L.N, L.key_stride, batch, (int32_t *)nl.emit.order, L.order_cap, d.blockcnt, L.n_blocks, (int32_t *)nl.n_dev,
                              ws + L.o_rank, s, d.bv, (float4 *)nl.boxes);
    if (rc != MV3D_OK) return rc;
    return mv3d_launch_nms(nl, s);
}

extern "C" int mv3d_proposal_3d(const float *prob_dev, const float *pred_dev, int batch, int H, int W,
                                const float *im_info_dev, const float *calib_dev, const mv3d_proposal_params *p,
                                float *blob_bv_dev, float *blob_img_dev, float *blob_3d_dev, int32_t *num_out_dev,
                                int32_t *status_dev, void *workspace, size_t workspace_bytes, void *stream)
{
    return mv3d_proposal_3d_masked(prob_dev, pred_dev, batch, H, W, im_info_dev, calib_dev, p, nullptr, blob_bv_dev, blob_img_dev,
                                   blob_3d_dev, num_out_dev, status_dev, workspace, workspace_bytes, stream);
}
