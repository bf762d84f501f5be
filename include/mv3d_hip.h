/*
 * mv3d_hip.h -- C-ABI of libmv3d_hip.so, the MI355X (gfx950) implementation of the
 * MV3D RPN -> ROI-pool -> NMS hot path.
 *
 * Drop-in boundary: every entry point below replaces one native or
 * numpy interface of the reference (cited per function, paths relative to the upstream
 * repository root).  Plain C: raw device pointers, sizes, an opaque stream handle
 * (a hipStream_t passed as void*; NULL = the null stream).  No torch types, no
 * exceptions, no exit(): every call returns an mv3d_status.  Hot calls never allocate:
 * the caller owns outputs and a workspace whose size the *_workspace_bytes() queries
 * return.  All calls are asynchronous on `stream` unless stated otherwise and are
 * re-entrant per (stream, workspace).
 *
 * Frames are an outer, independent dimension (`batch`): the reference asserts batch==1
 * in its RPN layers (lib/rpn_msr/proposal_layer_tf.py:48-49); here frame b of a batch
 * gives exactly what the reference gives for that frame alone, with ROI column 0 = b.
 */
#ifndef MV3D_HIP_H
#define MV3D_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    MV3D_OK = 0,
    MV3D_ERR_INVALID_ARG = 1,   /* bad shape / NULL pointer / unsupported size */
    MV3D_ERR_WORKSPACE = 2,     /* workspace too small or misaligned (256 B) */
    MV3D_ERR_HIP = 3,           /* a HIP runtime call or launch failed */
    MV3D_ERR_ZERO_DIVISION = 4  /* host entries only: the reference's ZeroDivisionError */
} mv3d_status;

int mv3d_version(void);                      /* 100 * major + minor */
const char *mv3d_status_string(int status);

/* ------------------------------------------------------------------ NMS
 * Replaces: lib/nms/cpu_nms.pyx:17-68 (== lib/utils/nms.pyx:17-68), dispatcher
 * lib/fast_rcnn/nms_wrapper.py:13-21, and the CUDA path lib/nms/nms_kernel.cu:34-144 /
 * lib/nms/gpu_nms.hpp:1-2.
 *
 * Semantics (CPU path = the parity target): f32 IoU with the +1 pixel convention,
 * separate IEEE f32 operations, box j suppressed by an earlier kept box iff
 * (double)IoU >= thresh.  The device-status word receives bit 0 = "a union was 0"
 * (the reference raises ZeroDivisionError there; the pair is treated as not
 * suppressing and the flag is raised). */

/* Device entry: dets_dev (n,5) f32 [x1,y1,x2,y2,score], ALREADY in processing order
 * (descending score).  keep_dev receives positions 0..n-1 of the kept boxes in order,
 * at most max_keep of them (max_keep <= 0: no cap; the result equals the reference's
 * keep[:max_keep]); num_keep_dev[0] the count; status_dev (may be NULL): flag bits are OR-ed into
 * status_dev[0], which the caller zeroes once when it allocates it (the call is kernel launches only:
 * no memset node, so it can be captured in a hipGraph and replayed). */
size_t mv3d_nms_workspace_bytes(int max_boxes);
int mv3d_nms_device(const float *dets_dev, int n, double thresh, int max_keep,
                    int32_t *keep_dev, int32_t *num_keep_dev, int32_t *status_dev,
                    void *workspace, size_t workspace_bytes, void *stream);

/* Host only (no device, no environment): the rounds every NMS launch of num_boxes boxes capped at max_keep runs -- the launcher
 * walks this very plan.  rounds_out receives up to 7 triples (b0, b1, width): the round covers the 64-box column blocks
 * [b0, b1); width 0 = round 1 (the tiles kernel + the LDS chain), else the later round's kernel width (32, 64 or 128 blocks).
 * Returns the number of rounds (num_boxes == 0: the one round (0, 0)), or 0 for a count that the launches refuse
 * (negative, above 32768) or a NULL rounds_out. */
int mv3d_nms_round_plan(int num_boxes, int max_keep, int32_t *rounds_out);

/* Diagnostics: mv3d_nms_device plus a per-64-box-block trace of the greedy chain,
 * trace_dev[4*b + 0..3] = {cycle at block start, cycle after waiting for the bulk workers,
 * cycle after the diagonal fixed point, (iterations << 32) | kept-in-block}, followed by 8
 * phase stamps of the first round's chain kernel {start, first tiles in LDS, chain done, end};
 * trace_dev holds 4*ceil(n/64) + 8 entries.  Used by tools/ and profiles/ only. */
int mv3d_nms_device_trace(const float *dets_dev, int n, double thresh, int max_keep,
                          int32_t *keep_dev, int32_t *num_keep_dev, int32_t *status_dev,
                          void *workspace, size_t workspace_bytes, void *stream, int64_t *trace_dev);

/* Host entry with cpu_nms(dets, thresh) semantics: host pointers, dets unsorted;
 * sorts on the device (descending score, ties by descending index -- the reference
 * leaves ties to numpy's unstable argsort), runs the NMS, returns indices into dets in
 * processing order.  Synchronous; allocates and frees its own device buffers (like
 * _nms below).  Returns MV3D_ERR_ZERO_DIVISION where the reference raises. */
int mv3d_nms_host(int32_t *keep_out, int32_t *num_out, const float *dets_host, int n,
                  double thresh, int device_id);

/* Symbol-compatible replacement for lib/nms/gpu_nms.hpp:1-2 (bound by gpu_nms.pyx:13-14):
 * host pointers, boxes pre-sorted by the caller, synchronous, selects device_id.  Keeps
 * the CUDA path's own rule (nms_kernel.cu:71): suppressed iff IoU > thresh compared in
 * f32 -- NOT identical to the CPU path; parity of this entry is
 * unpinned (no CUDA device to run the original on). */
void _nms(int *keep_out, int *num_out, const float *boxes_host, int boxes_num,
          int boxes_dim, float nms_overlap_thresh, int device_id);

/* ------------------------------------------------------------------ proposal_layer_3d
 * Replaces the numpy py_func body lib/rpn_msr/proposal_layer_tf.py:25-202 and all it
 * calls (bv_anchor_to_lidar, bbox_transform_inv_3d, lidar_3d_to_bv, lidar_3d_to_corners,
 * lidar_cnr_to_img, clip_boxes, _filter_boxes, _filter_img_boxes, argsort top-N, nms).
 *   prob_dev    (batch,H,W,8)  f32  rpn_cls_prob_reshape, channel 2a = bg, 2a+1 = fg
 *   pred_dev    (batch,H,W,24) f32  rpn_bbox_pred, channels 6a..6a+5
 *   im_info_dev (batch,3)      f32  [H_bev, W_bev, scale]
 *   calib_dev   (batch,4,12)   f32  rows P2, P3, R0(9)+000, Tr_velo_to_cam
 * Outputs, row capacity cap = mv3d_proposal_3d_capacity(): blob_bv (batch,cap,5),
 * blob_img (batch,cap,5), blob_3d (batch,cap,7), rows >= num_out[b] zero-filled;
 * num_out_dev (batch) i32; status_dev (batch) i32 flag bits as for the NMS (may be NULL). */
typedef struct {
    int32_t feat_stride;     /* 8: lib/networks/MV3D_train.py:5 */
    int32_t pre_nms_topN;    /* cfg[key].RPN_PRE_NMS_TOP_N  (<=0: keep all) */
    int32_t post_nms_topN;   /* cfg[key].RPN_POST_NMS_TOP_N (<=0: keep all) */
    int32_t img_height;      /* 375  hard-coded at proposal_layer_tf.py:147 */
    int32_t img_width;       /* 1242 */
    int32_t img_padding;     /* 50: proposal_layer_tf.py:345 */
    int32_t nms_strict_gt;   /* 0: cpu_nms rule, (double)IoU >= thresh (cfg.USE_GPU_NMS False, the parity target);
                                1: gpu_nms rule, IoU > thresh in f32 (what nms_wrapper.py:19-20 picks when USE_GPU_NMS) */
    int32_t reserved0;
    double nms_thresh;       /* cfg[key].RPN_NMS_THRESH */
    double min_size;         /* cfg[key].RPN_MIN_SIZE   */
} mv3d_proposal_params;

int mv3d_proposal_3d_capacity(int H, int W, const mv3d_proposal_params *p);
size_t mv3d_proposal_3d_workspace_bytes(int batch, int H, int W, const mv3d_proposal_params *p);
int mv3d_proposal_3d(const float *prob_dev, const float *pred_dev, int batch, int H, int W,
                     const float *im_info_dev, const float *calib_dev,
                     const mv3d_proposal_params *p,
                     float *blob_bv_dev, float *blob_img_dev, float *blob_3d_dev,
                     int32_t *num_out_dev, int32_t *status_dev,
                     void *workspace, size_t workspace_bytes, void *stream);
/* mv3d_proposal_3d with the empty anchors taken out (mv3d_anchor_occupancy below): anchor_mask_dev (batch,N) u8, N = 4 H W, anchor
 * order (h,w,a).  An anchor whose mask is 0 fails the filter exactly like one that fails _filter_boxes: its key is 0, it is not
 * counted, ranked or emitted.  Nothing else changes (capacity, workspace size, status words).  NULL: every anchor takes part --
 * mv3d_proposal_3d is this entry with a NULL mask. */
int mv3d_proposal_3d_masked(const float *prob_dev, const float *pred_dev, int batch, int H, int W,
                            const float *im_info_dev, const float *calib_dev,
                            const mv3d_proposal_params *p, const uint8_t *anchor_mask_dev,
                            float *blob_bv_dev, float *blob_img_dev, float *blob_3d_dev,
                            int32_t *num_out_dev, int32_t *status_dev,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ empty anchors (MV3D paper, section 3.2; not in the reference)
 * "Since LIDAR point cloud is sparse, which results in many empty anchors, we remove all the empty anchors during both training
 * and testing to reduce computation."  The rule, for a BEV map bev_dev (batch,map_h,map_w,channels) f32 NHWC:
 *   occupancy  cell (y,x) of a frame is OCCUPIED iff at least one of its channels satisfies !(v == 0.0f): -0.0f is empty, NaN and
 *              subnormals are occupied.
 *   count      anchor n = (h,w,a), a fastest, of the H x W grid at feat_stride is the integer pixel box x1,y1,x2,y2 of the proposal
 *              layer / anchor target layer (base anchor a shifted by (w,h) * feat_stride), corners inclusive; count[n] = number of
 *              occupied cells in the intersection of [x1,x2] x [y1,y2] with [0,map_w-1] x [0,map_h-1]; an empty intersection: 0.
 *   mask       mask[n] = count[n] >= min_cells (min_cells >= 1).  Counts are exact int32.
 * mask_dev (batch,4 H W) u8 0 / 1; count_dev (batch,4 H W) i32 or NULL.  Two kernel launches; no allocation, memset,
 * synchronisation or host read (capturable in a graph); the workspace (256-byte aligned, at least
 * mv3d_anchor_occupancy_workspace_bytes(), 0 for unsupported sizes) needs no initialisation.  MV3D_ERR_INVALID_ARG before any HIP
 * call: a NULL pointer (count_dev excepted), batch outside 1..65535, map_h or map_w outside 1..4096, channels outside 1..64,
 * feat_stride < 1, min_cells < 1, H or W < 1, 4 H W > 65536 (the proposal layer's limit), bev_dev not 4-byte aligned, or a grid
 * whose last anchor leaves int32 ((max(H,W) - 1) * feat_stride + 20 > INT32_MAX).  MV3D_ERR_WORKSPACE as elsewhere. */
size_t mv3d_anchor_occupancy_workspace_bytes(int batch, int map_h, int map_w);
int mv3d_anchor_occupancy(const float *bev_dev, int batch, int map_h, int map_w, int channels,
                          int H, int W, int feat_stride, int min_cells,
                          uint8_t *mask_dev, int32_t *count_dev,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ RoiPool / RoiPoolGrad
 * Replace lib/roi_pooling_layer/roi_pooling_op_gpu.h:18-27 (ROIPoolForwardLaucher /
 * ROIPoolBackwardLaucher, bodies roi_pooling_op_gpu.cu.cc:20-110,113-215) and the CPU
 * kernels roi_pooling_op.cc:74-190,319-452: the launchers' argument lists with a stream
 * handle where the reference takes `const Eigen::GpuDevice&` and a status instead of
 * exit(-1).  ONE DELIBERATE DEVIATION from roi_pooling_op_gpu.h:18-22: the forward takes
 * `batch_size` after `spatial_scale` (the reference's forward launcher has no such argument;
 * its backward launcher has it in the same place), see below.
 * NHWC f32 data, rois (R,5) [batch_idx,x1,y1,x2,y2], argmax = flat index inside the
 * frame (h*W+w)*C+c or -1; argmax_data may be NULL on forward.  `batch_size` lets the
 * kernel refuse out-of-range batch indices (outputs 0 / -1) instead of reading out of
 * bounds as the reference would.  Backward is the reference's deterministic gather
 * (ROIs ascending, then ph, pw ascending): bit-identical f32 sums, no atomics. */
int mv3d_roi_pool_forward(const float *bottom_data, float spatial_scale, int batch_size,
                          int num_rois, int height, int width, int channels,
                          int pooled_height, int pooled_width, const float *bottom_rois,
                          float *top_data, int32_t *argmax_data, void *stream);
int mv3d_roi_pool_backward(const float *top_diff, float spatial_scale, int batch_size,
                           int num_rois, int height, int width, int channels,
                           int pooled_height, int pooled_width, const float *bottom_rois,
                           float *bottom_diff, const int32_t *argmax_data, void *stream);

/* Several views in one launch (e.g. the BEV and RGB RoiPool layers of one step, MV3D_test.py:95-107):
 * same results as one mv3d_roi_pool_forward per view. */
#define MV3D_MAX_ROI_VIEWS 4
typedef struct {
    const float *bottom_data;    /* (batch_size, height, width, channels) NHWC */
    const float *bottom_rois;    /* (num_rois, 5) */
    float *top_data;             /* (num_rois, pooled_height, pooled_width, channels) */
    int32_t *argmax_data;        /* same shape, may be NULL */
    float spatial_scale;
    int32_t batch_size, num_rois, height, width, channels;
} mv3d_roi_view;
int mv3d_roi_pool_forward_views(int num_views, const mv3d_roi_view *views, int pooled_height, int pooled_width,
                                void *stream);
/* The same call for maps that are NOT cache-resident (inputs written long ago, e.g. a ring of resident batches): prefetch
 * workgroups at the front of the same launch stream the map pixels the ROIs cover into the memory-side cache ahead of the
 * pooling workgroups (58 -> 40 us on the training batch of bench.py).  Same results; pointless -- a few us slower -- when the
 * maps were just produced by the previous layer.  (No counterpart in the reference.) */
int mv3d_roi_pool_forward_views_cold(int num_views, const mv3d_roi_view *views, int pooled_height, int pooled_width,
                                     void *stream);
/* Inference in 16-bit mode: the same pooling with `top_data` written as f16 (top_type 1) or bf16 (top_type 2) -- exactly the values a
 * cast of the f32 output gives (the maximum is taken in f32, then rounded once), without the f32 output and without the cast launch in
 * front of the head's first GEMM.  Every view's argmax_data must be NULL and the shapes must be the XCD-sliced kernels'
 * (C in {256, 512, 1024}, 16-byte aligned buffers): INVALID_ARG otherwise.  (No counterpart in the reference: its op is f32.) */
int mv3d_roi_pool_forward_views_half(int num_views, const mv3d_roi_view *views, int pooled_height, int pooled_width,
                                     int top_type, int cold_maps, void *stream);

/* RoiPoolGrad of several views behind one call (the three RoiPool layers of a training step): same results as
 * one mv3d_roi_pool_backward per view.  In a backward view `top_data` is READ (top_diff, (num_rois,PH,PW,C)),
 * `argmax_data` is read and `bottom_data` is WRITTEN (bottom_diff, (batch_size,H,W,C)); the struct is shared with the
 * forward so that a caller fills it once per layer. */
typedef struct {
    float *bottom_diff;          /* out: (batch_size, height, width, channels) */
    const float *bottom_rois;    /* (num_rois, 5) */
    const float *top_diff;       /* (num_rois, pooled_height, pooled_width, channels) */
    const int32_t *argmax_data;  /* same shape */
    float spatial_scale;
    int32_t batch_size, num_rois, height, width, channels;
} mv3d_roi_grad_view;
size_t mv3d_roi_pool_backward_workspace_bytes(int num_views, const mv3d_roi_grad_view *views, int pooled_height,
                                              int pooled_width);
/* workspace (optional, 256-B aligned): with at least mv3d_roi_pool_backward_workspace_bytes() bytes the call runs as three
 * launches -- per-pixel candidate index (sizes, then lists), then a gather that reads every (roi, bin) record slice on one
 * XCD -- which is the fast path for ANY argmax plane (same C for all views, C in {64, 128, 256, 512}, pooled sizes <= 15,
 * 16-byte aligned buffers).
 * The workspace needs no initialisation (every word is written before it is read).  With workspace == NULL the call needs
 * no scratch memory and is slower (one launch, XCD-sliced, geometry recomputed per slice). */
int mv3d_roi_pool_backward_views(int num_views, const mv3d_roi_grad_view *views, int pooled_height, int pooled_width,
                                 void *workspace, size_t workspace_bytes, void *stream);
/* Host only (no device, no environment): the name of the body that runs such a RoiPoolGrad call -- mv3d_roi_pool_backward,
 * mv3d_roi_pool_backward_views and mv3d_roi_pool_backward_views_pair launch what this very selection returns, and the pair's forward
 * and decode ask it whether the argmax plane holds compact codes.  have_workspace != 0: a workspace of at least
 * mv3d_roi_pool_backward_workspace_bytes() bytes is given (a shorter one counts as none); pair != 0: the call goes through the pair's
 * entries.  Pointers in `views` may be NULL, as for the size queries; the alignment conditions apply where they are given.
 *   "generic"   any view outside the sliced kernel's shapes (C no multiple of 64 or > 4096, PH * PW > 512, a pooled size > 255,
 *               2^26 pixels or more): one launch per view, C <= 4096 (16-byte aligned buffers, C % 4 == 0) or <= 1024
 *   "sliced"    one launch, 64-channel slices, no scratch memory
 *   "indexed"   index + gather (three launches): have_workspace, same C in {64, 128, 256, 512} for all views, pooled sizes <= 15,
 *               16-byte aligned buffers
 *   "tiles"     the pair's LDS map tiles: pair, the indexed conditions, C in {256, 512}, every view with at least one ROI and a map of
 *               at most 65534 pixels
 * A static string, or NULL where the entries return MV3D_ERR_INVALID_ARG for the shapes. */
const char *mv3d_roi_pool_backward_path(int num_views, const mv3d_roi_grad_view *views, int pooled_height, int pooled_width,
                                        int have_workspace, int pair);

/* The PAIR: RoiPool and RoiPoolGrad of a training step with a PRIVATE argmax plane between them (the fast training path).
 * `top_data` and `bottom_diff` are bit-identical to mv3d_roi_pool_forward_views / mv3d_roi_pool_backward_views.
 *   argmax_data     (required) belongs to the pair: the forward writes it, the backward reads it, nobody else needs it (the
 *                   reference's own graph uses the op's second output only in RoiPoolGrad, roi_pooling_op_grad.py:7-43).  The
 *                   pair's kernels store it as ONE-BYTE codes -- the position of the first maximum in its bin's scan order
 *                   (h - hstart) * (wend - wstart) + (w - wstart), 0xFF for the reference's -1 -- in the first quarter of the
 *                   caller's (num_rois, PH, PW, C) int32 buffer (bins of more than 255 pixels, i.e. ROIs far larger than the
 *                   map: 16-bit codes in the two quarters behind it): 3 / 8 of the record bytes (8 -> 5 B per pooled value)
 *                   are neither written by the forward nor read by the backward.  The LAST quarter of view 0's buffer carries the
 *                   backward's work list (a few KB): one planning workgroup at the front of the forward launch estimates every map
 *                   tile's entry stream from the ROIs, cuts the tiles under long streams into four sub-tiles (first in the list: a
 *                   stream is one wave's serial work and the launch's makespan) and flags the tiles no ROI touches (written as
 *                   zeros without a ROI filter).  Both launches decide from the shapes alone whether the list exists (<= 3072 tiles
 *                   in all views, the list fits the quarter; otherwise the static tile grid).  mv3d_roi_pool_argmax_decode returns
 *                   the reference's int32 plane (tests, verification).
 *   backward        ONE launch (csrc/roi_grad_tiles.hip): a wave owns a unit of the work list -- a tile of <= 16 map pixels x 64
 *                   channels in LDS, or a sub-tile of a cut one (a single pixel keeps its sum in a register) --, finds the ROIs that
 *                   reach it, streams their (roi, bin) records in the reference's order (roi_pooling_op.cc:392-431) and routes every
 *                   value to the pixel its code names; a unit is written out whole (no index, no fill, no scratch memory).  The
 *                   views must be the forward's (same order, shapes, scale, ROIs) with the argmax buffers it wrote.  (For a
 *                   foreign argmax plane use mv3d_roi_pool_backward_views: int32 argmax.)
 *   workspace       optional (NULL, 0: none); the pair's own kernels never read it.  Checked for alignment and handed on to
 *                   mv3d_roi_pool_backward_views for shapes outside the pair's kernels: the plain layout, so
 *                   mv3d_roi_pool_pair_workspace_bytes returns exactly mv3d_roi_pool_backward_workspace_bytes.
 *   cold_maps       != 0: as mv3d_roi_pool_forward_views_cold.
 * Shapes outside the pair's kernels (C not in {256, 512} / not the same for all views, pooled sizes > 15, a map of more than 65534
 * pixels, an empty view) take the plain forward (int32 argmax) and mv3d_roi_pool_backward_views behind the same entries.
 * (Measured and dropped, round 5: the candidate index built by workgroups inside the FORWARD launch, and a single-pass index with
 * an in-launch look-back -- profiles/EXPERIMENTS.md, round 5.) */
size_t mv3d_roi_pool_pair_workspace_bytes(int num_views, const mv3d_roi_grad_view *views, int pooled_height, int pooled_width);
int mv3d_roi_pool_forward_views_pair(int num_views, const mv3d_roi_view *views, int pooled_height, int pooled_width,
                                     int cold_maps, void *stream);
int mv3d_roi_pool_backward_views_pair(int num_views, const mv3d_roi_grad_view *views, int pooled_height, int pooled_width,
                                      void *workspace, size_t workspace_bytes, void *stream);
/* views: as passed to mv3d_roi_pool_forward_views_pair (after it ran); argmax_out[k]: (num_rois, PH, PW, C) int32, a buffer of its
 * own: the reference's argmax plane of view k (flat index inside the frame, -1 for an empty bin). */
int mv3d_roi_pool_argmax_decode(int num_views, const mv3d_roi_view *views, int pooled_height, int pooled_width,
                                int32_t *const *argmax_out, void *stream);

/* Call-compatible aliases of the reference's two launchers (roi_pooling_op_gpu.h:18-27): EXACTLY their argument order -- the
 * forward WITHOUT a batch size (out-of-range batch indices are then the caller's problem, as in the reference) -- with `void *stream`
 * where the reference passes `const Eigen::GpuDevice &d` (a maintainer's call site passes `d.stream()`), returning `bool`-like
 * 1 on success and 0 on failure where the reference returns d.ok().  For a port of roi_pooling_op.cc:250-287 / :505-554 that
 * keeps its call sites untouched. */
int mv3d_ROIPoolForwardLaucher(const float *bottom_data, float spatial_scale, int num_rois, int height, int width, int channels,
                               int pooled_height, int pooled_width, const float *bottom_rois, float *top_data,
                               int32_t *argmax_data, void *stream);
int mv3d_ROIPoolBackwardLaucher(const float *top_diff, float spatial_scale, int batch_size, int num_rois, int height, int width,
                                int channels, int pooled_height, int pooled_width, const float *bottom_rois,
                                float *bottom_diff, const int32_t *argmax_data, void *stream);

/* ------------------------------------------------------------------ third (front-view) ROI
 * rois_3d_dev (R,7) [b,x,y,z,l,w,h] -> rois_fv_dev (R,5) [b,x1,y1,x2,y2] on the 64 x 512 cylindrical front-view map
 * of the MV3D paper (azimuth [-45,+45] deg -> 512 columns, elevation [-24.9,+2] deg -> 64 rows; min/max over the 8
 * corners, clipped to the map).  Fills the hook the reference leaves empty: `proposal_transform` returns None for
 * anything but 'bv' / 'img' (lib/networks/network.py:293-315).  PARITY UNPINNED (no reference code); the definition
 * is restated in oracle/mv3d_oracle.c and both agree bit for bit. */
int mv3d_rois_3d_to_fv(const float *rois_3d_dev, int num_rois, float *rois_fv_dev, void *stream);

/* ------------------------------------------------------------------ front-view input (csrc/front_view_raster.hip)
 * Velodyne points -> the (64, 512, 3) f32 map [height, distance, intensity] the third trunk reads as `lidar_fv_data`, for
 * `num_frames` clouds behind three launches (clear keys, one 64-bit atomicMin per point, resolve), whatever num_frames is.
 * PARITY UNPINNED (no reference code); a point lands on the pixel mv3d_rois_3d_to_fv gives its position (same projection).
 *   points_dev   (total_points, 4) f32 [x, y, z, reflectance], the frames' clouds concatenated, 16-byte aligned
 *   offsets_dev  (num_frames + 1) int32 ON THE DEVICE: frame b owns rows offsets[b] .. offsets[b + 1]; equal neighbours = an empty
 *                frame; rows no frame owns are ignored.  No value in it can make the call read or write out of bounds.  NULL with
 *                num_frames == 1: the one frame owns every row.
 *   fv_dev       (num_frames, 64, 512, 3) f32, 16-byte aligned: [z, d, reflectance] of the pixel's nearest point (d = the f64
 *                norm rounded once to f32; among equal d the last point), [0, 0, 0] where no point falls.  Dropped: non-finite
 *                x / y / z, x == y == 0, pixels outside the window (nothing is clipped into it).
 *   workspace    mv3d_point_cloud_2_front_workspace(num_frames) bytes (one 64-bit key per pixel), 16-byte aligned, the caller's;
 *                it needs no initialisation and holds nothing between calls.
 * No allocation, no host synchronisation; a plain chain of launches on `stream` (capturable).  MV3D_ERR_INVALID_ARG: NULL or
 * misaligned pointers, negative counts, num_frames > MV3D_FV_MAX_FRAMES (the size query then returns 0). */
#define MV3D_FV_MAX_FRAMES 1024
size_t mv3d_point_cloud_2_front_workspace(int num_frames);
int mv3d_point_cloud_2_front(const float *points_dev, const int32_t *offsets_dev, int num_frames, int total_points, float *fv_dev,
                             void *workspace_dev, void *stream);

/* ------------------------------------------------------------------ anchor_target_layer
 * Replaces the deterministic part of lib/rpn_msr/anchor_target_layer_tf.py:21-250 plus
 * lib/utils/bbox.pyx:15-55 and lib/fast_rcnn/bbox_transform.py:32-58 (one frame):
 * stage1 = inside filter, f64 IoU vs gt_boxes_bv, argmax / max, gt-argmax flood, labels
 * before any random subsampling, 6-d targets; it also compacts the three candidate
 * lists the reference subsamples from.  The draws themselves come from the caller's
 * numpy RNG (draw-for-draw parity needs the host's MT19937 stream): the caller reads
 * counts_dev, draws the permutations, and stage2 applies them.
 *   gt_bv_dev (G,5) f32, gt_3d_dev (G,7) f32, im_info_dev (3) f32.
 *   labels_dev (N) f32 in {-1,0,1}; targets_dev (N,6) f32; N = H*W*4, anchor order (h,w,a).
 *   counts_dev[8] i32: [0] n_inside, [1] n_fg (labels==1 before subsampling),
 *     [2] n_bg (labels==0 before subsampling), [3] n_low (max_overlap < NEGATIVE_OVERLAP
 *     among inside anchors), rest reserved.
 *   fg_hi_dev (N) u8: for the k-th fg candidate, 1 iff its max_overlap >= NEGATIVE_OVERLAP
 *     (lets the host know how many positives survive step 9 of SURVEY A.1).
 *   No inside anchor at all (the reference raises there, on the argmax of an empty column): every label is -1, every
 *     target 0, the four counts are 0, stage 2 emits no debug row and the caller draws nothing. */
typedef struct {
    int32_t feat_stride;
    int32_t clobber_positives;   /* cfg.TRAIN.RPN_CLOBBER_POSITIVES */
    double negative_overlap;     /* cfg.TRAIN.RPN_NEGATIVE_OVERLAP  */
    double positive_overlap;     /* cfg.TRAIN.RPN_POSITIVE_OVERLAP  */
} mv3d_anchor_target_params;

/* The workspace size grows with G; nothing in it has to be initialised (stage 1 = three launches, no memset). */
size_t mv3d_anchor_target_workspace_bytes(int H, int W, int G);
int mv3d_anchor_target_stage1(int H, int W, const float *im_info_dev, const float *gt_bv_dev,
                              const float *gt_3d_dev, int G, const mv3d_anchor_target_params *p,
                              float *labels_dev, float *targets_dev, int32_t *counts_dev,
                              uint8_t *fg_hi_dev, void *workspace, size_t workspace_bytes,
                              void *stream);
/* stage2: disable_fg_dev[n_dis_fg] = positions in the fg candidate list to set to -1,
 * disable_bg1_dev[n_dis_bg1] positions in the first bg list; then the debug outputs
 * anchors_dev (<=cap,5) / anchors_3d_dev (<=cap,7) / n_anchors_dev are taken (labels != -1),
 * labels[max_overlap < NEGATIVE_OVERLAP] = 0, and disable_bg2_dev[n_dis_bg2] positions in
 * the second bg list are set to -1 (anchor_target_layer_tf.py:146-183). */
int mv3d_anchor_target_stage2(int H, int W, const mv3d_anchor_target_params *p,
                              const int32_t *disable_fg_dev, int n_dis_fg,
                              const int32_t *disable_bg1_dev, int n_dis_bg1,
                              const int32_t *disable_bg2_dev, int n_dis_bg2,
                              float *labels_dev, float *anchors_dev, float *anchors_3d_dev,
                              int32_t *n_anchors_dev, int anchors_cap,
                              void *workspace, size_t workspace_bytes, void *stream);

/* Frames of a batch behind one launch of every kernel (the reference's layer is single-frame, lib/rpn_msr/
 * anchor_target_layer_tf.py:42-45; the per-frame entry points above are these with batch = 1).  Host-side arrays of `batch`
 * entries (device pointers / counts); labels_dev (batch,N), targets_dev (batch,N,6), im_info_dev (batch,3),
 * anchors_dev (batch,cap,5), anchors_3d_dev (batch,cap,7), n_anchors_dev (batch) are contiguous over the frames; one
 * workspace per frame, each of at least workspace_bytes = mv3d_anchor_target_workspace_bytes(H, W, max_b G[b]) bytes.
 * batch <= 16.  stage2 = two launches: the three disable lists, then debug rows + final labels.
 * ONE-SHOT CONTRACT: stage 2 CONSUMES the workspace stage 1 left (the second background draw marks its anchors in the
 * workspace's argmax array, the list look-back words are only cleared by stage 1's overlap launch): exactly one stage-2 call
 * per stage-1 call on a workspace; to apply other disable lists, run stage 1 again.  (Same for the per-frame entries.) */
int mv3d_anchor_target_stage1_batch(int batch, int H, int W, const float *im_info_dev, const float *const *gt_bv_dev,
                                    const float *const *gt_3d_dev, const int *G, const mv3d_anchor_target_params *p,
                                    float *labels_dev, float *targets_dev, int32_t *const *counts_dev,
                                    uint8_t *const *fg_hi_dev, void *const *workspace, size_t workspace_bytes, void *stream);
/* stage 1 with the empty anchors taken out: anchor_mask_dev is a host array of `batch` device pointers to (N) u8 masks
 * (mv3d_anchor_occupancy); an entry, or the array itself, may be NULL (= no mask for that frame).  An anchor whose mask is 0 is
 * treated as OUTSIDE the image (the mask extends inds_inside of anchor_target_layer_tf.py:93-98): label -1, target 0, max_overlap
 * -1, in no candidate list and no count, and no part of a ground-truth box's column maximum -- the "every anchor tying the column
 * max" flood moves to the best non-empty anchor.  A ground-truth box ALL of whose overlapping inside anchors are masked (a car
 * with no return under it) is left with a column maximum of 0, and then, as in the reference when a box lies outside every
 * inside anchor, every surviving anchor whose overlap with it is 0 -- nearly all of them -- ties that maximum and
 * is labelled positive before the subsampling.  That is the reference's rule applied to the reduced anchor set, kept as it is;
 * a caller that turns the mask on should drop such boxes from gt first if it does not want the flood.  Stage 2 is unchanged.
 * mv3d_anchor_target_stage1_batch is this entry with a NULL array. */
int mv3d_anchor_target_stage1_batch_masked(int batch, int H, int W, const float *im_info_dev, const float *const *gt_bv_dev,
                                           const float *const *gt_3d_dev, const int *G, const mv3d_anchor_target_params *p,
                                           const uint8_t *const *anchor_mask_dev, float *labels_dev, float *targets_dev,
                                           int32_t *const *counts_dev, uint8_t *const *fg_hi_dev, void *const *workspace,
                                           size_t workspace_bytes, void *stream);
int mv3d_anchor_target_stage2_batch(int batch, int H, int W, const mv3d_anchor_target_params *p,
                                    const int32_t *const *disable_fg_dev, const int *n_dis_fg,
                                    const int32_t *const *disable_bg1_dev, const int *n_dis_bg1,
                                    const int32_t *const *disable_bg2_dev, const int *n_dis_bg2, float *labels_dev,
                                    float *anchors_dev, float *anchors_3d_dev, int32_t *n_anchors_dev, int anchors_cap,
                                    void *const *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ proposal_target_layer_3d
 * Replaces lib/rpn_msr/proposal_target_layer_tf.py:19-94 with _sample_rois_3d (:227-298),
 * _compute_targets_cnr (:211-225), _get_bbox_regression_labels_3d (:172-194) and the image
 * projection (one frame).  stage1: candidate set = proposals followed by the GT boxes, f64 IoU
 * vs gt_boxes_bv, first-argmax / max, ordered fg / bg candidate lists; counts_dev[4] =
 * [n_candidates, n_fg (max_ov >= FG_THRESH), n_bg (LO <= max_ov < HI), 0].  The caller draws
 * npr.permutation(n_fg)[:k_fg] and npr.permutation(n_bg)[:k_bg] (legacy RandomState.choice
 * without replacement) and stage2 gathers the sampled ROIs: rois_bv (S,5), rois_img (S,5),
 * labels (S) i32, bbox_targets (S, 24*num_classes), rois_3d (S,7), S = n_fg + n_bg rows, fg first.
 * An empty candidate list is not drawn from; with both empty S = 0 (the reference asserts there), stage 2 launches nothing
 * and writes nothing. */
typedef struct {
    int32_t num_classes;         /* n_classes = 2: lib/networks/MV3D_train.py:4 */
    int32_t frame_index;         /* batch column written for the appended ground-truth rows: 0 = the reference
                                    (single-frame batches, :38-44); a batched caller passes the frame's index */
    double fg_thresh;            /* cfg.TRAIN.FG_THRESH    */
    double bg_thresh_hi;         /* cfg.TRAIN.BG_THRESH_HI */
    double bg_thresh_lo;         /* cfg.TRAIN.BG_THRESH_LO */
} mv3d_proposal_target_params;

size_t mv3d_proposal_target_workspace_bytes(int num_rois, int G);
int mv3d_proposal_target_stage1(const float *rois_bv_dev, const float *rois_3d_dev, int num_rois,
                                const float *gt_bv_dev, const float *gt_3d_dev, int G,
                                const mv3d_proposal_target_params *p, int32_t *counts_dev,
                                void *workspace, size_t workspace_bytes, void *stream);
int mv3d_proposal_target_stage2(const float *rois_bv_dev, const float *rois_3d_dev, int num_rois,
                                const float *gt_bv_dev, const float *gt_3d_dev,
                                const float *gt_corners_dev, int G, const float *calib_dev,
                                const mv3d_proposal_target_params *p,
                                const int32_t *fg_pick_dev, int n_fg, const int32_t *bg_pick_dev, int n_bg,
                                float *rois_bv_out, float *rois_img_out, int32_t *labels_out,
                                float *bbox_targets_out, float *rois_3d_out,
                                void *workspace, size_t workspace_bytes, void *stream);

/* The same for `batch` frames behind one launch of every kernel (host-side arrays of per-frame device pointers / counts /
 * parameter structs -- params[b].frame_index = the batch column of frame b's appended ground-truth rows); batch <= 16.
 * stage 2: rois_fv_out (may be NULL, as may its entries) = per-frame (S_b,5) buffers for the third view's ROIs of the sampled
 * boxes, the values mv3d_rois_3d_to_fv gives for rois_3d_out (one launch less on the training path). */
int mv3d_proposal_target_stage1_batch(int batch, const float *const *rois_bv_dev, const float *const *rois_3d_dev,
                                      const int *num_rois, const float *const *gt_bv_dev, const float *const *gt_3d_dev,
                                      const int *G, const mv3d_proposal_target_params *params, int32_t *const *counts_dev,
                                      void *const *workspace, const size_t *workspace_bytes, void *stream);
int mv3d_proposal_target_stage2_batch(int batch, const float *const *rois_bv_dev, const float *const *rois_3d_dev,
                                      const int *num_rois, const float *const *gt_bv_dev, const float *const *gt_3d_dev,
                                      const float *const *gt_corners_dev, const int *G, const float *const *calib_dev,
                                      const mv3d_proposal_target_params *params, const int32_t *const *fg_pick_dev,
                                      const int *n_fg, const int32_t *const *bg_pick_dev, const int *n_bg,
                                      float *const *rois_bv_out, float *const *rois_img_out, int32_t *const *labels_out,
                                      float *const *bbox_targets_out, float *const *rois_3d_out, float *const *rois_fv_out,
                                      void *const *workspace, const size_t *workspace_bytes, void *stream);
/* The batched entries for proposals whose NUMBER stays on the device (the `num_out_dev` of mv3d_proposal_3d): num_rois_cap[b]
 * = the capacity of frame b's proposal blobs (sizes the workspace: mv3d_proposal_target_workspace_bytes(num_rois_cap[b],
 * G[b])), num_rois_dev[b] -> the frame's count, read by the kernels (clamped to [0, cap]).  A training step then needs ONE
 * host round trip -- the counts of the candidate lists the caller draws from -- instead of two. */
int mv3d_proposal_target_stage1_batch_devn(int batch, const float *const *rois_bv_dev, const float *const *rois_3d_dev,
                                           const int *num_rois_cap, const int32_t *const *num_rois_dev,
                                           const float *const *gt_bv_dev, const float *const *gt_3d_dev, const int *G,
                                           const mv3d_proposal_target_params *params, int32_t *const *counts_dev,
                                           void *const *workspace, const size_t *workspace_bytes, void *stream);
int mv3d_proposal_target_stage2_batch_devn(int batch, const float *const *rois_bv_dev, const float *const *rois_3d_dev,
                                           const int *num_rois_cap, const int32_t *const *num_rois_dev,
                                           const float *const *gt_bv_dev, const float *const *gt_3d_dev,
                                           const float *const *gt_corners_dev, const int *G, const float *const *calib_dev,
                                           const mv3d_proposal_target_params *params, const int32_t *const *fg_pick_dev,
                                           const int *n_fg, const int32_t *const *bg_pick_dev, const int *n_bg,
                                           float *const *rois_bv_out, float *const *rois_img_out, int32_t *const *labels_out,
                                           float *const *bbox_targets_out, float *const *rois_3d_out, float *const *rois_fv_out,
                                           void *const *workspace, const size_t *workspace_bytes, void *stream);

/* ------------------------------------------------------------------ SURVEY §8(f) "next" rows
 * BEV rasteriser: replaces point_cloud_2_top (lib/utils/read_lidar.py:10-115, called with
 * res=0.1, zres=0.3, side_range=(-30,30), fwd_range=(0,60), height_range=(-2,0.4):
 * tools/read_lidar.py:121-133).  points_dev (P,4) f32 [x,y,z,reflectance], 16-byte aligned;
 * top_dev (601,601,9) f32: channels 0-7 = z + 2 of the last point of each height slice, channel
 * 8 = reflectance of the last point of the highest slice (numpy fancy-assignment order).
 * This entry and mv3d_point_cloud_2_top_ranges are the body of mv3d_point_cloud_2_top_batch below on ONE frame (offsets_dev == NULL,
 * num_frames == 1; csrc/bev_raster.hip): the same three launches, the clear alone with num_points == 0.  Their own refusals, decided
 * before any launch (MV3D_ERR_INVALID_ARG): num_points < 0 or >= 2^27 (a refusal, where the batched entry skips the rows behind),
 * NULL top_dev, NULL points_dev with num_points > 0, points_dev or top_dev not 16-byte aligned (the batched entry takes a 4-byte
 * aligned top_dev). */
int mv3d_point_cloud_2_top(const float *points_dev, int num_points, float *top_dev, void *stream);

/* The same function with its own parameters (lib/utils/read_lidar.py:10-16: res, zres, side_range, fwd_range, height_range).
 * mv3d_point_cloud_2_top_shape: dims[3] = (y_max + 1, x_max + 1, z_max + 1) of the map (read_lidar.py:49-52), host arithmetic only.
 * mv3d_point_cloud_2_top_ranges: top_dev of that shape; *status_dev (one int32 on the device, written by the call) becomes 1 when a
 * point's cell falls outside the map after numpy's wrap of negative indices -- where the reference's fancy assignment raises
 * IndexError (the point is skipped here; the host mirror raises).  MV3D_ERR_INVALID_ARG: empty or inverted ranges, more than
 * 32767 cells per axis or more than 31 height slices, NULL status_dev, and what mv3d_point_cloud_2_top refuses. */
int mv3d_point_cloud_2_top_shape(double res, double zres, double side_lo, double side_hi, double fwd_lo, double fwd_hi,
                                 double height_lo, double height_hi, int *dims);
int mv3d_point_cloud_2_top_ranges(const float *points_dev, int num_points, double res, double zres, double side_lo, double side_hi,
                                  double fwd_lo, double fwd_hi, double height_lo, double height_hi, float *top_dev,
                                  int *status_dev, void *stream);

/* The same rasteriser for `num_frames` clouds behind three launches (clear, scatter, resolve; the clear alone with total_points == 0),
 * whatever num_frames is (csrc/bev_raster.hip).  Frame b of the output equals, bit for bit, what
 * mv3d_point_cloud_2_top (ranges8_host == NULL) or mv3d_point_cloud_2_top_ranges writes for that frame's rows alone.
 *   points_dev    (total_points, 4) f32 [x, y, z, reflectance], the frames' clouds concatenated, 16-byte aligned (rows are read as
 *                 16-byte vectors); total_points up to INT_MAX
 *   offsets_dev   (num_frames + 1) int32 ON THE DEVICE, mv3d_point_cloud_2_front's rule: frame b owns rows offsets[b] .. offsets[b + 1];
 *                 the frame of a row is the last b with offsets[b] <= row; equal neighbours = an empty frame; rows no frame owns --
 *                 in front of offsets[0], behind offsets[num_frames], anything under offsets that do not ascend -- are ignored, and
 *                 so is a row more than 2^27 - 2 rows into its frame (mv3d_point_cloud_2_top's limit, per frame).  No value in it
 *                 can make the call read or write out of bounds.  NULL with num_frames == 1: the one frame owns every row.
 *   ranges8_host  NULL = the call MV3D makes -> (601, 601, 9) per frame; else res, zres, side_lo, side_hi, fwd_lo, fwd_hi, height_lo,
 *                 height_hi on the HOST, read before the call returns -> the shape mv3d_point_cloud_2_top_shape gives
 *   top_dev       (num_frames, H, W, C) f32 contiguous, 4-byte aligned: it may be any run of frames inside a larger batch buffer
 *                 (one MV3D frame is 13 003 236 bytes = 4 mod 16, so such a run is 16-byte aligned for one frame in four only)
 *   status_dev    required iff ranges8_host: ONE int32 for the whole batch, cleared by the call and set to 1 where
 *                 mv3d_point_cloud_2_top_ranges sets it; ignored without ranges (no cell of MV3D's map can fall outside)
 * Captured in a graph that replays on clouds of changing size (the front view's rule): points_dev is a static buffer of
 * `total_points` rows -- the capacity, which fixes the grid at capture -- and offsets_dev is rewritten before each replay; the rows
 * behind offsets[num_frames] belong to no frame, whatever they hold.
 * No allocation, no host synchronisation; num_frames == 0 returns MV3D_OK without a launch.  MV3D_ERR_INVALID_ARG: num_frames
 * outside [0, MV3D_FV_MAX_FRAMES], negative total_points, NULL or misaligned pointers, offsets_dev == NULL with num_frames != 1,
 * ranges mv3d_point_cloud_2_top_shape refuses, ranges without status_dev.
 * mv3d_point_cloud_2_top_batch is the entry: its resolve stores only the 16-byte vectors a point fell into (an empty key is
 * already 0.0f).  mv3d_point_cloud_2_top_batch_dense is the same call with a resolve that stores every element:
 * the same bits, 1.5 - 3 % slower where it was measured, and there for tools/bev_batch_bench.py to
 * time against the entry -- nothing else calls it. */
int mv3d_point_cloud_2_top_batch(const float *points_dev, const int32_t *offsets_dev, int num_frames, int total_points,
                                 const double *ranges8_host, float *top_dev, int32_t *status_dev, void *stream);
int mv3d_point_cloud_2_top_batch_dense(const float *points_dev, const int32_t *offsets_dev, int num_frames, int total_points,
                                       const double *ranges8_host, float *top_dev, int32_t *status_dev, void *stream);

/* The MV3D paper's BEV encoding (section 3.1 of the paper; csrc/bev_paper.hip) from the same inputs: a second
 * scatter / resolve body beside the one above, three launches whatever num_frames is.  PARITY UNPINNED: the reference has no such
 * raster; tests/bev_paper_restatement.py states the definition.  Kept rows, cells and height slices are those of
 * mv3d_point_cloud_2_top_batch (one statement, csrc/bev_cell.h): a row passes the two range tests and falls into the slice set
 * S = { i < M : z in [height_i, height_i + zres) }, M = ceil((height_hi - height_lo) / zres); a row with empty S is dropped; a row
 * with non-empty S whose cell lies outside the map sets *status_dev and is dropped.  Per frame (H, W, M + 2) -- (601, 601, 10)
 * without ranges:
 *   channel i < M   max z of the kept rows with i in S, as z - (float)height_lo
 *   channel M       reflectance (bit for bit) of the kept row with the largest z (-0.0 == +0.0); among equal z the last row of the frame
 *   channel M + 1   T[min(N, 63)], N = the cell's kept rows, T = mv3d_bev_density_table: min(1, log(N + 1) / log 64)
 * and an empty cell is all zeros.  The map does not depend on the order of a frame's rows.
 * Arguments, alignment, the offsets rule ("no value in it can make the call read or write out of bounds"), capture and refusals are
 * mv3d_point_cloud_2_top_batch's, plus
 *   workspace_dev  mv3d_point_cloud_2_top_paper_workspace(num_frames, ranges8_host) bytes on the device, 16-byte aligned, the
 *                  caller's: 8 bytes per cell and frame (the winner words).  Cleared by the call; nothing is kept in it between calls.
 * mv3d_point_cloud_2_top_paper_shape: dims[3] = (H, W, M + 2), refusing what mv3d_point_cloud_2_top_shape refuses.
 * mv3d_point_cloud_2_top_paper_workspace: 0 for num_frames outside [1, MV3D_FV_MAX_FRAMES] or such ranges.
 * mv3d_bev_density_table (HOST only, no device work): out64[n] = (float)fmin(1.0, log((double)(n + 1)) / log(64.0)), n = 0 .. 63,
 * computed with libm -- the table the resolve kernel is handed by value; out64[0] == 0, out64[63] == 1. */
int mv3d_point_cloud_2_top_paper_batch(const float *points_dev, const int32_t *offsets_dev, int num_frames, int total_points,
                                       const double *ranges8_host, float *top_dev, void *workspace_dev, int32_t *status_dev,
                                       void *stream);
size_t mv3d_point_cloud_2_top_paper_workspace(int num_frames, const double *ranges8_host);
int mv3d_point_cloud_2_top_paper_shape(double res, double zres, double side_lo, double side_hi, double fwd_lo, double fwd_hi,
                                       double height_lo, double height_hi, int *dims);
int mv3d_bev_density_table(float *out64);

/* ------------------------------------------------------------------ crop to the camera image (csrc/scan_crop.hip)
 * "We also remove points that are out of the image boundaries when projected to the image plane" (the MV3D paper, section 3.4), in
 * front of the rasterisers above: a stable compaction of `num_frames` clouds back to back into another such batch.  PARITY UNPINNED:
 * the reference has no such code; tests/scan_crop_restatement.py states the rule.
 *   points_dev      (total_points, 4) f32 [x, y, z, reflectance], the frames' clouds concatenated, 16-byte aligned; never written
 *   offsets_dev     (num_frames + 1) int32 ON THE DEVICE, mv3d_point_cloud_2_front's rule: frame b owns rows offsets[b] .. offsets[b + 1];
 *                   rows no frame owns -- in front of offsets[0], behind offsets[num_frames], anything under offsets that do not
 *                   ascend -- are dropped.  NULL with num_frames == 1: the one frame owns every row.
 *   calib_dev       (num_frames, 48) f32: per frame the (4, 12) calibration table of the feeds (P2, P3, R0_rect, Tr_velo_to_cam)
 *   image_hw_dev    (num_frames, 2) int32: per frame the height and the width of its image
 *   points_out_dev  (total_points, 4) f32, 16-byte aligned, no byte in common with points_dev: the kept rows of frame 0 from row 0 on
 *                   and the frames behind it back to back, each frame's rows in their order, every row copied as 16 bytes bit for bit
 *                   (a NaN reflectance keeps its payload); the rows at and behind offsets_out[num_frames] are not written
 *   offsets_out_dev (num_frames + 1) int32: offsets_out[b] = the kept rows of the frames < b, so offsets_out[0] = 0 --
 *                   (points_out_dev, offsets_out_dev) is a batch like (points_dev, offsets_dev)
 *   workspace_dev   workspace_bytes >= mv3d_scan_crop_workspace(total_points) bytes, 16-byte aligned, the caller's; it needs no
 *                   initialisation and holds nothing between calls
 * Kept: a row of frame b whose x, y, z are finite and for which, with M = (P2 . R0) . Tr of the frame's table in f32 (the matrix
 * mv3d_proposal_3d projects with, tests/golden/proj_matrix.npz) and v[r] = fma(M[r][3], 1, fma(M[r][2], z, fma(M[r][1], y,
 * fma(M[r][0], x, 0)))) in f64 (homogeneous w = 1, a position): v[2] > 0 and, u = v[0] / v[2], w = v[1] / v[2] in f64,
 * 0 <= u < width and 0 <= w < height.  No margin, no minimum depth; a frame whose height or width is <= 0 keeps nothing; the
 * reflectance is never examined.
 * No value in offsets_dev, calib_dev or image_hw_dev can make the call read or write out of bounds.  Three launches on `stream`
 * whatever the batch (flags, scan, copy; the scan alone with total_points == 0, which writes offsets_out = 0), none of whose workgroups
 * waits for another; no allocation, no host synchronisation; capturable, and a replay may find other clouds and other device
 * offsets in the same buffers (total_points, the capacity, fixes the grid).  num_frames == 0 returns MV3D_OK without a launch.
 * MV3D_ERR_INVALID_ARG before any launch: num_frames outside [0, MV3D_FV_MAX_FRAMES], negative total_points, NULL or misaligned
 * pointers (points, output and workspace may be NULL with total_points == 0), offsets_dev == NULL with num_frames != 1, a workspace
 * that is too small, points_out_dev overlapping points_dev.
 * mv3d_scan_crop_workspace: bytes for total_points rows (one bit per row and 4 bytes per tile, each part rounded up to 256); 0 for
 * a count <= 0.  mv3d_scan_crop_tile_rows (HOST only): the consecutive rows one workgroup compacts, for the tests' sizes. */
size_t mv3d_scan_crop_workspace(int total_points);
int mv3d_scan_crop_tile_rows(void);
int mv3d_scan_crop_to_image(const float *points_dev, const int32_t *offsets_dev, int num_frames, int total_points,
                            const float *calib_dev, const int32_t *image_hw_dev, float *points_out_dev, int32_t *offsets_out_dev,
                            void *workspace_dev, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ scan augmentation (csrc/scan_transform.hip)
 * A similarity transform of the LIDAR frame per cloud -- a rotation about the vertical axis, a uniform scale, a shift, A = [s R | t]
 * -- on `num_frames` clouds back to back, in front of the crop and the rasterisers above (cfg.TRAIN.SCAN_AUGMENT; the annotation and
 * the calibration follow on the host, mv3d_tf_amd/datasets/augment.py).  PARITY UNPINNED: the reference trains from stored maps and
 * has no such code; tests/scan_augment_restatement.py states the rule.
 *   points_dev      (total_points, 4) f32 [x, y, z, reflectance], the frames' clouds concatenated, 16-byte aligned
 *   offsets_dev     (num_frames + 1) int32 ON THE DEVICE, mv3d_point_cloud_2_front's rule: frame b owns rows offsets[b] .. offsets[b + 1];
 *                   rows no frame owns -- in front of offsets[0], behind offsets[num_frames], anything under offsets that do not
 *                   ascend -- are copied as they are.  NULL with num_frames == 1: the one frame owns every row.
 *   xform_dev       (num_frames, 12) f64 ON THE DEVICE, 8-byte aligned: per frame the 3x4 matrix A, row-major.  Any twelve numbers
 *                   are taken as they are; the entry does not ask for a similarity.
 *   points_out_dev  (total_points, 4) f32, 16-byte aligned: points_dev itself (in place) or a buffer with no byte in common with it
 * A row [x, y, z, r] of frame b with finite x, y, z becomes c'_i = (float)fma(A[i][3], 1, fma(A[i][2], z, fma(A[i][1], y,
 * fma(A[i][0], x, 0)))) in f64, i = 0, 1, 2, and r bit for bit (a NaN reflectance keeps its payload).  A row with a non-finite
 * coordinate is copied, all 16 bytes bit for bit: the rasterisers and the crop drop it as they drop it untransformed.  Every row of
 * [0, total_points) is written.
 * No value in offsets_dev or xform_dev can make the call read or write out of bounds.  One launch on `stream`, one thread per row; no
 * allocation, no host synchronisation, nothing read back; capturable, and a replay may find other clouds, other device offsets and
 * other matrices in the same buffers (total_points, the capacity, fixes the grid).  num_frames == 0 and total_points == 0 return
 * MV3D_OK without a launch.  MV3D_ERR_INVALID_ARG before any launch: num_frames outside [0, MV3D_FV_MAX_FRAMES], negative
 * total_points, NULL or misaligned pointers (points and output may be NULL with total_points == 0), offsets_dev == NULL with
 * num_frames != 1, points_out_dev overlapping points_dev without being equal to it. */
int mv3d_scan_transform(const float *points_dev, const int32_t *offsets_dev, int num_frames, int total_points,
                        const double *xform_dev, float *points_out_dev, void *stream);

/* ------------------------------------------------------------------ the target layers' random subsamplings (HOST code)
 * The reference subsamples with `npr.choice(inds, size=k, replace=False)` on the numpy GLOBAL legacy RandomState
 * (lib/rpn_msr/anchor_target_layer_tf.py:146-159,178-183; lib/rpn_msr/proposal_target_layer_tf.py:246-269) = 
 * `inds[permutation(len(inds))[:k]]`; the stage-2 entries above take those permutations as index lists.  These two host
 * functions draw them in C directly on the memory of numpy's generator (`mt19937_state` = the address numpy publishes as
 * `np.random.mtrand._rand._bit_generator.ctypes.state_address`: {uint32 key[624]; int32 pos}), restating numpy's
 * RandomState.permutation -> shuffle -> random_interval -> MT19937 genrand loop (numpy is a dependency of the reference that
 * /root/reference does not vendor; pinned against numpy itself in tests/test_legacy_rng.py).  The caller holds the
 * generator's lock (`bit_generator.lock`); no device work, no stream. */
/* out[0 .. n) = RandomState.permutation(n) */
int mv3d_legacy_permutation(void *mt19937_state, int32_t n, int32_t *out);
typedef struct {
    int32_t n_fg, n_bg, n_low;     /* anchor-target stage 1 counts: foreground / background / low-overlap candidates */
    int32_t pt_n_fg, pt_n_bg;      /* proposal-target stage 1 counts */
    int32_t reserved0;
    const uint8_t *fg_alive;       /* (n_fg) host bytes: foreground candidate i still positive after the relabel (:176) */
} mv3d_draw_frame;
typedef struct {
    int32_t rpn_batchsize;         /* cfg.TRAIN.RPN_BATCHSIZE */
    int32_t rpn_num_fg;            /* int(cfg.TRAIN.RPN_FG_FRACTION * RPN_BATCHSIZE) */
    int32_t rois_per_image;        /* cfg.TRAIN.BATCH_SIZE / images per batch (1) */
    int32_t roi_fg_max;            /* np.round(cfg.TRAIN.FG_FRACTION * rois_per_image) */
} mv3d_draw_params;
/* All draws of a batch, frame by frame, anchor targets before proposal targets (the order the numpy-contract layers draw in):
 * per frame five lists -- anchors to disable: surplus foreground, surplus background, surplus background after the relabel;
 * ROIs to keep: foreground picks, background picks -- appended to `lists` (host, e.g. pinned), sizes[5 * b + k] = their
 * lengths.  scratch: >= the largest candidate count, in int32 words.  MV3D_ERR_WORKSPACE if `lists` / `scratch` are too small. */
int mv3d_draw_training_subsamples(void *mt19937_state, int batch, const mv3d_draw_frame *frames, const mv3d_draw_params *par,
                                  int32_t *lists, size_t lists_cap, int32_t *sizes, int32_t *scratch, size_t scratch_cap);

/* ------------------------------------------------------------------ the training path on fresh frames, driven from C
 * One object runs what lib/networks/MV3D_train.py:83-112 wires behind the RPN heads for every training batch --
 *   proposal_layer_3d (TRAIN cfg)      lib/rpn_msr/proposal_layer_tf.py:25-202       = mv3d_proposal_3d
 *   anchor_target_layer                lib/rpn_msr/anchor_target_layer_tf.py:21-250  = mv3d_anchor_target_stage1/2_batch
 *   proposal_target_layer_3d           lib/rpn_msr/proposal_target_layer_tf.py:19-94 = mv3d_proposal_target_stage1/2_batch_devn
 * -- with the reference's host-side subsampling draws (mv3d_draw_training_subsamples on numpy's global generator) in between:
 *   submit()  enqueues every launch up to the candidate lists on `stream`, the copies of the counts to the slot's pinned host
 *             buffers and an event; returns at once.
 *   a helper thread owned by the object (created with helper_thread = 1) waits for that event, draws -- slots strictly in
 *             submission order, so the generator's stream is the reference's: frame by frame, anchor targets before proposal
 *             targets -- uploads the index lists and enqueues stage 2 on the same stream.
 *   finish()  waits until the slot's stage 2 is ENQUEUED (not executed) and reports the frames' row counts; the outputs are in the
 *             slot's buffers, ordered on the stream given to submit().  With helper_thread = 0 finish() does the helper's work itself.
 * A caller keeps up to `depth` batches in flight (submit batch i + 1 before finish of batch i): the host's draws of one batch then run
 * while the device works on its neighbours, and a batch costs its caller two calls.  Between submit() and finish() of a slot the
 * generator behind `mt19937_state` belongs to the object.  All buffers are the caller's (layouts: see the per-entry comments above;
 * B = batch <= 16, N = 4 H W anchors, cap = mv3d_proposal_3d_capacity): the object allocates only events and its thread. */
typedef struct {
    int32_t batch, H, W, num_classes;
    int32_t proposal_cap;          /* mv3d_proposal_3d_capacity(H, W, &proposal): rows per frame of the proposal blobs */
    int32_t anchor_cap;            /* rows per frame of anchors / anchors_3d */
    int32_t roi_cap;               /* rows per frame of the sampled-ROI outputs (cfg.TRAIN.BATCH_SIZE) */
    int32_t max_gt;                /* ground-truth boxes per frame the workspaces were sized for */
    mv3d_proposal_params proposal;
    mv3d_anchor_target_params anchor;
    mv3d_proposal_target_params target;      /* thresholds (frame_index is set per frame by the object) */
    mv3d_draw_params draw;
} mv3d_train_path_config;
typedef struct {
    /* device */
    float *blob_bv, *blob_img, *blob_3d;     /* proposals (B,cap,5) (B,cap,5) (B,cap,7) */
    int32_t *num_proposals;                  /* (2 B): the frames' proposal counts, then mv3d_proposal_3d's status words */
    void *proposal_ws; size_t proposal_ws_bytes;
    float *rpn_labels, *rpn_targets;         /* (B,N) (B,N,6) */
    float *anchors, *anchors_3d;             /* (B,anchor_cap,5) (B,anchor_cap,7) */
    int32_t *n_anchors;                      /* (B) */
    uint8_t *report; size_t report_row;      /* (B,report_row): per frame [counts 32 B | foreground flags N B], report_row % 256 == 0 */
    int32_t *pt_counts;                      /* (B,4) */
    void *anchor_ws; size_t anchor_ws_bytes; /* B workspaces back to back, each anchor_ws_bytes (a multiple of 256) */
    void *target_ws; size_t target_ws_bytes; /* the same for the proposal-target workspaces */
    float *rois_bev, *rois_rgb, *rois_fv;    /* (B roi_cap,5) each, frame b's rows behind frame b - 1's; rois_fv may be NULL */
    float *rois_3d; int32_t *labels; float *bbox_targets;    /* (B roi_cap,7) (B roi_cap) (B roi_cap, 24 num_classes) */
    int32_t *lists; size_t lists_cap;        /* the index lists of a batch, int32 words: >= B (3 N + 2 (cap + max_gt)) */
    /* host (pinned, except h_scratch) */
    uint8_t *h_report; size_t h_report_row;  /* (B,h_report_row): the first h_report_row <= report_row bytes of every report row */
    int32_t *h_pt_counts;                    /* (B,4) */
    int32_t *h_num_proposals;                /* (2 B) */
    int32_t *h_lists;                        /* lists_cap words */
    int32_t *h_scratch; size_t scratch_cap;  /* >= max(N, cap + max_gt) words: one permutation at its largest */
} mv3d_train_path_slot;
typedef struct mv3d_train_path mv3d_train_path;
int mv3d_train_path_create(const mv3d_train_path_config *config, int depth, const mv3d_train_path_slot *slots, int helper_thread,
                           mv3d_train_path **out);
/* replace the parameter structs (thresholds, NMS settings, draw sizes; the geometry must be unchanged); no slot may be in flight */
int mv3d_train_path_configure(mv3d_train_path *path, const mv3d_train_path_config *config);
/* prob (B,H,W,8), pred (B,H,W,24), im_info (B,3), calib (B,4,12): device f32; gt_*: host arrays of B device pointers -- gt_bv (G,5),
 * gt_3d (G,7), gt_corners (G,25) -- and G (B) with 1 <= G[b] <= max_gt.  The inputs must stay valid until finish() has returned. */
int mv3d_train_path_submit(mv3d_train_path *path, int slot, const float *prob_dev, const float *pred_dev, const float *im_info_dev,
                           const float *calib_dev, const float *const *gt_bv_dev, const float *const *gt_3d_dev,
                           const float *const *gt_corners_dev, const int *G, void *mt19937_state, void *stream);
/* submit with the frames' empty-anchor masks: anchor_mask_dev (B,N) u8, contiguous (mv3d_anchor_occupancy), or NULL.  It is handed
 * to the batch's proposal layer and anchor-target stage 1 (the masked entries above) and, like the other inputs, must stay valid
 * until finish() has returned.  The draws, the helper thread and finish() are the same.  mv3d_train_path_submit is this entry with
 * a NULL mask. */
int mv3d_train_path_submit_masked(mv3d_train_path *path, int slot, const float *prob_dev, const float *pred_dev,
                                  const float *im_info_dev, const float *calib_dev, const float *const *gt_bv_dev,
                                  const float *const *gt_3d_dev, const float *const *gt_corners_dev, const int *G,
                                  const uint8_t *anchor_mask_dev, void *mt19937_state, void *stream);
/* rows_out (B): sampled ROIs per frame (frame b's rows start at the sum of the frames before it); num_proposals_out (B); sizes_out
 * (5 B, may be NULL): the lengths of the drawn lists as mv3d_draw_training_subsamples reports them.  Returns the first error of the
 * slot's host stage (MV3D_ERR_ZERO_DIVISION where the reference's NMS raises); the slot is free again either way. */
int mv3d_train_path_finish(mv3d_train_path *path, int slot, int32_t *rows_out, int32_t *num_proposals_out, int32_t *sizes_out);
/* host seconds the helper spent waiting for stage 1 / drawing since the last call (diagnostics); either pointer may be NULL */
int mv3d_train_path_host_seconds(mv3d_train_path *path, double *wait_s, double *draw_s);
void mv3d_train_path_destroy(mv3d_train_path *path);     /* waits for the slots in flight, joins the thread */
/* What a path of this configuration enqueues per batch (host only, no device call): the launches of stage 1 (submit) and of stage 2
 * (the host stage; the lists' upload counts as one, and so does the disable launch, which a batch with nothing to disable skips), the
 * NMS rounds counted by the plan of mv3d_nms_round_plan (round 1 is two launches), the reports written through mapped pinned buffers.
 * Returns 1 when independent launches of the batch are paired in one grid (proposal decode || anchor overlap, local rank || anchor
 * labels, merge rank || anchor compaction, anchor emit || ROI emit; the reports written by the last launch of stage 1), 0 when the
 * configuration keeps the single-purpose launches (the counting rank path: more than 24576 keys per frame), -1 for a configuration
 * mv3d_train_path_create refuses.  Either pointer may be NULL. */
int mv3d_train_path_launch_plan(const mv3d_train_path_config *config, int32_t *stage1_launches, int32_t *stage2_launches);

/* KITTI label rows -> ground-truth encodings (lib/datasets/kitti_mv3d.py:240-272 with computeCorners3D, camera_to_lidar_cnr,
 * lidar_cnr_to_3d, lidar_3d_to_bv of lib/utils/transform.py:441-465,502-524,172-187,113-142), one thread per labelled object:
 *   box_cam_dev (G,6) f32 [tx,ty,tz,l,w,h] (label columns 11-13, 10, 9, 8), cos_sin_dev (G,2) f64 = cos / sin of rotation_y,
 *   inv_rot_dev (9) f32 = inverse of the 3x3 rotation part of Tr_velo_to_cam, tr_velo_to_cam_dev (12) f32
 *   -> corners_cam_dev (G,24), corners_lidar_dev (G,24) [x0..7,y0..7,z0..7], boxes_3d_dev (G,6) LIDAR box, boxes_bv_dev (G,4)
 *   BEV pixel box, all f32 as the roidb stores them.  (cos / sin and the 3x3 inverse are numpy / LAPACK calls on a handful of
 *   host scalars in the reference and stay on the host next to the text parsing.) */
int mv3d_gt_encode(const float *box_cam_dev, const double *cos_sin_dev, int num_objects, const float *inv_rot_dev,
                   const float *tr_velo_to_cam_dev, float *corners_cam_dev, float *corners_lidar_dev,
                   float *boxes_3d_dev, float *boxes_bv_dev, void *stream);

/* Test-time tail of box_detect (lib/fast_rcnn/test_mv.py:240-261): rois_3d_dev (R,7) = rois[2],
 * bbox_pred_dev (R,24*nc) -> corners (R,24) [lidar_3d_to_corners], pred_cnr_r (R,24*nc)
 * [bbox_transform_inv_cnr, lib/fast_rcnn/bbox_transform.py:157-176], pred_bv / pred_bv_r (R,4*nc)
 * [corners_to_bv, lib/utils/transform.py:342-366, of the unregressed / regressed corners]. */
int mv3d_box_detect_tail(const float *rois_3d_dev, const float *bbox_pred_dev, int num_rois, int num_classes,
                         float *corners_dev, float *pred_cnr_r_dev, float *pred_bv_dev, float *pred_bv_r_dev,
                         void *stream);

/* What test_net does with every frame behind box_detect (lib/fast_rcnn/test_mv.py:420-444, 491-501), for a batch of frames
 * laid out as the serving step leaves them (frame f owns rows [f * rows_per_frame, (f + 1) * rows_per_frame) of every input):
 * per foreground class j the rows r < num_rois[f] with cls_prob[r, j] > score_thresh (f32 compare; NaN drops out), in
 * descending score order (ties by descending row), greedy NMS of pred_bv[r, 4j:4j+4] at nms_thresh (the rule of
 * mv3d_nms_device, or of _nms if nms_strict_gt), then the cap over all classes: with more than max_per_image kept detections in
 * the frame, every class keeps its scores >= the max_per_image-th largest kept score (ties may keep more).
 *   cls_prob_dev (B*cap, K) f32, pred_bv_dev (B*cap, 4K), corners_dev (B*cap, 24) [the unregressed corners, shared by the
 *   classes], pred_cnr_r_dev (B*cap, 24K) or NULL, num_rois_dev (B) i32 or NULL (= every frame has cap rows)
 *   -> det_bv_dev (B, K, cap, 5) [x1,y1,x2,y2,score], det_cnr_dev (B, K, cap, 25) [24 corners, score], det_cnr_r_dev
 *   (B, K, cap, 25) (required iff pred_cnr_r_dev), det_row_dev (B, K, cap) i32 source row inside the frame, det_count_dev (B, K)
 *   i32 (class 0: 0); rows behind det_count are unspecified.  status_dev (B) i32 flag bits as for the NMS: OR-ed into, so zeroed
 *   by the caller; bit 0 = a zero union where the reference raises ZeroDivisionError (the pair does not suppress).
 * Kernel launches only (at most two): no allocation, memset, synchronisation or host read, so the call can be captured in a
 * graph.  num_classes 2..8, rows_per_frame 1..2048, batch 1..65535; MV3D_ERR_INVALID_ARG otherwise or for a NULL pointer, before
 * any HIP call.  No global scratch is needed: the workspace query returns 0 and `workspace` may be NULL. */
typedef struct {
    int32_t num_classes;     /* K, background class 0 included */
    int32_t rows_per_frame;  /* cap */
    int32_t max_per_image;   /* <= 0: no cap */
    int32_t nms_strict_gt;   /* 0: cpu_nms rule, (double)IoU >= thresh (the parity target); 1: gpu_nms rule, IoU > thresh in f32 */
    float score_thresh;      /* the callers pass 0.05 (lib/fast_rcnn/test_mv.py:421) */
    int32_t reserved0;
    double nms_thresh;       /* cfg.TEST.NMS */
} mv3d_detect_post_params;

size_t mv3d_detect_post_workspace_bytes(int batch, const mv3d_detect_post_params *p);
int mv3d_detect_post(const float *cls_prob_dev, const float *pred_bv_dev, const float *corners_dev,
                     const float *pred_cnr_r_dev, const int32_t *num_rois_dev, int batch,
                     const mv3d_detect_post_params *p, float *det_bv_dev, float *det_cnr_dev, float *det_cnr_r_dev,
                     int32_t *det_row_dev, int32_t *det_count_dev, int32_t *status_dev, void *workspace,
                     size_t workspace_bytes, void *stream);

/* The same tail with ORIENTED NMS (not in the reference's test_net; the MV3D paper's rule for final detections): candidates,
 * order, outputs and cap are mv3d_detect_post's, bit for bit; a candidate is suppressed by an earlier kept one by the IoU of
 * their BEV footprints, computed as the KITTI evaluator computes it (mv3d_kitti_eval_overlaps), all f64 from the f32 corners.
 *   footprint of row r, class j: 24 f32 [x0..7, y0..7, z0..7]; footprint_source 0 = corners_dev[r] (the proposal's box, shared by
 *   the classes), 1 = pred_cnr_r_dev[r, 24j : 24j + 24] (the regressed corners; pred_cnr_r_dev is then required).  The polygon is
 *   vertices 0..3.  It need not be a rectangle or convex: the result is defined by the operation order, as in the evaluator.
 *   overlap of (earlier a, later b) in processing order: f64 min / max of x and y over vertices 0..3; disjoint extents
 *   (a.maxx < b.minx || b.maxx < a.minx || a.maxy < b.miny || b.maxy < a.miny) = 0.0; otherwise the evaluator's clip with a as
 *   the polygon and b as the clipper.  b is suppressed iff iou_bev >= nms_thresh (nms_strict_gt: iou_bev > nms_thresh), compared
 *   in f64.  A box with a non-finite value among its 24 has IoU 0.0 with everything (it is kept and suppresses nothing) and sets
 *   MV3D_DETECT_STATUS_NONFINITE in status_dev[frame] if it passed the score cut; bit 0 is never set by this entry.
 * det_bv_dev still carries the rows' pixel boxes.  Kernel launches only (at most four), so the call can be captured in a graph.
 * The workspace (mv3d_detect_post_oriented_workspace_bytes: about batch * (K-1) * cap * (cap / 64) * 8 bytes) is
 * required and need not be initialised; only its base pointer has to be 16-byte aligned (a misaligned one is refused), the parts
 * inside are carved at 256-byte granularity and the query counts that padding; MV3D_ERR_INVALID_ARG for a NULL or short one, for footprint_source outside {0, 1} and
 * for everything mv3d_detect_post refuses, before any HIP call.  Same limits as mv3d_detect_post. */
#define MV3D_DETECT_STATUS_NONFINITE 2
size_t mv3d_detect_post_oriented_workspace_bytes(int batch, const mv3d_detect_post_params *p);
int mv3d_detect_post_oriented(const float *cls_prob_dev, const float *pred_bv_dev, const float *corners_dev,
                              const float *pred_cnr_r_dev, const int32_t *num_rois_dev, int batch,
                              const mv3d_detect_post_params *p, int footprint_source, float *det_bv_dev, float *det_cnr_dev,
                              float *det_cnr_r_dev, int32_t *det_row_dev, int32_t *det_count_dev, int32_t *status_dev,
                              void *workspace, size_t workspace_bytes, void *stream);

/* Training losses and their gradients (lib/fast_rcnn/train_mv.py:74-136), fused: losses_dev[0] = mean softmax
 * cross-entropy, losses_dev[1] = mean over rows of sum smooth-L1 (sigma = 3 in the reference) of pred - target;
 * d_*_dev (may be NULL) receive d loss / d logits and d loss / d pred.  A mean over no rows is NaN, as in TF.
 * RPN (:92-113): rpn_cls_score (N,2) = rpn_cls_score_reshape, labels f32 in {-1,0,1} = rpn_data[0]; cross-entropy
 * over label != -1, box loss over label == 1, rpn_bbox_pred / targets (N,6).
 * RCNN (:115-127): cls_score (S,K), labels i32 = roi_data_3d[2], bbox_pred / targets (S, box_dim = 24 K); all rows. */
size_t mv3d_loss_workspace_bytes(int rows);
int mv3d_rpn_loss(const float *rpn_cls_score_dev, const float *rpn_labels_dev, const float *rpn_bbox_pred_dev,
                  const float *rpn_bbox_targets_dev, int num_anchors, float sigma, float *losses_dev,
                  float *d_cls_score_dev, float *d_bbox_pred_dev, void *workspace, size_t workspace_bytes, void *stream);
int mv3d_rcnn_loss(const float *cls_score_dev, const int32_t *labels_dev, const float *bbox_pred_dev,
                   const float *bbox_targets_dev, int num_rois, int num_classes, int box_dim, float sigma,
                   float *losses_dev, float *d_cls_score_dev, float *d_bbox_pred_dev, void *workspace,
                   size_t workspace_bytes, void *stream);
/* (not in the reference) mv3d_rcnn_loss with the row selection label != -1 for BOTH terms: the means run over the selected rows, the
 * mean over no rows is NaN (the RPN's rule), the gradient rows of skipped rows are exactly 0.  Same kernels, same arguments, same
 * workspace; with no label at -1 every output is bit-equal to mv3d_rcnn_loss.  In mv3d_rcnn_loss itself a label of -1 stays out of
 * range (a NaN loss). */
int mv3d_rcnn_loss_ignore(const float *cls_score_dev, const int32_t *labels_dev, const float *bbox_pred_dev,
                          const float *bbox_targets_dev, int num_rois, int num_classes, int box_dim, float sigma,
                          float *losses_dev, float *d_cls_score_dev, float *d_bbox_pred_dev, void *workspace,
                          size_t workspace_bytes, void *stream);

/* (not in the reference) Ignore regions in training: sampled background anchors and sampled background ROIs that lie on an ignore
 * region of their frame get label -1.  Out of place: the inputs are not written, every output label is.
 *   IoA(c, q)  intersection over the CANDIDATE's area, all f64, +1 pixel convention: iw = min(c2, q2) - max(c0, q0) + 1, ih likewise,
 *              both > 0 or the result is 0; iw * ih / ((c2 - c0 + 1) (c3 - c1 + 1)); 0 when that area is not > 0 or any of the eight
 *              numbers is NaN.
 *   relabel    a label that is exactly 0 becomes -1 iff max_k IoA(c_bv, ignore_bv[b][k]) >= overlap or
 *              max_m IoA(c_img, ignore_img[b][m]) >= overlap (f64 compare; a NaN overlap relabels nothing); every other label passes
 *              through bit for bit.
 *   anchors    rpn_labels (batch, N = 4 H W) f32: c_bv = anchor n of the W-wide grid at feat_stride as integers, not clipped; c_img =
 *              the image box of that anchor's 3D prior under calib[b] (batch, 4, 12), as mv3d_proposal_3d decodes it (four int32).
 *   ROIs       roi_labels (num_rois) i32; c_bv = rois_bv[r, 1:5], c_img = rois_img[r, 1:5] (both (num_rois, 5) f32), frame =
 *              rois_bv[r, 0]; a row whose frame column is no integer in [0, batch) passes through.
 *   lists      ignore_*_dev (rows, 4) f32 [x1, y1, x2, y2] packed frame after frame, ignore_*_off_dev (batch + 1) i32 ON THE DEVICE:
 *              frame b owns rows off[b] .. off[b + 1].  Empty frames and empty lists (rows = 0, data pointer NULL) are ordinary.
 *   counts_dev (batch, 2) i32 or NULL: relabelled anchors and ROIs per frame.
 *   status_dev (batch) i32 or NULL: MV3D_OK, or MV3D_ERR_INVALID_ARG for a frame whose offsets (either list) are negative, decrease,
 *              run past the given row count or span more than 1024 boxes; such a frame's labels are written through unchanged and
 *              its counts are 0.  Nothing in the offsets can take a read out of bounds.
 * ONE launch, grid (batch, 2) of 1024 threads; no allocation, no read-back, no synchronisation (capturable).  MV3D_ERR_INVALID_ARG
 * before the launch: a NULL required pointer (the four ROI arrays are required only for num_rois > 0), batch outside [1, 65535],
 * H, W or feat_stride < 1, negative counts, 4 H W or the last anchor beyond int32. */
int mv3d_ignore_relabel(const float *rpn_labels_dev, const int32_t *roi_labels_dev, const float *rois_bv_dev,
                        const float *rois_img_dev, int num_rois, const float *calib_dev, int batch, int H, int W,
                        int feat_stride, const float *ignore_bv_dev, const int32_t *ignore_bv_off_dev, int ignore_bv_rows,
                        const float *ignore_img_dev, const int32_t *ignore_img_off_dev, int ignore_img_rows, double overlap,
                        float *rpn_labels_out_dev, int32_t *roi_labels_out_dev, int32_t *counts_dev, int32_t *status_dev,
                        void *stream);

/* ------------------------------------------------------------------ the VGG16 trunk's contraction (north_star "MFMA only for the
 * VGG16 conv backbone"): Network.conv(3, 3, c_o, 1, 1) [3x3, stride 1, SAME, + bias, optional ReLU] and
 * Network.max_pool(2, 2, 2, 2, 'VALID') of lib/networks/network.py:109-133,182-189 for the layers of
 * lib/networks/MV3D_train.py:44-81, as an implicit GEMM on v_mfma_f32_32x32x16_f16 (f16 operands, f32 accumulate).
 * This is the SERVING trunk (BASELINE configs[4]: fp16), lower precision than the reference's fp32 graph and not part of the
 * bit-exact contract; tolerance vs an fp32 convolution of the same f16-rounded operands: 2e-3 relative to the map's max.
 *   x_framed  (batch, height + 2, width + 2, c_in)  f16 NHWC with a one-pixel ZERO frame (the SAME padding, materialised)
 *   w_packed  (c_out, 9 * c_in) f16, k = (ky * 3 + kx) * c_in + c   [TF's HWIO filter transposed to (O, H, W, I)]
 *   bias      (c_out) f32
 *   y         out_framed ? (batch, height + 2, width + 2, c_out) interior only (the frame is the owner's, zeroed once)
 *                        : (batch, height, width, c_out);  f32 if out_f32 (the map a RoiPool layer reads) else f16
 * c_in and c_out multiples of 64, or c_in == 16 = the input layer (conv1_1: 9 / 3 channels zero-padded to 16), whose weights are
 * packed (c_out, 192): k = 16 * tap + c for the 9 taps, zero for tap slots 9..11.  Every buffer < 2 GiB (32-bit buffer
 * offsets: split the batch above that) and 16-byte aligned; MV3D_ERR_INVALID_ARG otherwise, before any launch. */
int mv3d_conv3x3_f16(const void *x_framed, const void *w_packed, const float *bias, void *y, int batch, int height, int width,
                     int c_in, int c_out, int out_framed, int out_f32, int relu, void *stream);
/* The same convolution in the REFERENCE'S precision: f32 framed maps (c_in a multiple of 32; the input layer's 9 / 3 channels padded to
 * 32), f32 packed weights (c_out, 9 * c_in), f32 output (framed or not), exact f32 products and sums on v_mfma_f32_32x32x2_f32 -- only
 * the summation order differs from any other fp32 convolution.  MFMA-bound at the f32 matrix rate (157 TFLOP/s peak). */
int mv3d_conv3x3_f32(const void *x_framed, const void *w_packed, const float *bias, void *y, int batch, int height, int width, int c_in,
                     int c_out, int out_framed, int relu, void *stream);
int mv3d_maxpool2x2_f32(const void *x_framed, void *y_framed, int batch, int height, int width, int channels, void *stream);
int mv3d_frame_nhwc_f32(const float *x_nhwc, void *y_framed, int batch, int height, int width, int channels, int channels_out,
                        void *stream);
/* The same three entries on bfloat16 activations / weights (v_mfma_f32_32x32x16_bf16, f32 accumulate): the TRAINING trunk's
 * forward and data-gradient convolutions (mv3d_tf_amd/trunk_train.py) -- f16's 5-bit exponent would need loss scaling. */
int mv3d_conv3x3_bf16(const void *x_framed, const void *w_packed, const float *bias, void *y, int batch, int height, int width,
                      int c_in, int c_out, int out_framed, int out_f32, int relu, void *stream);
/* y = (conv3x3(x) + bias) where gate > 0, else 0: the data-gradient step of the training trunk in one launch (x = the framed gradient
 * of the layer above, w = that layer's filter flipped with its channel axes swapped, gate_framed = this layer's framed ReLU
 * output (batch, height + 2, width + 2, c_out) bf16); framed bf16 output, no ReLU of its own. */
int mv3d_conv3x3_gated_bf16(const void *x_framed, const void *w_packed, const float *bias, const void *gate_framed, void *y,
                            int batch, int height, int width, int c_in, int c_out, void *stream);
int mv3d_maxpool2x2_bf16(const void *x_framed, void *y_framed, int batch, int height, int width, int channels, void *stream);
int mv3d_frame_nhwc_bf16(const float *x_nhwc, void *y_framed, int batch, int height, int width, int channels, int channels_out,
                         void *stream);
/* Gradient of ReLU + max_pool(2, 2, 2, 2, 'VALID') for the training trunk: y_framed = the pre-pool map (a ReLU output),
 * g_pooled_framed = gradient w.r.t. the pooled map -> gy_framed = gradient w.r.t. y's pre-activation (first maximum of the
 * window gets the gradient if it is > 0).  All framed bf16; rows / columns the pool dropped are left untouched (zero). */
int mv3d_maxpool2x2_bwd_bf16(const void *y_framed, const void *g_pooled_framed, void *gy_framed, int batch, int height, int width,
                             int channels, void *stream);
int mv3d_maxpool2x2_bwd_f32(const void *y_framed, const void *g_pooled_framed, void *gy_framed, int batch, int height, int width,
                            int channels, void *stream);      /* the same on f32 maps (the fp32 training trunk) */
/* Several views of ONE layer shape behind one launch (the BEV / image / front-view trunks of lib/networks/MV3D_train.py:44-81 at one
 * VGG depth have the same channel counts and different map sizes): the grid is the concatenation of the views' tiles, so that
 * the small maps of a training batch fill the chip together, on ONE stream.  Same arithmetic per view as the single-view
 * entries above (which are these with num_views = 1).  gate_framed: optional (bf16 / f16, framed 16-bit output only; all views
 * or none) = the ReLU gate of mv3d_conv3x3_gated_bf16; the f32 entry takes an f32 gate (framed f32 output). */
#define MV3D_MAX_CONV_VIEWS 3
typedef struct {
    const void *x_framed;        /* (batch, height + 2, width + 2, c_in) */
    const void *w_packed;        /* (c_out, 9 * c_in), this view's filter */
    const float *bias;           /* (c_out) */
    const void *gate_framed;     /* optional, (batch, height + 2, width + 2, c_out) */
    void *y;                     /* framed (batch, height + 2, width + 2, c_out) or bare (batch, height, width, c_out) */
    int32_t batch, height, width, reserved0;
} mv3d_conv_view;
int mv3d_conv3x3_views_f16(int num_views, const mv3d_conv_view *views, int c_in, int c_out, int out_framed, int out_f32, int relu,
                           void *stream);
int mv3d_conv3x3_views_bf16(int num_views, const mv3d_conv_view *views, int c_in, int c_out, int out_framed, int out_f32, int relu,
                            void *stream);
int mv3d_conv3x3_views_f32(int num_views, const mv3d_conv_view *views, int c_in, int c_out, int out_framed, int relu, void *stream);
/* Convolution + bias + ReLU + the 2x2 / stride 2 VALID max pool that follows it (lib/networks/network.py:182-189) in ONE launch, for
 * layers whose full-size output only the pool reads (the serving graph's conv1_2 / conv2_2 / conv3_3): y = the POOLED framed map
 * (batch, height / 2 + 2, width / 2 + 2, c_out); the full-size map is never written.  Same values as the convolution entry followed
 * by mv3d_maxpool2x2_*. */
int mv3d_conv3x3_pool_views_f16(int num_views, const mv3d_conv_view *views, int c_in, int c_out, void *stream);
int mv3d_conv3x3_pool_views_bf16(int num_views, const mv3d_conv_view *views, int c_in, int c_out, void *stream);
/* Host only (no device, no environment): the name of the kernel path the entries above select for such a launch -- they launch
 * what this very selection returns.  operand_bytes 2 = the f16 / bf16 entries, 4 = the f32 entries (f32 maps out whatever
 * out_f32 says; no pool form); pixels[k] = batch * height * width of view k; gated = a gate_framed is given; pool = the
 * *_pool_views_* entries.  One of "conv_input", "first_128x128", "first_256x64", "64x128", "128x128", "pp", "256x64",
 * "pool_128x128", "pool_256x64", "f32_64x128", "f32_128x128", "f32_128x64" (a static string), or NULL where the entries
 * return MV3D_ERR_INVALID_ARG for the channel counts or the flag combination (or for num_views, a pixel count <= 0). */
const char *mv3d_conv3x3_path(int operand_bytes, int num_views, const int32_t *pixels, int c_in, int c_out, int out_f32, int gated,
                              int pool);
/* The 2x2 pools of several views in one launch.  Forward: x_framed = the map, y_framed = the pooled map (g_pooled_framed unused).
 * Backward (mv3d_maxpool2x2_bwd_*): x_framed = the pre-pool map y, g_pooled_framed = the gradient w.r.t. the pooled map,
 * y_framed = the gradient w.r.t. y's pre-activation (written). */
typedef struct {
    const void *x_framed;
    const void *g_pooled_framed;
    void *y_framed;
    int32_t batch, height, width, reserved0;      /* size of the UNPOOLED map */
} mv3d_pool_view;
int mv3d_maxpool2x2_views_f16(int num_views, const mv3d_pool_view *views, int channels, void *stream);
int mv3d_maxpool2x2_views_bf16(int num_views, const mv3d_pool_view *views, int channels, void *stream);
int mv3d_maxpool2x2_views_f32(int num_views, const mv3d_pool_view *views, int channels, void *stream);
int mv3d_maxpool2x2_bwd_views_bf16(int num_views, const mv3d_pool_view *views, int channels, void *stream);
int mv3d_maxpool2x2_bwd_views_f32(int num_views, const mv3d_pool_view *views, int channels, void *stream);
/* Weight gradient of that convolution (csrc/conv3x3_wgrad.hip): dw (c_out, c_in_real, 3, 3) f32 [the OIHW filter layout; TF's
 * HWIO is its transpose(2, 3, 1, 0)], dw[co][ci][tap] = sum over the pixels of the batch of dy[pixel][co] * x[pixel + tap][ci],
 * for the first c_in_real <= c_in channels (the input layer's buffer is padded to 64 channels); db (c_out) f32 (may be NULL) =
 * the bias gradient, the sum of dy over the pixels, from the same launch; x_framed (batch, height + 2, width + 2, c_in) bf16 = the layer's input,
 * dy_framed (.., c_out) bf16 = the gradient w.r.t. its pre-activation with a ZERO frame; c_in, c_out multiples of 64.
 * workspace: >= mv3d_conv3x3_wgrad_workspace_bytes(...) bytes, 16-byte aligned (split-K partial sums, folded in a fixed order). */
size_t mv3d_conv3x3_wgrad_workspace_bytes(int batch, int height, int width, int c_in, int c_out);
int mv3d_conv3x3_wgrad_bf16(const void *x_framed, const void *dy_framed, float *dw, float *db, int batch, int height, int width,
                            int c_in, int c_in_real, int c_out, void *workspace, size_t workspace_bytes, void *stream);
/* The same on f32 maps (the fp32 training trunk; csrc/conv3x3_wgrad.hip, v_mfma_f32_32x32x2_f32: one ds_read_b32 per operand, no
 * transposing read): exact f32 products and sums, only the summation order differs from any other fp32 weight gradient. */
size_t mv3d_conv3x3_wgrad_f32_workspace_bytes(int batch, int height, int width, int c_in, int c_out);
int mv3d_conv3x3_wgrad_f32(const void *x_framed, const void *dy_framed, float *dw, float *db, int batch, int height, int width,
                           int c_in, int c_in_real, int c_out, void *workspace, size_t workspace_bytes, void *stream);
/* The weight gradients of several views (one filter SHAPE, every view its own maps and its own dw / db: the three trunks at one VGG
 * depth) behind one launch + one reduce launch.  db: NULL in every view or in none.  workspace: >=
 * mv3d_conv3x3_wgrad_views_workspace_bytes(...) bytes (f32_maps: 0 for the bf16 entry, 1 for the f32 one), 16-byte aligned. */
typedef struct {
    const void *x_framed;        /* (batch, height + 2, width + 2, c_in) */
    const void *dy_framed;       /* (batch, height + 2, width + 2, c_out), zero frame */
    float *dw;                   /* (c_out, c_in_real, 3, 3) */
    float *db;                   /* (c_out) or NULL */
    int32_t batch, height, width;
    int32_t c_in_real;           /* this view's real input channels (the input layers: 9 BEV, 3 image / front view); 0 = the call's */
} mv3d_wgrad_view;
size_t mv3d_conv3x3_wgrad_views_workspace_bytes(int num_views, const mv3d_wgrad_view *views, int c_in, int c_out, int f32_maps);
int mv3d_conv3x3_wgrad_views_bf16(int num_views, const mv3d_wgrad_view *views, int c_in, int c_in_real, int c_out, void *workspace,
                                  size_t workspace_bytes, void *stream);
int mv3d_conv3x3_wgrad_views_f32(int num_views, const mv3d_wgrad_view *views, int c_in, int c_in_real, int c_out, void *workspace,
                                 size_t workspace_bytes, void *stream);
/* fp32 OIHW filter (c_out, c_in, 3, 3) -> the packed bf16 forms of one training step in one launch: fwd_packed (c_out, 9 * c_in_pad)
 * [zero-initialised by the caller when c_in_pad > c_in] for mv3d_conv3x3_bf16, dgrad_packed (c_in, 9 * c_out) (may be NULL) for
 * the data-gradient convolution: the filter flipped by 180 degrees with its channel axes swapped. */
int mv3d_conv3x3_pack_bf16(const float *w_oihw, void *fwd_packed, void *dgrad_packed, int c_out, int c_in, int c_in_pad, void *stream);
/* the same for many filters in ONE launch (every 3x3 layer of the training graph at the top of a step) */
typedef struct {
    const float *w_oihw;
    void *fwd_packed, *dgrad_packed;               /* dgrad_packed may be NULL */
    int32_t c_out, c_in, c_in_pad, reserved0;
} mv3d_pack_item;
int mv3d_conv3x3_pack_many_bf16(int num_items, const mv3d_pack_item *items, void *stream);
int mv3d_conv3x3_pack_many_f32(int num_items, const mv3d_pack_item *items, void *stream);    /* f32 packings (c_out % 64 == 0 in both) */
/* framed f16 (batch, height + 2, width + 2, channels) -> framed (batch, height / 2 + 2, width / 2 + 2, channels); channels % 8 == 0 */
int mv3d_maxpool2x2_f16(const void *x_framed, void *y_framed, int batch, int height, int width, int channels, void *stream);
/* NHWC f32 (batch, height, width, channels) -> interior pixels, first `channels` channels of a framed f16 buffer
 * (batch, height + 2, width + 2, channels_out >= channels) */
int mv3d_frame_nhwc_f16(const float *x_nhwc, void *y_framed, int batch, int height, int width, int channels, int channels_out,
                        void *stream);

/* softmax over `rows` rows of `classes` f32 logits (row-major, 8-byte aligned): the RPN's reshape_layer(2) + softmax
 * (lib/networks/network.py:333-341, :399-403) and cls_prob (MV3D_train.py:178); forward only (the losses take the logits). */
int mv3d_softmax_rows(const float *logits_dev, float *prob_dev, long long rows, int classes, void *stream);

/* ------------------------------------------------------------------ the optimizer step (csrc/adam.hip)
 * Replaces tf.train.AdamOptimizer(lr).apply_gradients of lib/fast_rcnn/train_mv.py:138-146 (beta 0.9 / 0.999, eps 1e-8, no weight
 * decay) for ALL parameter tensors behind one launch: per element  m = m + (g - m) (1 - beta1);  v = beta2 v + (1 - beta2) g^2;
 * p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps), f32, in place.
 *   tensors_dev        device array of the tensors (each: f32 param / grad / both moments, numel elements)
 *   chunk_tensor_dev   device int32 [num_chunks]: chunk -> index into tensors_dev
 *   chunk_first_dev    device int32 [num_chunks]: chunk -> its first element / mv3d_adam_chunk_elements() inside that tensor
 *                      (the host cuts every tensor into chunks once; the tables change only with the parameter list)
 *   step               1-based count of this update (the bias corrections)
 *   lowp_dtype         the 16-bit type of the tensors' optional param_lowp copies (what the next step's GEMMs read the weights in) */
typedef struct {
    float *param;
    const float *grad;
    float *exp_avg, *exp_avg_sq;
    long long numel;
    void *param_lowp;            /* NULL, or `numel` 16-bit elements that receive the updated parameter rounded to lowp_dtype */
} mv3d_adam_tensor;
int mv3d_adam_chunk_elements(void);
int mv3d_adam_step(const mv3d_adam_tensor *tensors_dev, const int32_t *chunk_tensor_dev, const int32_t *chunk_first_dev, int num_chunks,
                   double lr, double beta1, double beta2, double eps, int step, int lowp_dtype /* of param_lowp: 0 none, 1 f16, 2 bf16 */,
                   void *stream);

/* ------------------------------------------------------------------ the training solver (csrc/solver.hip, csrc/adam.hip)
 * New here (the reference leaves its MomentumOptimizer, exponential_decay and WEIGHT_DECAY commented out or unread:
 * lib/fast_rcnn/train_mv.py:138-146, lib/fast_rcnn/config.py:38-40): the global gradient norm with a clip coefficient and a
 * non-finite guard that stay on the device, a momentum-SGD step and the Adam step above under the same control.  The chunk tables
 * are those of mv3d_adam_step (mv3d_adam_chunk_elements() elements per chunk).  DESIGN.md section 3.28.
 *
 * mv3d_grad_norm: sumsq = sum over every element of every tensor of (double)g * (double)g -- each square exact in f64, the sum in f64
 * in an order that is a function of the tensors' sizes alone (element i of a chunk always goes to the same thread and the same place
 * in its chain, the threads, waves, chunks' partials are reduced in fixed trees; no floating-point atomics), so neither addresses,
 * alignment nor scheduling move a bit of it.  Two launches: one workgroup per chunk writes partials_dev[chunk], one workgroup of
 * MV3D_GRAD_NORM_FINISH_THREADS reduces them and writes *control_dev:
 *   norm = (float)sqrt(sumsq);  skip = guard && !isfinite(sumsq);
 *   coef = 0 under skip, else 1 if max_norm == 0, else c = max_norm / (sqrt(sumsq) + 1e-6) in f64, coef = c >= 1 ? 1 : (float)c
 *          (torch.nn.utils.clip_grad_norm_'s rule);  skipped_total += skip;  calls_total += 1.
 * num_chunks == 0 writes sumsq 0, coef 1, skip 0.  The caller owns the record, zeroes it once and need never read it: the update
 * launches read coef and skip from the device.
 *
 * mv3d_sgd_step: per element, f32, g' = coef * g (not evaluated when coef == 1 or control_dev is NULL); g' += weight_decay * p (not
 * evaluated when the tensor's weight_decay == 0);  buf = momentum * buf + g';  p -= lr * buf -- torch.optim.SGD's and TensorFlow's
 * MomentumOptimizer's rule (state0 = the momentum buffer, state1 unused).  Under control_dev->skip nothing is written.
 *
 * mv3d_adam_step_ctl: mv3d_adam_step with g replaced by the same g' (state0 = exp_avg, state1 = exp_avg_sq), nothing written under
 * skip.  `step` lives on the host and the host never reads the flag back, so a skipped step still counts as a step for the bias
 * corrections.  With coef == 1, every weight_decay == 0 and skip == 0 the result equals mv3d_adam_step's bit for bit. */
typedef struct {
    float *param;
    const float *grad;
    float *state0, *state1;      /* SGD: momentum buffer, NULL;  Adam: exp_avg, exp_avg_sq */
    long long numel;
    void *param_lowp;            /* as mv3d_adam_tensor.param_lowp */
    float weight_decay;          /* L2 decay of this tensor, added to the gradient; 0 = none */
    int32_t reserved0;
} mv3d_solver_tensor;
typedef struct {
    double sumsq;                /* the squared global gradient norm of the last mv3d_grad_norm */
    float norm, coef;
    int32_t skip;                /* 1: the last norm was non-finite under `guard`; the update launches write nothing */
    int32_t skipped_total, calls_total;
    int32_t reserved0;
} mv3d_step_control;
#define MV3D_GRAD_NORM_FINISH_THREADS 1024
int mv3d_grad_norm(const mv3d_solver_tensor *tensors_dev, const int32_t *chunk_tensor_dev, const int32_t *chunk_first_dev, int num_chunks,
                   double max_norm /* 0 = no clipping */, int guard, double *partials_dev /* [num_chunks] */,
                   mv3d_step_control *control_dev, void *stream);
int mv3d_sgd_step(const mv3d_solver_tensor *tensors_dev, const int32_t *chunk_tensor_dev, const int32_t *chunk_first_dev, int num_chunks,
                  double lr, double momentum, const mv3d_step_control *control_dev /* may be NULL */, int lowp_dtype, void *stream);
int mv3d_adam_step_ctl(const mv3d_solver_tensor *tensors_dev, const int32_t *chunk_tensor_dev, const int32_t *chunk_first_dev,
                       int num_chunks, double lr, double beta1, double beta2, double eps, int step,
                       const mv3d_step_control *control_dev /* may be NULL */, int lowp_dtype, void *stream);

/* ------------------------------------------------------------------ KITTI evaluation (csrc/kitti_eval.hip)
 * Bird's-eye-view and 3D average precision of LIDAR-corner detections over a whole split (new here: the reference writes
 * result files for the KITTI devkit binary, lib/datasets/kitti_mv3d.py:321-352, and never runs it).  Frames are CSR ranges:
 * frame f owns detections det_off[f] .. det_off[f+1]-1, objects gt_off[f] .. gt_off[f+1]-1, and the D_f x G_f row-major
 * pair block pair_off[f] .. pair_off[f] + D_f G_f - 1, pair_off[0] = 0, pair_off[f+1] = pair_off[f] + D_f G_f.
 * det_off / gt_off are HOST arrays, validated before any device call (start at 0, monotone, end at num_dets / num_gts, at
 * most MV3D_KITTI_MAX_DETS detections per frame, sum of D_f G_f == num_pairs < 2^31); offsets_dev holds the same det_off,
 * gt_off and the pair_off above on the device.  Conventions, operation order and launch shapes: DESIGN.md §3.12.
 *   det_cnr_dev    (num_dets, 24) f32 LIDAR corners (x0..x7, y0..y7, z0..z7), det_score_dev (num_dets) f32
 *   calib_dev      (num_frames, 4, 12) f32 calibration tables (P2 | P3 | R0 | Tr_velo_to_cam), for the detections' image height
 *   gt_cnr_dev     (num_gts, 24) f32 LIDAR corners, gt_cls_dev (num_gts) int32 class codes (the caller's numbering),
 *   gt_attr_dev    (num_gts, 4) f32: truncation, occlusion, y1, y2 of the label's image box
 *   img_height     rows of the image the detections' projected boxes are clipped to */
#define MV3D_KITTI_MAX_DETS 2048
#define MV3D_KITTI_NUM_SAMPLE_PTS 41
typedef struct {
    int32_t num_frames, num_dets, num_gts, img_height;
    const int32_t *det_off, *gt_off;     /* host, (num_frames + 1) each */
    const int32_t *offsets_dev;          /* device (3, num_frames + 1): det_off | gt_off | pair_off */
    const float *det_cnr_dev, *det_score_dev, *calib_dev, *gt_cnr_dev;
    const int32_t *gt_cls_dev;
    const float *gt_attr_dev;
} mv3d_kitti_split;
/* iou_dev (2, num_pairs) f64: iou_bev | iou_3d; det_height_dev (num_dets) f64: height of the projected, clipped image box. */
int mv3d_kitti_eval_overlaps(const mv3d_kitti_split *split, long long num_pairs, double *iou_dev, double *det_height_dev,
                             void *stream);
/* Pass 1 of the devkit's statistics (no false positives): matched_dev (2 metrics, 3 difficulties, num_gts) f32 = the score of
 * the detection matched to that object as a true positive, -inf otherwise.  Objects of class eval_class are evaluated, those
 * of neighbor_class ignored, all others skipped; min_overlap >= 0. */
int mv3d_kitti_eval_match(const mv3d_kitti_split *split, long long num_pairs, const double *iou_dev, const double *det_height_dev,
                          int eval_class, int neighbor_class, double min_overlap, float *matched_dev, void *stream);
/* Pass 2: thresholds_dev (2, 3, MV3D_KITTI_NUM_SAMPLE_PTS) f32 score thresholds, num_thresholds_dev (2, 3) int32 (<= 41 used);
 * counts_dev (2, 3, MV3D_KITTI_NUM_SAMPLE_PTS, 3) int32 tp | fp | fn, zeroed by the call, then summed over frames. */
int mv3d_kitti_eval_count(const mv3d_kitti_split *split, long long num_pairs, const double *iou_dev, const double *det_height_dev,
                          int eval_class, int neighbor_class, double min_overlap, const float *thresholds_dev,
                          const int32_t *num_thresholds_dev, int32_t *counts_dev, void *stream);

/* 2D detection and orientation (AP_2D, AOS) of the same split, passed next to it: the label's image boxes and alphas, the
 * frames' DontCare boxes as CSR ranges (frame f owns dc_off[f] .. dc_off[f+1]-1; dc_off is a HOST array, validated like
 * det_off; dc_off_dev the same on the device) and each frame's image shape.  The entries need no pair blocks: split's
 * num_pairs is not used.  Conventions and operation order: the header comment of csrc/kitti_eval.hip, DESIGN.md §3.12.
 *   gt_box_dev       (num_gts, 4) f32 label image box x1, y1, x2, y2; gt_alpha_dev (num_gts) f32 label alpha
 *   dc_box_dev       (num_dontcare, 4) f32 DontCare image boxes
 *   image_shape_dev  (num_frames, 2) int32 rows, columns of the image the detections' boxes are clipped to */
typedef struct {
    int32_t num_dontcare, reserved0;
    const int32_t *dc_off;               /* host, (num_frames + 1) */
    const int32_t *dc_off_dev;           /* device, (num_frames + 1) */
    const float *gt_box_dev, *gt_alpha_dev, *dc_box_dev;
    const int32_t *image_shape_dev;
} mv3d_kitti_image_split;
/* det_box_dev (num_dets, 4) f64 clipped image box of the LIDAR corners (all zeros when it cannot be formed); det_cam_dev
 * (num_dets, 8) f64 camera box h, w, l, x, y, z, ry, alpha. */
int mv3d_kitti_eval_image_boxes(const mv3d_kitti_split *split, const mv3d_kitti_image_split *image, double *det_box_dev,
                                double *det_cam_dev, void *stream);
/* Pass 1 with the 2D IoU: matched_dev (3 difficulties, num_gts) f32, as mv3d_kitti_eval_match. */
int mv3d_kitti_eval_match_2d(const mv3d_kitti_split *split, const mv3d_kitti_image_split *image, const double *det_box_dev,
                             int eval_class, int neighbor_class, double min_overlap, float *matched_dev, void *stream);
/* Pass 2 with the 2D IoU and the DontCare rule: thresholds_dev (3, MV3D_KITTI_NUM_SAMPLE_PTS) f32, num_thresholds_dev (3) int32;
 * counts_dev (3, MV3D_KITTI_NUM_SAMPLE_PTS, 3) int32 tp | fp | fn summed over frames and similarity_dev (num_frames, 3,
 * MV3D_KITTI_NUM_SAMPLE_PTS) f64 per-frame sums of (1 + cos(alpha_gt - alpha_det)) / 2 over the true positives, both zeroed by
 * the call (no float atomics: the caller sums similarity_dev over frames in frame order). */
int mv3d_kitti_eval_count_2d(const mv3d_kitti_split *split, const mv3d_kitti_image_split *image, const double *det_box_dev,
                             const double *det_cam_dev, int eval_class, int neighbor_class, double min_overlap,
                             const float *thresholds_dev, const int32_t *num_thresholds_dev, int32_t *counts_dev,
                             double *similarity_dev, void *stream);

/* ------------------------------------------------------------------ proposal recall (csrc/proposal_recall.hip)
 * lib/datasets/imdb.py:162-196 (evaluate_recall's greedy matching of proposals to objects) over a whole split and several
 * proposal limits in ONE launch.  Frames are CSR ranges: frame f owns boxes box_off[f] .. box_off[f+1]-1 and objects
 * gt_off[f] .. gt_off[f+1]-1.  box_off / gt_off are HOST arrays, validated before any device call (start at 0, monotone, end
 * at num_boxes / num_gts, at most MV3D_RECALL_MAX_GT objects per frame, num_boxes < 2^31); box_off_dev / gt_off_dev hold the
 * same on the device.  Contract and operation order: the header comment of csrc/proposal_recall.hip, DESIGN.md §3.14.
 *   boxes_dev       (num_boxes, 4) f32 x1, y1, x2, y2 in the reference's proposal order; gt_dev (num_gts, 4) f32
 *   limits_dev      (num_limits) int32: only the first limits[l] boxes of every frame are matched, <= 0 means all of them
 *   thresholds_dev  (num_thresholds) f64 IoU thresholds
 *   short_mode      a frame with 0 < n < G_f boxes (the reference fails its assert there): MV3D_RECALL_SHORT_ASSERT sets
 *                   MV3D_RECALL_STATUS_SHORT and records -1.0 for the rounds without a box; MV3D_RECALL_SHORT_ZERO (this
 *                   library's definition, not the reference's) records 0.0 for them and sets nothing */
#define MV3D_RECALL_MAX_GT 256
#define MV3D_RECALL_SHORT_ASSERT 0
#define MV3D_RECALL_SHORT_ZERO 1
#define MV3D_RECALL_STATUS_SHORT 1
#define MV3D_RECALL_STATUS_NONFINITE 2
typedef struct {
    int32_t num_frames, num_gts, num_limits, num_thresholds, short_mode, reserved0;
    long long num_boxes;
    const int32_t *box_off, *gt_off;           /* host, (num_frames + 1) each */
    const int32_t *box_off_dev, *gt_off_dev;   /* device, (num_frames + 1) each */
    const float *boxes_dev, *gt_dev;
    const int32_t *limits_dev;
    const double *thresholds_dev;
} mv3d_recall_split;
/* gt_overlaps_dev (num_limits, num_gts) f64: frame f's block holds the overlap recorded in round j at position gt_off[f] + j
 * (-1.0 throughout for a frame without boxes, which the reference skips); counts_dev (num_limits, num_thresholds) int32: the
 * number of recorded overlaps >= thresholds[t] over the frames that were not skipped, zeroed by the call, integer atomics
 * only; status_dev (num_frames) int32, zeroed by the call: MV3D_RECALL_STATUS_* bits, over all limits.  Asynchronous. */
int mv3d_proposal_recall(const mv3d_recall_split *split, double *gt_overlaps_dev, int32_t *counts_dev, int32_t *status_dev,
                         void *stream);

/* ------------------------------------------------------------------ proposal recall by oriented IoU (csrc/proposal_recall_3d.hip)
 * The same matching with the KITTI evaluator's oriented-box overlap (csrc/box_iou.h) against the objects' LIDAR corners, for the
 * BEV IoU and the 3D IoU at once: MV3D's 3D-proposal recall.  Frames are CSR ranges as above, plus pair_off: frame f's R_f x G_f
 * block of the IoU workspace starts at pair_off[f], pair_off[0] = 0, pair_off[f+1] = pair_off[f] + R_f * G_f.  box_off / gt_off /
 * pair_off are HOST arrays, validated before any device call (start at 0, monotone, end at num_boxes / num_gts / num_pairs, at
 * most MV3D_RECALL_MAX_GT objects per frame, pair_off consistent with the other two, num_boxes and num_pairs < 2^31); the *_dev
 * members hold the same on the device.  Contract and operation order: the header comment of csrc/proposal_recall_3d.hip,
 * DESIGN.md §3.15.
 *   boxes_dev       MV3D_RECALL3D_BOX6: (num_boxes, 6) f32 x, y, z, l, w, h (rois[2][:, 1:7] of the proposal layer);
 *                   MV3D_RECALL3D_CNR24: (num_boxes, 24) f32 x0..7, y0..7, z0..7; in proposal order
 *   gt_cnr_dev      (num_gts, 24) f32 LIDAR corners (the roidb's boxes_corners)
 *   limits_dev, thresholds_dev, short_mode   as in mv3d_recall_split */
#define MV3D_RECALL3D_BOX6 0
#define MV3D_RECALL3D_CNR24 1
typedef struct {
    int32_t num_frames, num_gts, num_limits, num_thresholds, short_mode, box_format;
    long long num_boxes, num_pairs;
    const int32_t *box_off, *gt_off, *pair_off;
    const int32_t *box_off_dev, *gt_off_dev, *pair_off_dev;
    const float *boxes_dev, *gt_cnr_dev;
    const int32_t *limits_dev;
    const double *thresholds_dev;
} mv3d_recall3d_split;
/* bytes of the IoU workspace of a split with num_pairs (proposal, object) pairs: two f64 planes, 16 * num_pairs */
size_t mv3d_proposal_recall_3d_workspace_bytes(long long num_pairs);
/* iou_ws_dev: caller-owned workspace of that many bytes, written in full (no memset needed), plane 0 = BEV IoU, plane 1 = 3D IoU.
 * gt_overlaps_dev (2, num_limits, num_gts) f64, metric 0 = bev, 1 = 3d: frame f's block holds the overlap recorded in round j at
 * position gt_off[f] + j (-1.0 throughout for a frame without proposals); counts_dev (2, num_limits, num_thresholds) int32,
 * zeroed by the call, integer atomics only; status_dev (num_frames) int32, zeroed by the call: MV3D_RECALL_STATUS_* bits, over
 * all limits and both metrics.  Asynchronous; allocates nothing. */
int mv3d_proposal_recall_3d(const mv3d_recall3d_split *split, double *iou_ws_dev, double *gt_overlaps_dev, int32_t *counts_dev,
                            int32_t *status_dev, void *stream);
/* The two launches of mv3d_proposal_recall_3d on their own, with the same validation (tools/proposal_recall_3d_bench.py times them
 * separately; another set of limits can be matched against overlaps that are already there).  _overlaps zeroes status_dev and
 * writes the workspace and the MV3D_RECALL_STATUS_NONFINITE bits; _match zeroes counts_dev, reads both and adds
 * MV3D_RECALL_STATUS_SHORT bits: it must follow an _overlaps call on the same split, workspace and status, on the same stream. */
int mv3d_proposal_recall_3d_overlaps(const mv3d_recall3d_split *split, double *iou_ws_dev, int32_t *status_dev, void *stream);
int mv3d_proposal_recall_3d_match(const mv3d_recall3d_split *split, const double *iou_ws_dev, double *gt_overlaps_dev,
                                  int32_t *counts_dev, int32_t *status_dev, void *stream);

/* ------------------------------------------------------------------ mirrored training frames (cfg.TRAIN.USE_FLIPPED)
 * Left/right mirror of a contiguous (rows, width, channels) f32 array IN PLACE: afterwards data[r][w][c] holds the old
 * data[r][width - 1 - w][c].  No workspace; every element is read once and written once (one thread per pair of mirrored
 * elements), the middle column of an odd width is not touched; width == 1 or rows == 0 launches nothing.  Nothing is assumed
 * about alignment beyond the floats' own (pixels of 3 and 9 channels are 12 and 36 bytes); element offsets are 64-bit, one row
 * (width * channels) must stay below 2^31 elements.  One launch, no allocation or synchronisation.  MV3D_ERR_INVALID_ARG: NULL
 * data with rows > 0, rows < 0, width < 1, channels < 1, or a row of 2^31 elements or more. */
int mv3d_mirror_columns(float *data_dev, long long rows, int width, int channels, void *stream);

/* ------------------------------------------------------------------ image input (csrc/image_blob.hip)
 * `num_frames` uint8 BGR frames of their own sizes -> the (num_frames, canvas_h, canvas_w, 3) f32 blob of the image trunk, mean
 * subtracted, every frame at the top-left corner of a zero canvas (lib/utils/blob.py:14-27, im_list_to_blob), in ONE launch
 * whatever num_frames is.
 *   pixels_dev    uint8: the frames' (h_b, w_b, 3) pixels back to back, total_bytes bytes in all (up to INT_MAX).  Byte alignment
 *                 is all it needs: a frame may start at any byte, and a row is 3 w_b bytes.
 *   frames_dev    (num_frames, 4) int32 ON THE DEVICE, a row is [byte offset, h, w, flip]: under a captured graph the pixels, the
 *                 shapes and the flags may change before every replay (total_bytes, the capacity of pixels_dev, stays).
 *   means3_host   three doubles on the HOST, the per-channel means, read before the call returns
 *   out_dev       (num_frames, canvas_h, canvas_w, 3) f32 contiguous, 4-byte aligned: it may be any run of frames inside a larger
 *                 batch buffer (a 375 x 1242 x 3 frame is 8 mod 16 bytes)
 * For y < h_b and x < w_b: out[b][y][x][c] = (float)((double)src_b[y][x'][c] - means[c]), ONE rounding from f64, with x' = x when
 * flip is 0 and x' = w_b - 1 - x otherwise (the mirror within the frame's own width: mv3d_mirror_columns of the unpadded frame).
 * Every other element of the frame's canvas is +0.0f.  Every element of out is written exactly once, padding included: nothing has
 * to be cleared in front.
 * A table row is used only if offset >= 0, 1 <= h <= canvas_h, 1 <= w <= canvas_w and offset + 3 h w <= total_bytes (in 64 bits);
 * the canvas of any other frame is all zeros and its neighbours are what they would be without it.  No value in frames_dev can make
 * the call read outside pixels_dev[0 : total_bytes] or write outside out.
 * No allocation, no workspace, no host synchronisation; num_frames == 0 returns MV3D_OK without a launch.  MV3D_ERR_INVALID_ARG
 * before any launch: num_frames outside [0, MV3D_IMAGE_MAX_FRAMES], negative total_bytes, a canvas side < 1, a canvas of 2^31
 * elements or more, num_frames * canvas_h above 2^31 - 1 workgroup rows, and with num_frames > 0 a NULL frames_dev, means3_host or
 * out_dev, a NULL pixels_dev with total_bytes > 0, frames_dev or out_dev not 4-byte aligned. */
#define MV3D_IMAGE_MAX_FRAMES 1024
int mv3d_image_blob(const uint8_t *pixels_dev, int total_bytes, const int32_t *frames_dev, int num_frames, const double *means3_host,
                    int canvas_h, int canvas_w, float *out_dev, void *stream);

/* ------------------------------------------------------------------ the deep-fusion join (csrc/fusion_join.hip)
 * The element-wise mean that joins the views after a fully connected layer of the deep-fusion head (MV3D paper §3.3, Fig. 3c), with
 * the layer's ReLU in front and the join's dropout behind, for `paths` networks at once (the main one and the auxiliary paths).
 *   h      (sets_in, views, rows, channels) contiguous, the layer's pre-ReLU output; sets_in = 1 (every path reads the same h) or paths
 *   out    (paths, rows, channels), g_out the same, g_h like h; all in `dtype`: 0 = f32, 1 = f16, 2 = bf16
 *   keep   HOST bytes (paths, views), non-zero = path p reads view v; copied into the kernel's arguments by the call
 *   drop   NULL, or DEVICE bytes (paths, rows, channels), non-zero = the element survives the dropout and is scaled by `scale`
 * Forward, per element, in f32: a_v = x < 0 ? 0 : x (a NaN propagates); s = 0 + a_v over the kept views in ascending v; m = s / n_p
 * (n_p = kept views of the path, a true division); with a mask m = drop ? m * scale : 0; the store rounds to nearest even and writes
 * the type's canonical quiet NaN for a NaN.  A view no path keeps is never read.
 * Backward, per element: t = g_out * (drop ? scale : 0) (g_out without a mask); g = (keep[p][v] && x > 0) ? t / n_p : 0; with
 * sets_in == 1 the paths' g are added to 0 in ascending p by the one thread that owns (v, r, c).  No atomics, no workspace,
 * bit-reproducible; views a path dropped get zeros.
 * One launch each, no allocation, memset or synchronisation (capturable in a graph).  16-byte vector accesses when rows * channels is a
 * multiple of the vector width (4 f32, 8 16-bit elements) and the buffers are 16-byte aligned (drop: 4 / 8 bytes).  Otherwise the
 * WHOLE launch runs with scalar accesses -- there is no vector body with a scalar tail: the planes of h, out and the mask start at
 * multiples of rows * channels, so with an odd product they are misaligned against each other and no element range is 16-byte aligned
 * in all of them.  Expect several times less bandwidth there; the head's planes (channels = 2048) always vectorise.  Offsets are 64-bit.  rows == 0 launches nothing.  MV3D_ERR_INVALID_ARG before any HIP call: dtype outside 0..2, views
 * outside 1..4, paths outside 1..8, sets_in not 1 or paths, rows < 0, channels < 1, rows * channels > 2^48, keep NULL, a path that
 * keeps no view, or a NULL buffer (drop excepted) with rows > 0. */
int mv3d_fusion_join_forward(const void *h_dev, int dtype, int sets_in, int paths, int views, int rows, int channels,
                             const uint8_t *keep, const uint8_t *drop_dev, float scale, void *out_dev, void *stream);
int mv3d_fusion_join_backward(const void *h_dev, const void *g_out_dev, int dtype, int sets_in, int paths, int views, int rows,
                              int channels, const uint8_t *keep, const uint8_t *drop_dev, float scale, void *g_h_dev, void *stream);

/* ------------------------------------------------------------------ upsampled ROI features (csrc/upsample.hip)
 * Bilinear upsampling of a feature map by an integer factor s = 2 or 4 in front of RoiPool (MV3D paper §3.2), for up to
 * MV3D_MAX_ROI_VIEWS views in ONE launch (the views' workgroups share the grid).  x (batch, height, width, channels) ->
 * y (batch, s*height, s*width, channels).
 * The coordinate rule is TensorFlow 1's resize_bilinear(align_corners=False): up-pixel o sits at source coordinate o / s.  Up-pixel
 * s*i therefore IS source pixel i -- RoiPool's own convention (feature pixel i <-> input coordinate i / scale) -- and the ROI scale
 * after the upsampling is s / 8 with no half-pixel shift.  (NOT the half-pixel rule of torch's F.interpolate.)
 * Per axis of n source pixels, up-index o has the taps i0 = o / s with weight (s - o % s) / s and i1 = min(i0 + 1, n - 1) with weight
 * (o % s) / s.  A tap of weight 0 is dropped: its value never enters the arithmetic, so a NaN or Inf neighbour does not reach an
 * aligned up-pixel.  Two taps on the same source index (the clamped last rows and columns) merge into one tap of weight 1.  So every
 * up-index has one tap of weight 1, or two taps with dyadic weights.
 * Forward, per channel, in f32 with every operation rounded on its own (no contraction): horizontally first, on each of the one or
 * two source rows: t = a (one tap) or t = fadd(fmul(w0, a), fmul(w1, b)) (two taps); then the same rule vertically on the one or two
 * t.  f16 / bf16 inputs are converted to f32 first (exact); the output is f32.
 * Backward, the exact transpose: g_x[iy][ix] = sum of fmul(W, g_y[oy][ox]) over the up-pixels that have a tap on (iy, ix), W = wy * wx
 * (exact in f32), the terms added to 0.0f in raster order (oy ascending, then ox ascending) -- at most (2s - 1)^2 of them -- by the one
 * thread that owns the element.  No atomics, no workspace, bit-reproducible; every element of g_x is written.
 *   in       forward: x in `dtype` (0 = f32, 1 = f16, 2 = bf16, the numbering of mv3d_fusion_join_*), addressed through the strides;
 *            backward: g_y (batch, s*height, s*width, channels) contiguous f32 (dtype must be 0, the strides are ignored)
 *   out      forward: y contiguous f32; backward: g_x (batch, height, width, channels) contiguous f32
 *   frame_stride, row_stride, pixel_stride   of `in`, in ELEMENTS (forward): the interior of a framed 16-bit map is read where it lies
 * One launch each, no allocation, memset or synchronisation (capturable in a graph); 64-bit element offsets.  A view whose channel
 * count is a multiple of the vector width (4 f32, 8 16-bit elements) and whose pointers and strides are 16-byte aligned moves 16 bytes
 * per lane; otherwise the WHOLE view runs with scalar accesses (no vector body with a scalar tail).  batch == 0 in a view launches
 * nothing for it.  MV3D_ERR_INVALID_ARG before any HIP call: num_views outside 1..MV3D_MAX_ROI_VIEWS or NULL views; dtype outside
 * 0..2 (backward: not 0), a factor other than 2 or 4; batch < 0, height, width or channels < 1; (forward) a pixel stride < channels,
 * a row stride < width * pixel stride or a frame stride < height * row stride; an up-map of 2^31 elements per frame or more; a NULL
 * buffer with batch > 0. */
typedef struct {
    const void *in;
    void *out;
    int64_t frame_stride, row_stride, pixel_stride;
    int32_t dtype, batch, height, width, channels, factor;
} mv3d_upsample_view;
int mv3d_upsample_bilinear_views(int num_views, const mv3d_upsample_view *views, void *stream);
int mv3d_upsample_bilinear_backward_views(int num_views, const mv3d_upsample_view *views, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MV3D_HIP_H */
