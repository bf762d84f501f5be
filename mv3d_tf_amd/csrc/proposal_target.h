// proposal_target_layer_3d's argument blocks, workspace layout and the emit body (proposal_target.hip has the kernels and the
// C-ABI; train_stream.hip runs pt_emit_body side by side with anchor_target.h's at_emit_relabel_body in one grid -- see there
// why the bodies are __device__ functions of a header).
#pragma once
#include "geometry.h"
#include "front_view.h"

struct PtDev {
    const float *rois_bv, *rois_3d;      // (R,5), (R,7)
    const float *gt_bv, *gt_3d;          // (G,5), (G,7)
    int R, G;
    const int32_t *R_dev;                // optional: the proposals' number lives on the device (<= R = the capacity)
    float gt_frame;                      // batch column of the appended ground-truth rows (0 in the reference)
    double fg_thresh, bg_hi, bg_lo;
    double *max_ov;                      // (R+G)
    int32_t *assign;                     // (R+G)
    int32_t *fg_list, *bg_list;          // (R+G) each
};

struct PtEmit {
    const int32_t *fg_pick, *bg_pick;    // positions in the fg / bg lists
    int n_fg, n_bg, num_classes;
    const float *gt_corners, *calib;     // (G,25), (4,12)
    float *rois_bv, *rois_img, *targets, *rois_3d;
    float *rois_fv;                      // third view's ROIs (front_view.hip), NULL = not wanted
    int32_t *labels;
};

// frames of a batch behind one launch of every kernel: blockIdx.y = frame
#define PT_MAX_BATCH 16
struct PtFrame { PtDev d; PtEmit e; int32_t *counts; };
struct PtBatch { PtFrame f[PT_MAX_BATCH]; };

// What pt_emit_body reads of a frame (a kernel that carries another body's arguments as well passes only this)
struct PtEmitFrame {
    const float *rois_bv, *rois_3d, *gt_bv, *gt_3d;
    const int32_t *R_dev, *assign, *fg_list, *bg_list;
    int R;
    float gt_frame;
    PtEmit e;
};
__host__ __device__ __forceinline__ PtEmitFrame pt_emit_frame(const PtFrame &F)
{
    const PtDev &d = F.d;
    return PtEmitFrame{d.rois_bv, d.rois_3d, d.gt_bv, d.gt_3d, d.R_dev, d.assign, d.fg_list, d.bg_list, d.R, d.gt_frame, F.e};
}

// Stage 1's reports as the host reads them, written by pt_compact_kernel's workgroup of frame b next to the device copies
// (pinned buffers mapped into the device; h_report NULL: no mirrors).  The workgroup runs behind everything the reports hold:
// the anchor report of frame b (`report`, written by an earlier launch), its own counts, and the proposal layer's count and
// status word of the frame (num_proposals[b], num_proposals[batch + b]).
struct PtMirror {
    const uint8_t *report;               // (batch, report_row) device
    uint8_t *h_report;                   // (batch, h_row): the first h_row bytes of every row, in 16-byte stores
    size_t report_row, h_row;            // h_row a multiple of 16, both buffers 16-byte aligned
    int32_t *h_pt_counts;                // (batch, 4)
    const int32_t *num_proposals;        // (2, batch) device
    int32_t *h_num_proposals;            // (2, batch)
    int batch;
};

// row r of the candidate set: proposals then ground truth with a 0 batch column (:38-44); a batched caller sets
// params.frame_index so that the ground-truth rows of frame b carry b like the frame's proposals do
template <typename D> __device__ __forceinline__ int pt_num_rois(const D &d) { return d.R_dev ? min(max(*d.R_dev, 0), d.R) : d.R; }
template <typename D> __device__ __forceinline__ void cand_bv(const D &d, const int R, int r, float o[5])
{
    if (r < R) { for (int j = 0; j < 5; ++j) o[j] = d.rois_bv[5 * r + j]; }
    else { o[0] = d.gt_frame; for (int j = 0; j < 4; ++j) o[1 + j] = d.gt_bv[5 * (r - R) + j]; }
}
template <typename D> __device__ __forceinline__ void cand_3d(const D &d, const int R, int r, float o[7])
{
    if (r < R) { for (int j = 0; j < 7; ++j) o[j] = d.rois_3d[7 * r + j]; }
    else { o[0] = d.gt_frame; for (int j = 0; j < 6; ++j) o[1 + j] = d.gt_3d[7 * (r - R) + j]; }
}

// Eight lanes per sampled ROI (lane k of the group = corner k): the f64 projections of the 8 corners (image box, and the
// front-view box when asked for) run side by side and are folded by the same first-extreme-wins scan as the one-thread
// loops of image_box() / rois_3d_to_fv_kernel; one wave per 8 ROIs instead of 64 puts the ~2 k dependent f64 instructions
// of a ROI on eight times as many SIMDs (the kernel was a single-wave latency chain: 10 us for 256 ROIs).
// PT_EMIT_THREADS threads of workgroup wg (no barrier inside: a larger workgroup's other waves may return before the call).
#define PT_EMIT_THREADS 128
__device__ __forceinline__ void pt_emit_body(const PtEmitFrame &d, const int wg)
{
    const PtEmit &e = d.e;
    const int gid = wg * PT_EMIT_THREADS + threadIdx.x;
    const int t = gid >> 3, k = gid & 7;
    const int lane_base = (threadIdx.x & 63) & ~7;
    const int S = e.n_fg + e.n_bg;
    if (t >= S) return;
    // keep_inds = append(fg_inds, bg_inds) (:272)
    const int r = (t < e.n_fg) ? d.fg_list[e.fg_pick[t]] : d.bg_list[e.bg_pick[t - e.n_fg]];
    const int g = d.assign[r];
    // labels = gt_boxes_bv[gt_assignment, 4]; labels[fg_rois_per_this_image:] = 0 (:238, :276)
    const float lab = (t < e.n_fg) ? d.gt_bv[5 * g + 4] : 0.0f;
    float b[5], q[7];
    const int R = pt_num_rois(d);
    cand_bv(d, R, r, b);
    cand_3d(d, R, r, q);
    if (k == 0) {
        for (int j = 0; j < 5; ++j) e.rois_bv[5 * t + j] = b[j];
        for (int j = 0; j < 7; ++j) e.rois_3d[7 * t + j] = q[j];
        e.labels[t] = (int32_t)lab;
    }
    // lidar_3d_to_corners (transform.py:290-315), f32: this lane's corner
    const float *P = q + 1;
    float cx, cy, cz;
    box_corner(P, k, cx, cy, cz);
    // bbox_transform_cnr (bbox_transform.py:61-72): f32; diag = sqrt((d0^2 + d1^2) + d2^2)
    const float *gc = e.gt_corners + 25 * g;
    const float d0 = gc[0] - gc[6], d1 = gc[8] - gc[14], d2 = gc[16] - gc[22];
    float ss = __fmul_rn(d0, d0);
    ss = __fadd_rn(ss, __fmul_rn(d1, d1));
    ss = __fadd_rn(ss, __fmul_rn(d2, d2));
    const float diag = sqrtf(ss);   // IEEE (correctly rounded) sqrt; __fsqrt_rn is the native approximation in HIP
    // _get_bbox_regression_labels_3d (:172-194): class slot, zeros elsewhere; lane k owns columns k, 8 + k, 16 + k of a slot
    const int nc = e.num_classes;
    float *T = e.targets + (long long)t * 24 * nc;
    const int cls = (int)(unsigned short)lab;           // np.array(..., dtype=np.uint16)
    for (int c = 0; c < nc; ++c) {
        const bool own = (c == cls) && cls > 0;
        T[24 * c + k] = own ? __fdiv_rn(gc[k] - cx, diag) : 0.0f;
        T[24 * c + 8 + k] = own ? __fdiv_rn(gc[8 + k] - cy, diag) : 0.0f;
        T[24 * c + 16 + k] = own ? __fdiv_rn(gc[16 + k] - cz, diag) : 0.0f;
    }
    // lidar_cnr_to_img (transform.py:483-500); first column = the ROI's batch index (:76)
    float M[12];
    proj_matrix(e.calib, M);
    double px, py;
    image_point(M, cx, cy, cz, px, py);
    double xmin, xmax, ymin, ymax;
    bool nanx, nany;
    group8_minmax(px, lane_base, xmin, xmax, nanx);
    group8_minmax(py, lane_base, ymin, ymax, nany);
    if (nanx) xmin = xmax = NAN;
    if (nany) ymin = ymax = NAN;
    if (k == 0) {
        e.rois_img[5 * t] = b[0];
        e.rois_img[5 * t + 1] = (float)f64_to_i32(xmin); e.rois_img[5 * t + 2] = (float)f64_to_i32(ymin);
        e.rois_img[5 * t + 3] = (float)f64_to_i32(xmax); e.rois_img[5 * t + 4] = (float)f64_to_i32(ymax);
    }
    if (e.rois_fv) {      // (workgroup-uniform) the third view's ROI: front_view.hip, same arithmetic per corner
        double col, row;
        fv_point((double)cx, (double)cy, (double)cz, col, row);
        double cmin, cmax, rmin, rmax;
        bool nc_, nr_;
        group8_minmax(col, lane_base, cmin, cmax, nc_);
        group8_minmax(row, lane_base, rmin, rmax, nr_);
        if (nc_ || nr_) cmin = cmax = rmin = rmax = NAN;
        if (k == 0) {
            float *o = e.rois_fv + 5 * (long long)t;
            o[0] = q[0];
            o[1] = fv_clip(cmin, FV_W - 1.0); o[2] = fv_clip(rmin, FV_H - 1.0);
            o[3] = fv_clip(cmax, FV_W - 1.0); o[4] = fv_clip(rmax, FV_H - 1.0);
        }
    }
}

struct PtLayout { size_t o_maxov, o_assign, o_fg, o_bg, total; };
static inline bool pt_layout(int R, int G, PtLayout &L)
{
    if (R < 0 || G <= 0 || G > TARGET_MAX_GT || (long long)R + G > (1 << 22)) return false;
    const size_t n = (size_t)R + G;
    size_t o = 0;
    L.o_maxov = o; o += mv3d_align_up(n * 8);
    L.o_assign = o; o += mv3d_align_up(n * 4);
    L.o_fg = o; o += mv3d_align_up(n * 4);
    L.o_bg = o; o += mv3d_align_up(n * 4);
    L.total = o;
    return true;
}

static inline void pt_fill(PtDev &d, const PtLayout &L, char *ws, const float *rois_bv, const float *rois_3d, int R,
                           const float *gt_bv, const float *gt_3d, int G, const mv3d_proposal_target_params *p)
{
    d.rois_bv = rois_bv; d.rois_3d = rois_3d; d.gt_bv = gt_bv; d.gt_3d = gt_3d; d.R = R; d.G = G; d.R_dev = nullptr;
    d.fg_thresh = p->fg_thresh; d.bg_hi = p->bg_thresh_hi; d.bg_lo = p->bg_thresh_lo; d.gt_frame = (float)p->frame_index;
    d.max_ov = (double *)(ws + L.o_maxov); d.assign = (int32_t *)(ws + L.o_assign);
    d.fg_list = (int32_t *)(ws + L.o_fg); d.bg_list = (int32_t *)(ws + L.o_bg);
}

// the argument block of stage 2 from the arguments of mv3d_proposal_target_stage2_batch[_devn] (checked here); `most` = the
// longest frame's sampled ROIs (0: nothing to emit)
static inline int pt_stage2_args(int batch, const float *const *rois_bv_dev, const float *const *rois_3d_dev, const int *num_rois,
                                 const int32_t *const *num_rois_dev, const float *const *gt_bv_dev, const float *const *gt_3d_dev,
                                 const float *const *gt_corners_dev, const int *G, const float *const *calib_dev,
                                 const mv3d_proposal_target_params *p, const int32_t *const *fg_pick_dev, const int *n_fg,
                                 const int32_t *const *bg_pick_dev, const int *n_bg, float *const *rois_bv_out,
                                 float *const *rois_img_out, int32_t *const *labels_out, float *const *bbox_targets_out,
                                 float *const *rois_3d_out, float *const *rois_fv_out, void *const *workspace,
                                 const size_t *workspace_bytes, PtBatch &bt, int &most)
{
    if (batch <= 0 || batch > PT_MAX_BATCH || !p || !num_rois || !G || !n_fg || !n_bg || !workspace || !workspace_bytes)
        return MV3D_ERR_INVALID_ARG;
    bt = PtBatch{};
    most = 0;
    for (int b = 0; b < batch; ++b) {
        PtLayout L;
        if (!pt_layout(num_rois[b], G[b], L) || n_fg[b] < 0 || n_bg[b] < 0 || p[b].num_classes <= 0) return MV3D_ERR_INVALID_ARG;
        PtEmit &e = bt.f[b].e;
        e.n_fg = n_fg[b]; e.n_bg = n_bg[b]; e.num_classes = p[b].num_classes;
        if (n_fg[b] + n_bg[b] == 0) continue;
        if (!gt_bv_dev[b] || !gt_3d_dev[b] || !gt_corners_dev[b] || !calib_dev[b] || (n_fg[b] && !fg_pick_dev[b]) ||
            (n_bg[b] && !bg_pick_dev[b]) || !rois_bv_out[b] || !rois_img_out[b] || !labels_out[b] || !bbox_targets_out[b] ||
            !rois_3d_out[b])
            return MV3D_ERR_INVALID_ARG;
        if (!workspace[b] || workspace_bytes[b] < L.total || ((uintptr_t)workspace[b] % MV3D_ALIGN)) return MV3D_ERR_WORKSPACE;
        pt_fill(bt.f[b].d, L, (char *)workspace[b], rois_bv_dev[b], rois_3d_dev[b], num_rois[b], gt_bv_dev[b], gt_3d_dev[b], G[b], &p[b]);
        bt.f[b].d.R_dev = num_rois_dev ? num_rois_dev[b] : nullptr;
        e.fg_pick = fg_pick_dev[b]; e.bg_pick = bg_pick_dev[b];
        e.gt_corners = gt_corners_dev[b]; e.calib = calib_dev[b];
        e.rois_bv = rois_bv_out[b]; e.rois_img = rois_img_out[b]; e.targets = bbox_targets_out[b]; e.rois_3d = rois_3d_out[b];
        e.labels = labels_out[b];
        e.rois_fv = rois_fv_out ? rois_fv_out[b] : nullptr;
        if (n_fg[b] + n_bg[b] > most) most = n_fg[b] + n_bg[b];
    }
    return MV3D_OK;
}
static inline int pt_emit_workgroups(int most) { return (most * 8 + PT_EMIT_THREADS - 1) / PT_EMIT_THREADS; }

// mv3d_proposal_target_stage1_batch_devn with the reports' host mirrors written by the compaction launch (train_stream.hip)
int mv3d_pt_stage1_batch_mirrored(int batch, const float *const *rois_bv_dev, const float *const *rois_3d_dev, const int *num_rois_cap,
                                  const int32_t *const *num_rois_dev, const float *const *gt_bv_dev, const float *const *gt_3d_dev,
                                  const int *G, const mv3d_proposal_target_params *p, int32_t *const *counts_dev, void *const *workspace,
                                  const size_t *workspace_bytes, const PtMirror &mirror, void *stream);
