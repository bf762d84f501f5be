// The test-time tail with ORIENTED NMS: detect_post's score cut, order, outputs and cap, with the greedy
// suppression judged by the IoU of the boxes' BEV footprints (the evaluator's polygon clip, box_iou.h) instead of the IoU of the
// axis-aligned pixel boxes.  The clip needs 32 KiB of LDS per wave, so it cannot sit in detect_post_nms_kernel's 16 waves; this is
// the three-step NMS instead, kernel launches only:
//
//   detect_post_oriented_order_kernel   grid (K - 1, batch), 1024 threads: steps 1-2 of detect_post (dp_sort_candidates); the
//       sorted source rows and their footprint extents go to the workspace, nc (the number of candidates) too; a candidate with a
//       non-finite footprint value sets MV3D_DETECT_STATUS_NONFINITE in status[f].
//   detect_post_oriented_mask_kernel    grid (tiles ti <= tj, batch, K - 1), ONE wave per workgroup: the 64 x 64 tile of sorted
//       positions (i in block ti, j in block tj, i < j < nc).  Extent pretest on every pair; the pairs that pass are queued in LDS
//       (ballot + prefix count) and clipped a full wave at a time; bit (j % 64) of mask[i][tj] = "i suppresses j".  Every row
//       i < nc of the tile writes its word, whatever it holds; a tile with 64 * tj >= nc returns at once (uniform).
//   detect_post_oriented_reduce_kernel  grid (K, batch), 256 threads: blocks of 64 sorted positions in order.  The block's rows of
//       the mask (words tb .. last) are staged in LDS (the next block's are already in flight in registers); wave 0 settles the
//       block's own 64 x 64 triangle out of registers (lane i holds the diagonal word of row i; one readlane per KEPT row), then
//       lane w ORs the kept rows' words w into its word of the removed set.  Position i is kept iff no kept k < i has bit i set.
//       Then step 5 of detect_post (dp_emit), and detect_post_cap_kernel unchanged.
//
// Contract (tests/oriented_nms_restatement.py follows it line by line):
//   candidates, order   detect_post's: rows r < min(num_rois[f], cap) with cls_prob[r, j] > score_thresh in f32, descending score,
//                       equal scores by larger row, +-0 one score.
//   footprint of row r  24 f32 x0..7, y0..7, z0..7: footprint_source 0 = corners[r], 1 = pred_cnr_r[r, 24j : 24j + 24]; the polygon
//                       is vertices k = 0..3.
//   overlap of (earlier a, later b) in sorted order:
//     1. f64 min / max of x and of y over k = 0..3: start from k = 0, then strict < / >.
//     2. a.maxx < b.minx || b.maxx < a.minx || a.maxy < b.miny || b.maxy < a.miny: IoU = 0.0, nothing else runs.
//     3. otherwise ke_load(a), ke_load(b), and if both are finite ke_iou(a, b): a is the polygon, b the clipper; iou_bev is used.
//        A non-finite box has IoU 0.0 with everything: it is kept and suppresses nothing.
//   suppression         in f64 against nms_thresh: nms_strict_gt 0: iou_bev >= nms_thresh; 1: iou_bev > nms_thresh.
//   status              bit MV3D_DETECT_STATUS_NONFINITE where a candidate (of any class) has a non-finite value among the 24 of
//                       its footprint; bit 0 is never set (ke_iou gives 0.0 for a non-positive union).
//   outputs, cap        detect_post's, bit for bit.
// The overlap is a pure function of the two rows, so the mask of ALL pairs i < j reduces to the same kept set as the greedy walk.
// Extents are kept as f32 (the minimum of f32 values converted to f64 is the converted f32 minimum).
//
// Workspace (never memset; the reduce step reads only what the two steps before it wrote), per (frame, foreground class) fc and
// capp = cap rounded up to 64, W = capp / 64:  nc[fc] i32 | order[fc][capp] i32 | ext[fc][capp] float4 | mask[fc][capp][W] u64,
// each part at 256-B granularity.  No workgroup waits on another; every loop bound is nc <= cap or a host-validated count.
#include "detect_post.h"
#include "box_iou.h"

#define DPO_QUEUE 128             // queued pair indices: drained whenever 64 are waiting, so never more than 127
#define DPO_REDUCE_THREADS 256
#define DPO_MAX_WORDS (DP_MAX_ROWS / 64)
#define DPO_STAGE (64 * DPO_MAX_WORDS / DPO_REDUCE_THREADS)      // mask words a reduce thread stages per block

struct OrientedDev {
    DetectPostDev d;
    const float *foot;            // footprint of row r, class j: foot + r * foot_stride + j * foot_class_stride, 24 floats
    int foot_stride, foot_class_stride;
    int capp, W, strict;
    double thresh;
    int32_t *nc, *order;
    float4 *ext;
    unsigned long long *mask;
};

// step 1: (minx, maxx, miny, maxy) over the footprint vertices
__device__ __forceinline__ float4 dpo_extent(const float c[24])
{
    float lox = c[0], hix = c[0], loy = c[8], hiy = c[8];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        if (c[k] < lox) lox = c[k];
        if (c[k] > hix) hix = c[k];
        if (c[8 + k] < loy) loy = c[8 + k];
        if (c[8 + k] > hiy) hiy = c[8 + k];
    }
    return make_float4(lox, hix, loy, hiy);
}

__device__ __forceinline__ const float *dpo_foot(const OrientedDev &o, long long row0, int row, int j)
{
    return o.foot + (row0 + row) * o.foot_stride + (long long)j * o.foot_class_stride;
}

__global__ __launch_bounds__(DP_THREADS) void detect_post_oriented_order_kernel(const OrientedDev o)
{
    __shared__ unsigned long long s_sort[DP_MAX_ROWS];
    __shared__ int s_nc;
    const int j = blockIdx.x + 1, f = blockIdx.y, t = threadIdx.x;
    const int nc = dp_sort_candidates(o.d, j, f, s_sort, &s_nc);
    const long long fc = (long long)f * (o.d.K - 1) + (j - 1), row0 = (long long)f * o.d.cap;
    if (t == 0) o.nc[fc] = nc;
    bool bad = false;
    for (int p = t; p < nc; p += DP_THREADS) {
        const int row = (int)(unsigned)s_sort[p];
        const float *q = dpo_foot(o, row0, row, j);
        float c[24];
#pragma unroll
        for (int k = 0; k < 24; ++k) { c[k] = q[k]; bad = bad || !isfinite(c[k]); }
        o.order[fc * o.capp + p] = row;
        o.ext[fc * o.capp + p] = dpo_extent(c);
    }
    if (__any(bad) && (t & 63) == 0) atomicOr(&o.d.status[f], MV3D_DETECT_STATUS_NONFINITE);
}

__global__ __launch_bounds__(KE_OVERLAP_THREADS) void detect_post_oriented_mask_kernel(const OrientedDev o)
{
    __shared__ double poly[2 * KE_MAXV * 2 * KE_OVERLAP_THREADS];
    __shared__ float4 s_ea[64], s_eb[64];
    __shared__ int s_ra[64], s_rb[64];
    __shared__ int s_queue[DPO_QUEUE];
    __shared__ unsigned long long s_word[64];

    const int lane = threadIdx.x, f = blockIdx.y, j = blockIdx.z + 1;
    int ti = 0, rest = blockIdx.x;                          // tile (ti <= tj) of the upper triangle, row by row
    while (rest >= o.W - ti) { rest -= o.W - ti; ++ti; }
    const int tj = ti + rest;
    const long long fc = (long long)f * (o.d.K - 1) + (j - 1), row0 = (long long)f * o.d.cap;
    const int nc = o.nc[fc];
    if (64 * tj >= nc) return;                              // (uniform; ti <= tj, so the tile's first row is checked with it)

    const int pa = 64 * ti + lane, pb = 64 * tj + lane;     // this lane's row position / column position
    s_word[lane] = 0ull;
    if (pa < nc) { s_ea[lane] = o.ext[fc * o.capp + pa]; s_ra[lane] = o.order[fc * o.capp + pa]; }
    if (pb < nc) { s_eb[lane] = o.ext[fc * o.capp + pb]; s_rb[lane] = o.order[fc * o.capp + pb]; }
    __syncthreads();
    const int rows = nc - 64 * ti < 64 ? nc - 64 * ti : 64;
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);             // x = minx, y = maxx, z = miny, w = maxy
    if (pb < nc) b = s_eb[lane];

    auto clip = [&](int p) {
        const int r = p >> 6, c = p & 63;
        const float *qa = dpo_foot(o, row0, s_ra[r], j), *qb = dpo_foot(o, row0, s_rb[c], j);
        float ca[24], cb[24];
#pragma unroll
        for (int k = 0; k < 24; ++k) { ca[k] = qa[k]; cb[k] = qb[k]; }
        KeBox A, B;
        const bool fa = ke_load(ca, A);
        const bool fb = ke_load(cb, B);
        if (fa && fb) {
            double ib = 0.0, i3 = 0.0;
            ke_iou(A, B, poly, lane, ib, i3);
            if (o.strict ? (ib > o.thresh) : (ib >= o.thresh)) atomicOr(&s_word[r], 1ull << c);
        }
    };
    int queued = 0;                                         // (uniform)
    for (int r = 0; r < rows; ++r) {
        bool pass = false;
        if (pb < nc && 64 * ti + r < pb) {
            const float4 a = s_ea[r];
            pass = !((double)a.y < (double)b.x || (double)b.y < (double)a.x || (double)a.w < (double)b.z || (double)b.w < (double)a.z);
        }
        const unsigned long long m = __ballot(pass);
        if (m == 0ull) continue;                            // (uniform: nothing was queued, nothing to publish)
        if (pass) s_queue[queued + __popcll(m & ((1ull << lane) - 1ull))] = 64 * r + lane;
        queued += __popcll(m);
        __syncthreads();
        if (queued >= KE_OVERLAP_THREADS) {                 // a full wave of pairs is waiting
            clip(s_queue[lane]);
            const int left = queued - KE_OVERLAP_THREADS;
            const int moved = lane < left ? s_queue[KE_OVERLAP_THREADS + lane] : 0;
            __syncthreads();
            if (lane < left) s_queue[lane] = moved;
            queued = left;
            __syncthreads();
        }
    }
    if (lane < queued) clip(s_queue[lane]);
    __syncthreads();
    if (pa < nc) o.mask[(fc * o.capp + pa) * o.W + tj] = s_word[lane];
}

// lane l's value of v; l is uniform
__device__ __forceinline__ unsigned long long dpo_readlane(unsigned long long v, int l)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(DPO_REDUCE_THREADS) void detect_post_oriented_reduce_kernel(const OrientedDev o)
{
    __shared__ unsigned long long s_rows[64 * DPO_MAX_WORDS];        // [row of the block][word], 16 KiB
    __shared__ int s_order[DP_MAX_ROWS];
    __shared__ unsigned long long s_kmask[DPO_MAX_WORDS];
    __shared__ unsigned short s_kpos[DP_MAX_ROWS];
    const int j = blockIdx.x, f = blockIdx.y, t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    if (j == 0) {                                            // background: no detections
        if (t == 0) o.d.det_count[(long long)f * o.d.K] = 0;
        return;
    }
    const long long fc = (long long)f * (o.d.K - 1) + (j - 1);
    const int nc = o.nc[fc], nblk = (nc + 63) >> 6;
    for (int p = t; p < nc; p += DPO_REDUCE_THREADS) s_order[p] = o.order[fc * o.capp + p];

    // the words [tb, nblk) of the rows of block tb that are < nc: exactly what the mask kernel wrote of them; 0 elsewhere
    unsigned long long pre[DPO_STAGE];
    auto fetch = [&](int tb) {
#pragma unroll
        for (int k = 0; k < DPO_STAGE; ++k) {
            const int e = t + DPO_REDUCE_THREADS * k, i = e / DPO_MAX_WORDS, w = e % DPO_MAX_WORDS;
            pre[k] = (w >= tb && w < nblk && 64 * tb + i < nc) ? o.mask[(fc * o.capp + 64 * tb + i) * o.W + w] : 0ull;
        }
    };
    if (nblk > 0) fetch(0);
    unsigned long long removed = 0ull;                       // wave 0, lane w < 32: word w of the removed set
    for (int tb = 0; tb < nblk; ++tb) {
#pragma unroll
        for (int k = 0; k < DPO_STAGE; ++k) s_rows[t + DPO_REDUCE_THREADS * k] = pre[k];
        __syncthreads();
        if (tb + 1 < nblk) fetch(tb + 1);
        if (wave == 0) {
            const unsigned long long diag = s_rows[lane * DPO_MAX_WORDS + tb];
            unsigned long long cur = dpo_readlane(removed, tb), kept = 0ull;
            const int rows = nc - 64 * tb < 64 ? nc - 64 * tb : 64;
            for (int i = 0; i < rows; ++i) {
                if ((cur >> i) & 1ull) continue;
                kept |= 1ull << i;
                cur |= dpo_readlane(diag, i);
            }
            unsigned long long m = kept;
            while (m) {
                const int i = __builtin_ctzll(m);
                m &= m - 1ull;
                if (lane < DPO_MAX_WORDS) removed |= s_rows[i * DPO_MAX_WORDS + lane];
            }
            if (lane == 0) s_kmask[tb] = kept;
        }
        __syncthreads();
    }
    __syncthreads();                                         // (s_order, for nblk == 0 too)
    dp_emit<DPO_REDUCE_THREADS>(o.d, j, f, nblk, s_kmask, s_kpos, s_order, (const float4 *)nullptr);
}

// ------------------------------------------------------------------ C-ABI
struct DpoLayout {
    size_t nc, order, ext, mask, total;
    int capp, W;
};

static DpoLayout dpo_layout(int batch, const mv3d_detect_post_params *p)
{
    DpoLayout L;
    const size_t fc = (size_t)batch * (size_t)(p->num_classes - 1);
    L.capp = (p->rows_per_frame + 63) / 64 * 64;
    L.W = L.capp / 64;
    L.nc = 0;
    L.order = L.nc + mv3d_align_up(fc * sizeof(int32_t));
    L.ext = L.order + mv3d_align_up(fc * L.capp * sizeof(int32_t));
    L.mask = L.ext + mv3d_align_up(fc * L.capp * sizeof(float4));
    L.total = L.mask + mv3d_align_up(fc * L.capp * L.W * sizeof(unsigned long long));
    return L;
}

extern "C" size_t mv3d_detect_post_oriented_workspace_bytes(int batch, const mv3d_detect_post_params *p)
{
    return dp_params_ok(batch, p) ? dpo_layout(batch, p).total : 0;
}

extern "C" int mv3d_detect_post_oriented(const float *cls_prob_dev, const float *pred_bv_dev, const float *corners_dev,
                                         const float *pred_cnr_r_dev, const int32_t *num_rois_dev, int batch,
                                         const mv3d_detect_post_params *p, int footprint_source, float *det_bv_dev,
                                         float *det_cnr_dev, float *det_cnr_r_dev, int32_t *det_row_dev, int32_t *det_count_dev,
                                         int32_t *status_dev, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!dp_params_ok(batch, p) || !cls_prob_dev || !pred_bv_dev || !corners_dev || !det_bv_dev || !det_cnr_dev ||
        !det_row_dev || !det_count_dev || !status_dev || (pred_cnr_r_dev && !det_cnr_r_dev))
        return MV3D_ERR_INVALID_ARG;
    if ((footprint_source != 0 && footprint_source != 1) || (footprint_source == 1 && !pred_cnr_r_dev)) return MV3D_ERR_INVALID_ARG;
    const DpoLayout L = dpo_layout(batch, p);
    if (!workspace || workspace_bytes < L.total || ((uintptr_t)workspace & 15u)) return MV3D_ERR_INVALID_ARG;
    OrientedDev o;
    DetectPostDev &d = o.d;
    d.cls_prob = cls_prob_dev; d.pred_bv = pred_bv_dev; d.corners = corners_dev; d.pred_cnr_r = pred_cnr_r_dev;
    d.num_rois = num_rois_dev;
    d.det_bv = det_bv_dev; d.det_cnr = det_cnr_dev; d.det_cnr_r = det_cnr_r_dev;
    d.det_row = det_row_dev; d.det_count = det_count_dev; d.status = status_dev;
    d.K = p->num_classes; d.cap = p->rows_per_frame; d.max_per_image = p->max_per_image;
    d.score_thresh = p->score_thresh;
    d.tf = 0.0f;                                             // (the pixel-box rule's threshold: unused here)
    o.foot = footprint_source ? pred_cnr_r_dev : corners_dev;
    o.foot_stride = footprint_source ? 24 * d.K : 24;
    o.foot_class_stride = footprint_source ? 24 : 0;
    o.capp = L.capp; o.W = L.W;
    o.strict = p->nms_strict_gt ? 1 : 0;
    o.thresh = p->nms_thresh;
    char *ws = (char *)workspace;
    o.nc = (int32_t *)(ws + L.nc); o.order = (int32_t *)(ws + L.order);
    o.ext = (float4 *)(ws + L.ext); o.mask = (unsigned long long *)(ws + L.mask);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(detect_post_oriented_order_kernel, dim3(d.K - 1, batch), dim3(DP_THREADS), 0, st, o);
    hipLaunchKernelGGL(detect_post_oriented_mask_kernel, dim3(L.W * (L.W + 1) / 2, batch, d.K - 1), dim3(KE_OVERLAP_THREADS), 0, st, o);
    hipLaunchKernelGGL(detect_post_oriented_reduce_kernel, dim3(d.K, batch), dim3(DPO_REDUCE_THREADS), 0, st, o);
    if (d.max_per_image > 0) mv3d_launch_detect_post_cap(d, batch, st);
    return mv3d_launch_status();
}
