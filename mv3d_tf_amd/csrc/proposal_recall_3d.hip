// Proposal recall by oriented BEV / 3D IoU against the objects' LIDAR corners: the greedy matching of
// lib/datasets/imdb.py:162-196 with the evaluator's polygon clip (box_iou.h) in the place of bbox_overlaps, for every frame of a
// split, every proposal limit and both metrics.  Two launches:
//
//   recall3d_overlap_kernel   grid (frame, chunk of R3_ROWS proposal rows), one wave per workgroup: iou_bev / iou_3d of every
//                             (proposal, object) pair of the chunk into the frame's R x G row-major block of the workspace at
//                             pair_off[f] (two planes: bev | 3d), ONCE per frame: every limit is a row prefix of the same block.
//                             Also the frame's finiteness (status bit), since it reads every row anyway.
//   recall3d_match_kernel     grid (frame, limit, metric), 256 lanes: the rounds of the matching over the first n rows of the
//                             block, which it only reads.
//
// Frames are CSR ranges: frame f owns proposals box_off[f] .. box_off[f+1]-1 (R of them), objects gt_off[f] .. gt_off[f+1]-1 (G),
// and the workspace block pair_off[f] .. pair_off[f+1]-1, pair_off[0] = 0, pair_off[f+1] = pair_off[f] + R * G.
//
// Contract (tests/recall3d_restatement.py follows it line by line):
//   proposals  MV3D_RECALL3D_BOX6: (N, 6) f32 x, y, z, l, w, h; corner k = box_corner(P, k) of geometry.h in f32, the reference's
//              lidar_3d_to_corners: halves by / 2.0f, signs x [+,+,-,-,...], y [+,-,-,+,...], z [- x 4, + x 4], the centre added
//              to the signed half.  MV3D_RECALL3D_CNR24: (N, 24) f32 x0..7, y0..7, z0..7 as they are.
//   objects    (G_total, 24) f32 LIDAR corners, at most MV3D_RECALL_MAX_GT per frame.
//   overlap of (proposal a, object b), both planes at once:
//     1. in f64, min / max of x and of y over each box's footprint vertices k = 0..3: start from k = 0, then k = 1..3 with
//        strict < / >.
//     2. a.maxx < b.minx || b.maxx < a.minx || a.maxy < b.miny || b.maxy < a.miny: iou_bev = iou_3d = 0.0, nothing else runs.
//     3. otherwise ke_load(a), ke_load(b), and if both are finite ke_iou(a, b) exactly as the evaluator runs it (the polygon is
//        a's footprint, the clipper b's edges); a non-finite box gives 0.0 / 0.0 as there.
//   matching, per (frame f, limit l, metric m in {bev, 3d}): n, R == 0, rounds, short, finite and counts as the header comment of
//     recall_match.h states them, with the overlap above; finite is over every one of the 6 / 24 values of ALL of the frame's R
//     proposal rows and over its G objects, the overlap kernel sets the bit, and the counts are counts[m][l][t].  The match
//     kernel only reads the workspace, which all limits share.
//
// The extents of step 1 are kept as f32: the minimum of f32 values converted to f64 is the converted f32 minimum, so the f64
// comparisons of step 2 see the same numbers.  Pairs that pass step 2 are few (a few percent) and scattered over the lanes; the
// overlap kernel therefore queues their indices in LDS (ballot + prefix count) and runs the clip on full waves of queued pairs.
// The stored values do not depend on that order.  -DMV3D_RECALL3D_NO_COMPACT (an experiment build) clips in place instead.
// No workgroup waits on another; every loop bound is a count validated on the host.
#include "box_iou.h"
#include "recall_match.h"

#define R3_ROWS 128           // proposal rows of one overlap workgroup
#define R3_QUEUE 128          // queued pair indices: drained whenever 64 are waiting, so never more than 127
#define R3_MASK_ROWS 4096     // used-row bits kept in LDS (512 B); a used row beyond them is looked up in the list of used rows

// the 24 corner values of proposal row `r` (absolute row index)
__device__ __forceinline__ void r3_corners(const float *__restrict__ boxes, int fmt, long long r, float c[24])
{
    if (fmt == MV3D_RECALL3D_BOX6) {
        float P[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) P[k] = boxes[6 * r + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) box_corner(P, k, c[k], c[8 + k], c[16 + k]);
    } else {
#pragma unroll
        for (int k = 0; k < 24; ++k) c[k] = boxes[24 * r + k];
    }
}

// step 1: (minx, maxx, miny, maxy) over the footprint vertices
__device__ __forceinline__ float4 r3_extent(const float c[24])
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

__global__ __launch_bounds__(KE_OVERLAP_THREADS) void recall3d_overlap_kernel(
    const int32_t *__restrict__ box_off, const int32_t *__restrict__ gt_off, const int32_t *__restrict__ pair_off,
    const float *__restrict__ boxes, int fmt, const float *__restrict__ gt_cnr, double *__restrict__ iou, long long P,
    int32_t *__restrict__ status)
{
    __shared__ double poly[2 * KE_MAXV * 2 * KE_OVERLAP_THREADS];
    __shared__ float4 s_gt[MV3D_RECALL_MAX_GT];
    __shared__ float4 s_row[R3_ROWS];
    __shared__ int s_queue[R3_QUEUE];

    const int f = blockIdx.x, lane = threadIdx.x;
    const int b0 = box_off[f], R = box_off[f + 1] - b0, g0 = gt_off[f], G = gt_off[f + 1] - g0;
    const int r0 = blockIdx.y * R3_ROWS;
    if (r0 >= R) return;                                   // (uniform; a frame without proposals launches nothing)
    const int rows = R - r0 < R3_ROWS ? R - r0 : R3_ROWS;
    bool bad = false;
    for (int i = lane; i < rows; i += KE_OVERLAP_THREADS) {
        const long long r = (long long)b0 + r0 + i;
        const int nv = fmt == MV3D_RECALL3D_BOX6 ? 6 : 24;
        for (int k = 0; k < nv; ++k) bad = bad || !isfinite(boxes[nv * r + k]);
        float c[24];
        r3_corners(boxes, fmt, r, c);
        s_row[i] = r3_extent(c);
    }
    for (int g = lane; g < G; g += KE_OVERLAP_THREADS) {
        const float *q = gt_cnr + 24 * (long long)(g0 + g);
        float c[24];
#pragma unroll
        for (int k = 0; k < 24; ++k) { c[k] = q[k]; bad = bad || !isfinite(c[k]); }
        s_gt[g] = r3_extent(c);
    }
    if (__syncthreads_or(bad ? 1 : 0) && lane == 0) atomicOr(status + f, MV3D_RECALL_STATUS_NONFINITE);
    if (G == 0) return;

    double *out = iou + (long long)pair_off[f] + (long long)r0 * G;      // the chunk's pairs, row-major
    const int np = rows * G;
    auto clip = [&](int p) {
        const int i = p / G, g = p - i * G;
        float ca[24], cb[24];
        r3_corners(boxes, fmt, (long long)b0 + r0 + i, ca);
        const float *q = gt_cnr + 24 * (long long)(g0 + g);
#pragma unroll
        for (int k = 0; k < 24; ++k) cb[k] = q[k];
        KeBox a, b;
        const bool fa = ke_load(ca, a);
        const bool fb = ke_load(cb, b);
        double ib = 0.0, i3 = 0.0;
        if (fa && fb) ke_iou(a, b, poly, lane, ib, i3);
        out[p] = ib;
        out[P + p] = i3;
    };
    int queued = 0;                                        // (uniform)
    for (int base = 0; base < np; base += KE_OVERLAP_THREADS) {
        const int p = base + lane;
        bool pass = false;
        if (p < np) {
            const int i = p / G, g = p - i * G;
            const float4 a = s_row[i], b = s_gt[g];        // x = minx, y = maxx, z = miny, w = maxy
            pass = !((double)a.y < (double)b.x || (double)b.y < (double)a.x || (double)a.w < (double)b.z || (double)b.w < (double)a.z);
            if (!pass) { out[p] = 0.0; out[P + p] = 0.0; }
        }
#ifdef MV3D_RECALL3D_NO_COMPACT
        if (pass) clip(p);
#else
        const unsigned long long m = __ballot(pass);
        if (pass) s_queue[queued + __popcll(m & ((1ull << lane) - 1ull))] = p;
        queued += __popcll(m);
        __syncthreads();
        if (queued >= KE_OVERLAP_THREADS) {                // a full wave of pairs is waiting
            clip(s_queue[lane]);
            const int rest = queued - KE_OVERLAP_THREADS;
            const int moved = lane < rest ? s_queue[KE_OVERLAP_THREADS + lane] : 0;
            __syncthreads();
            if (lane < rest) s_queue[lane] = moved;
            queued = rest;
            __syncthreads();
        }
#endif
    }
#ifndef MV3D_RECALL3D_NO_COMPACT
    if (lane < queued) clip(s_queue[lane]);
#endif
}

__global__ __launch_bounds__(RM_THREADS) void recall3d_match_kernel(
    const int32_t *__restrict__ box_off, const int32_t *__restrict__ gt_off, const int32_t *__restrict__ pair_off,
    const double *__restrict__ iou, long long P, const int32_t *__restrict__ limits, const double *__restrict__ thresholds, int T,
    int short_mode, long long Gtot, double *__restrict__ gt_overlaps, int32_t *__restrict__ counts, int32_t *status)
{
    __shared__ RmState<R3_MASK_ROWS> s_match;

    const int f = blockIdx.x, l = blockIdx.y, metric = blockIdx.z, L = gridDim.y;
    const int tid = threadIdx.x;
    const int R = box_off[f + 1] - box_off[f], g0 = gt_off[f], G = gt_off[f + 1] - g0;
    const int limit = limits[l];
    const int n = (limit <= 0 || limit > R) ? R : limit;
    double *out = gt_overlaps + ((long long)metric * L + l) * Gtot + g0;
    if (R == 0) {                                      // skipped frame
        for (int g = tid; g < G; g += RM_THREADS) out[g] = -1.0;
        return;
    }
    const double *blk = iou + (long long)metric * P + pair_off[f];
    // the overlap launch, complete before this one starts, has set the bit; match workgroups only ever add the other bit
    const bool nonfinite = (__hip_atomic_load(status + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & MV3D_RECALL_STATUS_NONFINITE) != 0;
    rm_clear(s_match, G);
    __syncthreads();
    auto overlap = [&](int g) {
        const double *col = blk + g;
        return [=](int i) { return col[(long long)i * G]; };
    };
    rm_match(s_match, G, n, nonfinite, short_mode, overlap, out, thresholds, T, counts + ((long long)metric * L + l) * T, status + f);
}

// ------------------------------------------------------------------ C-ABI
extern "C" size_t mv3d_proposal_recall_3d_workspace_bytes(long long num_pairs)
{
    return num_pairs > 0 ? 16 * (size_t)num_pairs : 0;
}

// everything the host can check; -> MV3D_OK and the number of row chunks of the overlap grid
static int r3_validate(const mv3d_recall3d_split *s, long long *chunks)
{
    if (rm_validate_split(s) != MV3D_OK || s->num_pairs < 0 || s->num_pairs > INT32_MAX || !s->pair_off) return MV3D_ERR_INVALID_ARG;
    if (s->box_format != MV3D_RECALL3D_BOX6 && s->box_format != MV3D_RECALL3D_CNR24) return MV3D_ERR_INVALID_ARG;
    const int F = s->num_frames;
    if (s->pair_off[0] != 0 || s->pair_off[F] != s->num_pairs) return MV3D_ERR_INVALID_ARG;
    long long max_rows = 0;
    for (int f = 0; f < F; ++f) {
        const long long R = (long long)s->box_off[f + 1] - s->box_off[f], G = (long long)s->gt_off[f + 1] - s->gt_off[f];
        if ((long long)s->pair_off[f + 1] - s->pair_off[f] != R * G) return MV3D_ERR_INVALID_ARG;    // (R * G <= 2^31 * 256)
        max_rows = R > max_rows ? R : max_rows;
    }
    *chunks = (max_rows + R3_ROWS - 1) / R3_ROWS;
    if (*chunks > 65535) return MV3D_ERR_INVALID_ARG;
    if (F > 0 && !s->pair_off_dev) return MV3D_ERR_INVALID_ARG;
    if (s->num_gts > 0 && !s->gt_cnr_dev) return MV3D_ERR_INVALID_ARG;
    return MV3D_OK;
}

// the two launches of a validated split
static int r3_queue_overlaps(const mv3d_recall3d_split *s, long long chunks, double *iou_ws_dev, int32_t *status_dev, void *stream)
{
    if (s->num_frames == 0) return MV3D_OK;
    MV3D_HIP_TRY(hipMemsetAsync(status_dev, 0, sizeof(int32_t) * (size_t)s->num_frames, (hipStream_t)stream));
    if (chunks == 0) return MV3D_OK;
    hipLaunchKernelGGL(recall3d_overlap_kernel, dim3(s->num_frames, (unsigned)chunks), dim3(KE_OVERLAP_THREADS), 0, (hipStream_t)stream,
                       s->box_off_dev, s->gt_off_dev, s->pair_off_dev, s->boxes_dev, s->box_format, s->gt_cnr_dev, iou_ws_dev, s->num_pairs,
                       status_dev);
    return mv3d_launch_status();
}

static int r3_queue_match(const mv3d_recall3d_split *s, const double *iou_ws_dev, double *gt_overlaps_dev, int32_t *counts_dev,
                          int32_t *status_dev, void *stream)
{
    if (s->num_thresholds > 0)
        MV3D_HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(int32_t) * 2 * (size_t)s->num_limits * (size_t)s->num_thresholds, (hipStream_t)stream));
    if (s->num_frames == 0) return MV3D_OK;
    hipLaunchKernelGGL(recall3d_match_kernel, dim3(s->num_frames, s->num_limits, 2), dim3(RM_THREADS), 0, (hipStream_t)stream, s->box_off_dev,
                       s->gt_off_dev, s->pair_off_dev, iou_ws_dev, s->num_pairs, s->limits_dev, s->thresholds_dev, s->num_thresholds,
                       s->short_mode, (long long)s->num_gts, gt_overlaps_dev, counts_dev, status_dev);
    return mv3d_launch_status();
}

static bool r3_match_outputs(const mv3d_recall3d_split *s, const double *iou_ws_dev, const double *gt_overlaps_dev, const int32_t *counts_dev,
                             const int32_t *status_dev)
{
    return !((s->num_frames > 0 && !status_dev) || (s->num_pairs > 0 && !iou_ws_dev) || (s->num_gts > 0 && !gt_overlaps_dev) ||
             (s->num_thresholds > 0 && !counts_dev));
}

extern "C" int mv3d_proposal_recall_3d_overlaps(const mv3d_recall3d_split *s, double *iou_ws_dev, int32_t *status_dev, void *stream)
{
    long long chunks = 0;
    if (r3_validate(s, &chunks) != MV3D_OK) return MV3D_ERR_INVALID_ARG;
    if ((s->num_frames > 0 && !status_dev) || (s->num_pairs > 0 && !iou_ws_dev)) return MV3D_ERR_INVALID_ARG;
    return r3_queue_overlaps(s, chunks, iou_ws_dev, status_dev, stream);
}

extern "C" int mv3d_proposal_recall_3d_match(const mv3d_recall3d_split *s, const double *iou_ws_dev, double *gt_overlaps_dev,
                                             int32_t *counts_dev, int32_t *status_dev, void *stream)
{
    long long chunks = 0;
    if (r3_validate(s, &chunks) != MV3D_OK || !r3_match_outputs(s, iou_ws_dev, gt_overlaps_dev, counts_dev, status_dev)) return MV3D_ERR_INVALID_ARG;
    return r3_queue_match(s, iou_ws_dev, gt_overlaps_dev, counts_dev, status_dev, stream);
}

extern "C" int mv3d_proposal_recall_3d(const mv3d_recall3d_split *s, double *iou_ws_dev, double *gt_overlaps_dev, int32_t *counts_dev,
                                       int32_t *status_dev, void *stream)
{
    long long chunks = 0;
    if (r3_validate(s, &chunks) != MV3D_OK || !r3_match_outputs(s, iou_ws_dev, gt_overlaps_dev, counts_dev, status_dev)) return MV3D_ERR_INVALID_ARG;
    const int rc = r3_queue_overlaps(s, chunks, iou_ws_dev, status_dev, stream);
    if (rc != MV3D_OK) return rc;
    return r3_queue_match(s, iou_ws_dev, gt_overlaps_dev, counts_dev, status_dev, stream);
}
