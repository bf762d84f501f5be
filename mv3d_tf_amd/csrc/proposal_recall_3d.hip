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
//   matching, per (frame f, limit l, metric m in {bev, 3d}), DESIGN.md §3.14 with the overlap above:
//     n        = limit <= 0 ? R : min(R, limit)
//     R == 0   the frame is skipped: its G entries are -1.0, nothing is counted, no status.
//     rounds   j = 0 .. G-1; used rows and used columns count as -1: per object the maximum over the rows and the first index of
//              that maximum; gt_ind = the object with the largest maximum, first index on a tie; box_ind = that object's row; the
//              overlap is recorded at position j of the frame's block, NOT at gt_ind; box_ind and gt_ind are marked used.
//     short    0 < n < G: short_mode 0 sets MV3D_RECALL_STATUS_SHORT and rounds n .. G-1 record -1.0; short_mode 1 records 0.0
//              for them and sets nothing.
//     finite   R > 0 and any non-finite value among ALL of the frame's R proposal rows (whatever the limit, every one of the 6 /
//              24 values) or its G objects: status MV3D_RECALL_STATUS_NONFINITE, the frame records 0.0 throughout.
//     counts   counts[m][l][t] += the number of the frame's G recorded values >= thresholds[t]; integer atomics only.
// An overlap of finite boxes is >= 0, so while an unused row is left a used row (-1) never holds a column's maximum: the match
// kernel skips used rows instead of storing -1 (the workspace is shared by all limits and stays read-only), and the first-index
// (value, index) reductions across lanes give exactly numpy's argmax.  After a round only the columns whose argmax was the
// consumed row are recomputed.
//
// The extents of step 1 are kept as f32: the minimum of f32 values converted to f64 is the converted f32 minimum, so the f64
// comparisons of step 2 see the same numbers.  Pairs that pass step 2 are few (a few percent) and scattered over the lanes; the
// overlap kernel therefore queues their indices in LDS (ballot + prefix count) and runs the clip on full waves of queued pairs.
// The stored values do not depend on that order.  -DMV3D_RECALL3D_NO_COMPACT (an experiment build) clips in place instead.
// No workgroup waits on another; every loop bound is a count validated on the host.
#include "box_iou.h"

#define R3_ROWS 128           // proposal rows of one overlap workgroup
#define R3_QUEUE 128          // queued pair indices: drained whenever 64 are waiting, so never more than 127
#define R3_THREADS 256        // match kernel
#define R3_WAVES 4
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

// (largest key, first index) over the wave's 64 lanes
__device__ __forceinline__ void r3_argmax(double &key, int &idx)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double k2 = __shfl_xor(key, o);
        const int i2 = __shfl_xor(idx, o);
        if (k2 > key || (k2 == key && i2 < idx)) { key = k2; idx = i2; }
    }
}

__global__ __launch_bounds__(R3_THREADS) void recall3d_match_kernel(
    const int32_t *__restrict__ box_off, const int32_t *__restrict__ gt_off, const int32_t *__restrict__ pair_off,
    const double *__restrict__ iou, long long P, const int32_t *__restrict__ limits, const double *__restrict__ thresholds, int T,
    int short_mode, long long Gtot, double *__restrict__ gt_overlaps, int32_t *__restrict__ counts, int32_t *status)
{
    __shared__ double s_max[MV3D_RECALL_MAX_GT];      // per object: the maximum over the unused rows ...
    __shared__ int s_arg[MV3D_RECALL_MAX_GT];         // ... and the first row that has it
    __shared__ int s_col_used[MV3D_RECALL_MAX_GT];
    __shared__ double s_rec[MV3D_RECALL_MAX_GT];      // the frame's recorded overlaps, round by round
    __shared__ int s_used_row[MV3D_RECALL_MAX_GT];    // the rows consumed so far, in round order
    __shared__ uint32_t s_mask[R3_MASK_ROWS / 32];
    __shared__ double s_wkey[R3_WAVES];
    __shared__ int s_widx[R3_WAVES];

    const int f = blockIdx.x, l = blockIdx.y, metric = blockIdx.z, L = gridDim.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = box_off[f + 1] - box_off[f], g0 = gt_off[f], G = gt_off[f + 1] - g0;
    const int limit = limits[l];
    const int n = (limit <= 0 || limit > R) ? R : limit;
    double *out = gt_overlaps + ((long long)metric * L + l) * Gtot + g0;
    if (R == 0) {                                      // skipped frame
        for (int g = tid; g < G; g += R3_THREADS) out[g] = -1.0;
        return;
    }
    const double *blk = iou + (long long)metric * P + pair_off[f];
    // the overlap launch, complete before this one starts, has set the bit; match workgroups only ever add the other bit
    const bool nonfinite = (__hip_atomic_load(status + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & MV3D_RECALL_STATUS_NONFINITE) != 0;
    for (int g = tid; g < G; g += R3_THREADS) s_col_used[g] = 0;
    for (int w = tid; w < R3_MASK_ROWS / 32; w += R3_THREADS) s_mask[w] = 0u;
    __syncthreads();

    const int rounds = G < n ? G : n;
    if (nonfinite) {
        for (int g = tid; g < G; g += R3_THREADS) s_rec[g] = 0.0;
    } else {
        // the maximum of column g over the unused rows (`nused` of them consumed so far) and its first index
        auto column = [&](int g, int nused) {
            double best = -1.0;
            int bi = INT32_MAX;
            for (int i = lane; i < n; i += 64) {
                bool used = false;
                if (nused > 0) {
                    if (i < R3_MASK_ROWS) used = (s_mask[i >> 5] >> (i & 31)) & 1u;
                    else
                        for (int k = 0; k < nused; ++k) used = used || s_used_row[k] == i;
                }
                if (used) continue;
                const double o = blk[(long long)i * G + g];
                if (o > best) { best = o; bi = i; }
            }
            r3_argmax(best, bi);
            if (lane == 0) { s_max[g] = best; s_arg[g] = bi; }
        };
        for (int g = wave; g < G; g += R3_WAVES) column(g, 0);
        __syncthreads();
        for (int j = 0; j < rounds; ++j) {
            // max_overlaps.argmax() over the unused columns: lane t holds column t
            double key = -INFINITY;
            int idx = INT32_MAX;
            if (tid < G && !s_col_used[tid]) { key = s_max[tid]; idx = tid; }
            r3_argmax(key, idx);
            if (lane == 0) { s_wkey[wave] = key; s_widx[wave] = idx; }
            __syncthreads();
            key = s_wkey[0]; idx = s_widx[0];
#pragma unroll
            for (int w = 1; w < R3_WAVES; ++w) {
                const double k2 = s_wkey[w];
                const int i2 = s_widx[w];
                if (k2 > key || (k2 == key && i2 < idx)) { key = k2; idx = i2; }
            }
            const int row = s_arg[idx];
            if (tid == 0) {                             // (nothing a lane still reads in this phase)
                s_rec[j] = key;
                s_col_used[idx] = 1;
                s_used_row[j] = row;
                if (row < R3_MASK_ROWS) s_mask[row >> 5] |= 1u << (row & 31);
            }
            __syncthreads();
            if (j + 1 < rounds)
                for (int g = wave; g < G; g += R3_WAVES)
                    if (!s_col_used[g] && s_arg[g] == row) column(g, j + 1);
            __syncthreads();
        }
        if (rounds < G) {                               // short frame: no unused row is left
            for (int j = rounds + tid; j < G; j += R3_THREADS) s_rec[j] = short_mode == MV3D_RECALL_SHORT_ZERO ? 0.0 : -1.0;
            if (tid == 0 && short_mode != MV3D_RECALL_SHORT_ZERO) atomicOr(status + f, MV3D_RECALL_STATUS_SHORT);
        }
    }
    __syncthreads();
    for (int g = tid; g < G; g += R3_THREADS) out[g] = s_rec[g];
    for (int t = wave; t < T; t += R3_WAVES) {
        const double thr = thresholds[t];
        int c = 0;
        for (int g = lane; g < MV3D_RECALL_MAX_GT; g += 64) c += __popcll(__ballot(g < G && s_rec[g] >= thr));
        if (lane == 0 && c) atomicAdd(counts + ((long long)metric * L + l) * T + t, c);
    }
}

// ------------------------------------------------------------------ C-ABI
extern "C" size_t mv3d_proposal_recall_3d_workspace_bytes(long long num_pairs)
{
    return num_pairs > 0 ? 16 * (size_t)num_pairs : 0;
}

// everything the host can check; -> MV3D_OK and the number of row chunks of the overlap grid
static int r3_validate(const mv3d_recall3d_split *s, long long *chunks)
{
    if (!s || s->num_frames < 0 || s->num_gts < 0 || s->num_boxes < 0 || s->num_boxes > INT32_MAX || s->num_pairs < 0 ||
        s->num_pairs > INT32_MAX || s->num_limits < 1 || s->num_limits > 65535 || s->num_thresholds < 0 || !s->box_off || !s->gt_off ||
        !s->pair_off || !s->limits_dev)
        return MV3D_ERR_INVALID_ARG;
    if (s->short_mode != MV3D_RECALL_SHORT_ASSERT && s->short_mode != MV3D_RECALL_SHORT_ZERO) return MV3D_ERR_INVALID_ARG;
    if (s->box_format != MV3D_RECALL3D_BOX6 && s->box_format != MV3D_RECALL3D_CNR24) return MV3D_ERR_INVALID_ARG;
    const int F = s->num_frames;
    if (s->box_off[0] != 0 || s->gt_off[0] != 0 || s->pair_off[0] != 0 || s->box_off[F] != s->num_boxes || s->gt_off[F] != s->num_gts ||
        s->pair_off[F] != s->num_pairs)
        return MV3D_ERR_INVALID_ARG;
    long long max_rows = 0;
    for (int f = 0; f < F; ++f) {
        const long long R = (long long)s->box_off[f + 1] - s->box_off[f], G = (long long)s->gt_off[f + 1] - s->gt_off[f];
        if (R < 0 || G < 0 || G > MV3D_RECALL_MAX_GT) return MV3D_ERR_INVALID_ARG;
        if ((long long)s->pair_off[f + 1] - s->pair_off[f] != R * G) return MV3D_ERR_INVALID_ARG;    // (R * G <= 2^31 * 256)
        max_rows = R > max_rows ? R : max_rows;
    }
    *chunks = (max_rows + R3_ROWS - 1) / R3_ROWS;
    if (*chunks > 65535) return MV3D_ERR_INVALID_ARG;
    if (F > 0 && (!s->box_off_dev || !s->gt_off_dev || !s->pair_off_dev)) return MV3D_ERR_INVALID_ARG;
    if (s->num_boxes > 0 && !s->boxes_dev) return MV3D_ERR_INVALID_ARG;
    if (s->num_gts > 0 && !s->gt_cnr_dev) return MV3D_ERR_INVALID_ARG;
    if (s->num_thresholds > 0 && !s->thresholds_dev) return MV3D_ERR_INVALID_ARG;
    return MV3D_OK;
}

extern "C" int mv3d_proposal_recall_3d_overlaps(const mv3d_recall3d_split *s, double *iou_ws_dev, int32_t *status_dev, void *stream)
{
    long long chunks = 0;
    if (r3_validate(s, &chunks) != MV3D_OK) return MV3D_ERR_INVALID_ARG;
    if ((s->num_frames > 0 && !status_dev) || (s->num_pairs > 0 && !iou_ws_dev)) return MV3D_ERR_INVALID_ARG;
    if (s->num_frames == 0) return MV3D_OK;
    MV3D_HIP_TRY(hipMemsetAsync(status_dev, 0, sizeof(int32_t) * (size_t)s->num_frames, (hipStream_t)stream));
    if (chunks == 0) return MV3D_OK;
    hipLaunchKernelGGL(recall3d_overlap_kernel, dim3(s->num_frames, (unsigned)chunks), dim3(KE_OVERLAP_THREADS), 0, (hipStream_t)stream,
                       s->box_off_dev, s->gt_off_dev, s->pair_off_dev, s->boxes_dev, s->box_format, s->gt_cnr_dev, iou_ws_dev, s->num_pairs,
                       status_dev);
    return mv3d_launch_status();
}

extern "C" int mv3d_proposal_recall_3d_match(const mv3d_recall3d_split *s, const double *iou_ws_dev, double *gt_overlaps_dev,
                                             int32_t *counts_dev, int32_t *status_dev, void *stream)
{
    long long chunks = 0;
    if (r3_validate(s, &chunks) != MV3D_OK) return MV3D_ERR_INVALID_ARG;
    if ((s->num_frames > 0 && !status_dev) || (s->num_pairs > 0 && !iou_ws_dev) || (s->num_gts > 0 && !gt_overlaps_dev) ||
        (s->num_thresholds > 0 && !counts_dev))
        return MV3D_ERR_INVALID_ARG;
    if (s->num_thresholds > 0)
        MV3D_HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(int32_t) * 2 * (size_t)s->num_limits * (size_t)s->num_thresholds, (hipStream_t)stream));
    if (s->num_frames == 0) return MV3D_OK;
    hipLaunchKernelGGL(recall3d_match_kernel, dim3(s->num_frames, s->num_limits, 2), dim3(R3_THREADS), 0, (hipStream_t)stream, s->box_off_dev,
                       s->gt_off_dev, s->pair_off_dev, iou_ws_dev, s->num_pairs, s->limits_dev, s->thresholds_dev, s->num_thresholds,
                       s->short_mode, (long long)s->num_gts, gt_overlaps_dev, counts_dev, status_dev);
    return mv3d_launch_status();
}

extern "C" int mv3d_proposal_recall_3d(const mv3d_recall3d_split *s, double *iou_ws_dev, double *gt_overlaps_dev, int32_t *counts_dev,
                                       int32_t *status_dev, void *stream)
{
    long long chunks = 0;
    if (r3_validate(s, &chunks) != MV3D_OK) return MV3D_ERR_INVALID_ARG;
    if ((s->num_frames > 0 && !status_dev) || (s->num_pairs > 0 && !iou_ws_dev) || (s->num_gts > 0 && !gt_overlaps_dev) ||
        (s->num_thresholds > 0 && !counts_dev))
        return MV3D_ERR_INVALID_ARG;
    const int rc = mv3d_proposal_recall_3d_overlaps(s, iou_ws_dev, status_dev, stream);
    if (rc != MV3D_OK) return rc;
    return mv3d_proposal_recall_3d_match(s, iou_ws_dev, gt_overlaps_dev, counts_dev, status_dev, stream);
}
