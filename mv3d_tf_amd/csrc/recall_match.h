// The greedy matching of lib/datasets/imdb.py:162-196 (evaluate_recall) for one (frame, limit), once, for both proposal-recall
// kernels: proposal_recall.hip (pixel-box IoU, recomputed on the fly) and proposal_recall_3d.hip (oriented BEV / 3D IoU, read from
// the workspace).  Only where an overlap value comes from and how many used-row bits are kept differ; both are parameters here.
//
// Contract per (frame f, limit l), R = the frame's rows (boxes / proposals), G = its objects; overlap(g)(i) is the overlap of row
// i with object g as the including kernel defines it (tests/recall_restatement.py and tests/recall3d_restatement.py follow this
// text line by line, each with its own overlap):
//   n        = limit <= 0 ? R : min(R, limit)                       (boxes[:limit], imdb.py:171-172)
//   R == 0   the frame is skipped (imdb.py:169-170): its G entries are -1.0, nothing is counted, no status.  (The kernels return
//            before anything here runs.)
//   rounds   j = 0 .. G-1 (imdb.py:178-194); used rows and used object columns count as -1:
//            per object, the maximum over the rows and the first index of that maximum      (overlaps.max / argmax(axis=0))
//            gt_ind = the object with the largest maximum, first index on a tie               (max_overlaps.argmax())
//            box_ind = that object's row                                                      (argmax_overlaps[gt_ind])
//            the overlap is recorded at position j of the frame's block, NOT at gt_ind (the reference's _gt_overlaps[j]; the
//            vector is only ever used sorted, but parity is on the raw vector); box_ind and gt_ind are marked used.
//   short    0 < n < G: from round n on every row is used and the reference fails assert(gt_ovr >= 0).  short_mode 0: the
//            frame's status gets MV3D_RECALL_STATUS_SHORT and rounds n .. G-1 record -1.0; short_mode 1 (this library's
//            definition, not the reference's): they record 0.0, no status.
//   finite   R > 0 and any non-finite value among ALL of the frame's R rows (whatever the limit) or its G objects: status
//            MV3D_RECALL_STATUS_NONFINITE (set by the including kernel's own code), the frame records 0.0 throughout (the
//            reference's result there hangs on C min / max of NaN and is not a target).
//   counts   counts[t] += the number of the frame's G recorded values >= thresholds[t] (skipped frames add nothing); integer
//            atomics only.
// An overlap of finite boxes is >= 0, so while an unused row is left a used row (-1) never holds a column's maximum or ties
// with it: used rows are skipped, not stored as -1 (so the 3D workspace, shared by all limits, stays read-only), and the
// first-index (value, index) reductions across lanes give exactly numpy's argmax.  After a round only the columns whose argmax
// was the consumed row are recomputed.
#pragma once
#include "common.h"

#define RM_THREADS 256        // one workgroup per matching: lane t holds column t in the round reduction (MV3D_RECALL_MAX_GT <= 256)
#define RM_WAVES 4

// The LDS state of one matching.  The first MASK_ROWS rows have a used bit; a used row beyond them is looked up in `used_row`.
template <int MASK_ROWS>
struct RmState {
    double col_max[MV3D_RECALL_MAX_GT];    // per object: the maximum over the unused rows ...
    double rec[MV3D_RECALL_MAX_GT];        // the frame's recorded overlaps, round by round
    double wkey[RM_WAVES];                 // the round reduction's per-wave (key, index)
    int col_arg[MV3D_RECALL_MAX_GT];       // ... and the first row that has it
    int col_used[MV3D_RECALL_MAX_GT];
    int used_row[MV3D_RECALL_MAX_GT];      // the rows consumed so far, in round order
    int widx[RM_WAVES];
    uint32_t mask[MASK_ROWS / 32];
};

// (largest key, first index) over the wave's 64 lanes
__device__ __forceinline__ void rm_argmax(double &key, int &idx)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double k2 = __shfl_xor(key, o);
        const int i2 = __shfl_xor(idx, o);
        if (k2 > key || (k2 == key && i2 < idx)) { key = k2; idx = i2; }
    }
}

// No column and no row is used yet.  The caller's next barrier publishes it: it must stand between this and rm_match.
template <int MASK_ROWS>
__device__ __forceinline__ void rm_clear(RmState<MASK_ROWS> &s, const int G)
{
    for (int g = threadIdx.x; g < G; g += RM_THREADS) s.col_used[g] = 0;
    for (int w = threadIdx.x; w < MASK_ROWS / 32; w += RM_THREADS) s.mask[w] = 0u;
}

// The matching of the frame's G objects against its first n >= 1 rows, by all RM_THREADS lanes: the rounds, the short-frame
// tail (status bit into *status), the G recorded values into out[0 .. G-1] and the threshold counts into counts[0 .. T-1].
// overlap(g) -> a callable i -> the overlap of row i with object g (whatever belongs to the object alone is loaded once per
// column that way).  nonfinite (workgroup-uniform): the frame records 0.0 and no overlap is evaluated.
template <int MASK_ROWS, typename Overlap>
__device__ __forceinline__ void rm_match(RmState<MASK_ROWS> &s, const int G, const int n, const bool nonfinite, const int short_mode,
                                         Overlap overlap, double *__restrict__ out, const double *__restrict__ thresholds, const int T,
                                         int32_t *__restrict__ counts, int32_t *status)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rounds = G < n ? G : n;
    if (nonfinite) {
        for (int g = tid; g < G; g += RM_THREADS) s.rec[g] = 0.0;
    } else {
        // the maximum of column g over the unused rows (`nused` of them consumed so far) and its first index
        auto column = [&](int g, int nused) {
            const auto ov = overlap(g);
            double best = -1.0;
            int bi = INT32_MAX;
            for (int i = lane; i < n; i += 64) {
                bool used = false;
                if (nused > 0) {
                    if (i < MASK_ROWS) used = (s.mask[i >> 5] >> (i & 31)) & 1u;
                    else
                        for (int k = 0; k < nused; ++k) used = used || s.used_row[k] == i;
                }
                if (used) continue;
                const double o = ov(i);
                if (o > best) { best = o; bi = i; }
            }
            rm_argmax(best, bi);
            if (lane == 0) { s.col_max[g] = best; s.col_arg[g] = bi; }
        };
        for (int g = wave; g < G; g += RM_WAVES) column(g, 0);
        __syncthreads();
        for (int j = 0; j < rounds; ++j) {
            // max_overlaps.argmax() over the unused columns: lane t holds column t
            double key = -INFINITY;
            int idx = INT32_MAX;
            if (tid < G && !s.col_used[tid]) { key = s.col_max[tid]; idx = tid; }
            rm_argmax(key, idx);
            if (lane == 0) { s.wkey[wave] = key; s.widx[wave] = idx; }
            __syncthreads();
            key = s.wkey[0]; idx = s.widx[0];
#pragma unroll
            for (int w = 1; w < RM_WAVES; ++w) {
                const double k2 = s.wkey[w];
                const int i2 = s.widx[w];
                if (k2 > key || (k2 == key && i2 < idx)) { key = k2; idx = i2; }
            }
            const int row = s.col_arg[idx];
            if (tid == 0) {                             // (nothing a lane still reads in this phase)
                s.rec[j] = key;
                s.col_used[idx] = 1;
                s.used_row[j] = row;
                if (row < MASK_ROWS) s.mask[row >> 5] |= 1u << (row & 31);
            }
            __syncthreads();
            if (j + 1 < rounds)
                for (int g = wave; g < G; g += RM_WAVES)
                    if (!s.col_used[g] && s.col_arg[g] == row) column(g, j + 1);
            __syncthreads();
        }
        if (rounds < G) {                               // short frame: no unused row is left
            for (int j = rounds + tid; j < G; j += RM_THREADS) s.rec[j] = short_mode == MV3D_RECALL_SHORT_ZERO ? 0.0 : -1.0;
            if (tid == 0 && short_mode != MV3D_RECALL_SHORT_ZERO) atomicOr(status, MV3D_RECALL_STATUS_SHORT);
        }
    }
    __syncthreads();
    for (int g = tid; g < G; g += RM_THREADS) out[g] = s.rec[g];
    for (int t = wave; t < T; t += RM_WAVES) {
        const double thr = thresholds[t];
        int c = 0;
        for (int g = lane; g < MV3D_RECALL_MAX_GT; g += 64) c += __popcll(__ballot(g < G && s.rec[g] >= thr));
        if (lane == 0 && c) atomicAdd(counts + t, c);
    }
}

// ------------------------------------------------------------------ host
// What mv3d_recall_split and mv3d_recall3d_split have in common, checked on the host before any device call: the counts, the
// limits range, the short mode, box_off / gt_off from 0 to the totals, R >= 0 and 0 <= G <= MV3D_RECALL_MAX_GT per frame.
template <typename Split>
static int rm_validate_split(const Split *s)
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
    if (F > 0 && (!s->box_off_dev || !s->gt_off_dev)) return MV3D_ERR_INVALID_ARG;
    if (s->num_boxes > 0 && !s->boxes_dev) return MV3D_ERR_INVALID_ARG;
    if (s->num_thresholds > 0 && !s->thresholds_dev) return MV3D_ERR_INVALID_ARG;
    return MV3D_OK;
}
