// What the two test-time tails share (detect_post.hip: NMS of the axis-aligned pixel boxes; detect_post_oriented.hip: NMS of the
// oriented BEV footprints): the argument block, the candidate order (steps 1-2 of the header comment of detect_post.hip), the
// output step (5) and the launcher of the cap kernel.
#pragma once
#include "kernels.h"

#define DP_MAX_ROWS 2048
#define DP_MAX_CLASSES 8
#define DP_THREADS 1024
#define DP_WAVES (DP_THREADS / 64)

struct DetectPostDev {
    const float *cls_prob, *pred_bv, *corners, *pred_cnr_r;
    const int32_t *num_rois;
    float *det_bv, *det_cnr, *det_cnr_r;
    int32_t *det_row, *det_count, *status;
    int K, cap, max_per_image;
    float score_thresh, tf;
};

static inline bool dp_params_ok(int batch, const mv3d_detect_post_params *p)
{
    return p && batch > 0 && batch <= 65535 && p->num_classes >= 2 && p->num_classes <= DP_MAX_CLASSES &&
           p->rows_per_frame >= 1 && p->rows_per_frame <= DP_MAX_ROWS;
}

// the cap over all classes (detect_post_cap_kernel, detect_post.hip), grid (batch); only for max_per_image > 0
void mv3d_launch_detect_post_cap(const DetectPostDev &d, int batch, hipStream_t stream);

// Steps 1-2 for class j of frame f, by a workgroup of DP_THREADS threads: s_sort[0 .. nc) = the candidates' keys
// (mv3d_score_key(score) << 32 | row), descending; returns nc.  Ends behind a barrier.
__device__ __forceinline__ int dp_sort_candidates(const DetectPostDev &d, const int j, const int f, unsigned long long *s_sort, int *s_nc)
{
    const int t = threadIdx.x, K = d.K, cap = d.cap;
    int n = cap;
    if (d.num_rois) { const int v = d.num_rois[f]; n = v < n ? v : n; }
    if (n < 0) n = 0;
    int ns = 64;                                             // sort size: a power of two >= n
    while (ns < n) ns <<= 1;
    const long long row0 = (long long)f * cap;

    // 1. keys
    if (t == 0) *s_nc = 0;
    for (int p = t; p < ns; p += DP_THREADS) {
        unsigned long long c = 0ull;
        if (p < n) {
            const float s = d.cls_prob[(row0 + p) * K + j];
            if (s > d.score_thresh) c = ((unsigned long long)mv3d_score_key(s) << 32) | (unsigned)p;
        }
        s_sort[p] = c;
    }
    __syncthreads();

    // 2. bitonic sort, descending
    for (int k = 2; k <= ns; k <<= 1) {
        for (int h = k >> 1; h > 0; h >>= 1) {
            for (int q = t; q < (ns >> 1); q += DP_THREADS) {
                const int i = ((q & ~(h - 1)) << 1) | (q & (h - 1)), l = i | h;
                const unsigned long long a = s_sort[i], b = s_sort[l];
                const bool desc = (i & k) == 0;
                if (desc ? (a < b) : (a > b)) { s_sort[i] = b; s_sort[l] = a; }
            }
            __syncthreads();
        }
    }
    for (int p = t; p < ns; p += DP_THREADS)
        if (s_sort[p] != 0ull && (p + 1 == ns || s_sort[p + 1] == 0ull)) *s_nc = p + 1;
    __syncthreads();
    return *s_nc;
}

// Step 5 for class j of frame f, by a workgroup of THREADS threads: s_kmask[b] = the kept sorted positions of block b (of nblk),
// s_row[p] = the source row of sorted position p in its low 32 bits, s_box[p] = its BEV box (NULL: read from pred_bv).
// Starts behind a barrier of the caller's.
template <int THREADS, typename RowT>
__device__ __forceinline__ void dp_emit(const DetectPostDev &d, const int j, const int f, const int nblk, const unsigned long long *s_kmask,
                                        unsigned short *s_kpos, const RowT *s_row, const float4 *s_box)
{
    constexpr int WAVES = THREADS / 64;
    const int t = threadIdx.x, lane = t & 63, K = d.K, cap = d.cap;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const long long row0 = (long long)f * cap;
    int kc = 0;
    for (int b = 0; b < nblk; ++b) {
        const unsigned long long km = s_kmask[b];
        if (wave == b % WAVES && ((km >> lane) & 1ull))
            s_kpos[kc + __popcll(km & ((1ull << lane) - 1ull))] = (unsigned short)(64 * b + lane);
        kc += __popcll(km);
    }
    __syncthreads();
    const long long o = ((long long)f * K + j) * cap;
    if (t == 0) d.det_count[(long long)f * K + j] = kc;
    for (int e = t; e < kc; e += THREADS) d.det_row[o + e] = (int)(unsigned)s_row[s_kpos[e]];
    for (int e = t; e < kc * 5; e += THREADS) {
        const int slot = e / 5, c = e - slot * 5, p = s_kpos[slot];
        const int row = (int)(unsigned)s_row[p];
        float v;
        if (c == 4) v = d.cls_prob[(row0 + row) * K + j];
        else if (s_box) v = reinterpret_cast<const float *>(&s_box[p])[c];
        else v = d.pred_bv[(row0 + row) * (4 * K) + 4 * j + c];
        d.det_bv[o * 5 + e] = v;
    }
    for (int e = t; e < kc * 25; e += THREADS) {
        const int slot = e / 25, c = e - slot * 25;
        const int row = (int)(unsigned)s_row[s_kpos[slot]];
        const float sc = d.cls_prob[(row0 + row) * K + j];
        d.det_cnr[o * 25 + e] = c < 24 ? d.corners[(row0 + row) * 24 + c] : sc;
        if (d.pred_cnr_r) d.det_cnr_r[o * 25 + e] = c < 24 ? d.pred_cnr_r[(row0 + row) * (24 * K) + 24 * j + c] : sc;
    }
}
