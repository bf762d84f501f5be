// KITTI object evaluation on the device: bird's-eye-view and 3D average precision of LIDAR-frame corner detections
// (DESIGN.md §3.12).  Three launches over a whole split, frames as CSR ranges (det_off / gt_off / pair_off):
//
//   kitti_overlap_kernel   one 64-lane workgroup per frame: iou_bev / iou_3d of every (det, gt) pair of the frame, stored as
//                          the frame's D x G row-major block at pair_off[f] (two planes: bev | 3d), plus every detection's
//                          image-box height.
//   kitti_match_kernel     pass 1 (no false positives): one wave per (frame, metric, difficulty); one slot per GT receives the
//                          score of the detection matched to it as a true positive, or -inf.
//   kitti_count_kernel     pass 2: one 256-lane workgroup per (frame, metric, difficulty), its four waves take the score
//                          thresholds round robin; integer tp / fp / fn per (metric, difficulty, threshold) by atomics.
//
// Operation order of the overlap (all f64 from the f32 corners; tests/kitti_eval_restatement.py follows it line by line):
//   box  (x0..x7, y0..y7, z0..z7) f32.  Any non-finite value in either box -> both IoUs 0.
//   footprint  v_k = (x_k, y_k), k = 0..3.  s = 0; for k = 0..3: s = s + (x_k * y_n - x_n * y_k), n = (k + 1) % 4; A = 0.5 * s.
//              if A < 0: vertices reversed (v3, v2, v1, v0) and A = -A.
//   height     lo = z0, hi = z0; for k = 1..7: if z_k < lo: lo = z_k; if z_k > hi: hi = z_k.
//   clip       P = footprint of a; for each edge i = 0..3 of b in order (b0 = w_i, b1 = w_{(i+1)%4}): ex = b1x - b0x,
//              ey = b1y - b0y; Q = []; for j = 0..n-1 (p = P_j, q = P_{(j+1)%n}): cp = ex * (py - b0y) - ey * (px - b0x),
//              cq likewise for q; if cp >= 0: Q += p; if (cp >= 0) != (cq >= 0): t = cp / (cp - cq),
//              Q += (px + t * (qx - px), py + t * (qy - py)).  P = Q.
//   I          shoelace of the final P (sequential k = 0..n-1, same term as the footprint, 0 for n = 0) times 0.5;
//              if !(I > 0): I = 0.
//   iou_bev    U = (A_a + A_b) - I;  U > 0 ? I / U : 0.
//   iou_3d     h = min(hi_a, hi_b) - max(lo_a, lo_b); if h < 0: h = 0.  VI = I * h; V = A * (hi - lo);
//              U = (V_a + V_b) - VI;  U > 0 ? VI / U : 0.
// A convex 4-gon clipped by 4 half-planes keeps at most 1.5 n vertices per stage (4 -> 6 -> 9 -> 13 -> 19); the three stored
// stages fit 16 slots, the last stage is never stored: its shoelace is accumulated as the vertices come out.
//
// Detection image height: the 8 corners through proj_matrix / image_point (geometry.h, the proposal layer's projection),
// lo / hi of the 8 image rows as above, both clipped to [0, img_height - 1], height = hi - lo; 0 if anything is non-finite.
//
// Matching (KITTI object devkit rules, restated; difficulty e / m / h): MIN_HEIGHT 40 / 25 / 25, MAX_OCCLUSION 0 / 1 / 2,
// MAX_TRUNCATION 0.15f / 0.30f / 0.50f (compared in f32, the label's decimal value).  GT flag: the evaluated class ->
// (occ > MAX_OCC || trunc > MAX_TRUNC || y2 - y1 <= MIN_HEIGHT) ? 1 : 0; the neighbouring class -> 1; anything else -> -1
// (skipped).  Detection flag: height < MIN_HEIGHT ? 1 : 0.  For each GT in order, over the unassigned detections with
// iou > min_overlap:
//   pass 1   the highest score (first index on a tie; only scores > -1e7, as the devkit's NO_DETECTION start value).
//   pass 2   detections with score < t are not candidates; the flag-0 detection with the largest IoU (first index on a
//            tie), else the first flag-1 one.
//   no match and GT flag 0 -> fn; a match with GT flag 1 or detection flag 1 -> the detection is consumed, nothing counted;
//   any other match -> tp (pass 1: the GT's slot = the detection's score).  Pass 2 then counts every unassigned flag-0
//   detection with !(score < t) as fp.
// Lanes hold detections j = 64 c + lane (c < 32: at most MV3D_KITTI_MAX_DETS detections per frame); the argmax / first-index
// reductions across lanes give exactly the sequential scan's pick.
// This is the only statement of the rule: ke_match_wave is pass 1 and ke_count_wave pass 2 for every metric.  A kernel hands them
// a source object with the three things BEV / 3D and 2D differ in: overlap(j) with the current object (set by object(g)),
// ignored(j, MIN_HEIGHT), and the pass-2 hooks true_positive(g, j) and keeps_fp(j) on a counted fp ("statistics" below for 2D).
//
// 2D detection and orientation (AP_2D, AOS), three more launches over the same split plus a mv3d_kitti_image_split:
//
//   kitti_image_box_kernel  one lane per detection: its image box (x1, y1, x2, y2) and camera box (h, w, l, x, y, z, ry, alpha).
//   kitti_match_2d_kernel   pass 1 as kitti_match_kernel, one wave per (frame, difficulty), the 2D IoU computed on the fly from
//                           the frame's boxes (staged in LDS per wave when the frame has <= KE2_MATCH_LDS detections).
//   kitti_count_2d_kernel   pass 2 as kitti_count_kernel, one 256-lane workgroup per (frame, difficulty), plus the DontCare rule
//                           and the per-frame orientation similarity sum S_f[t] (no float atomics).
//
// Operation order (all f64 from the f32 inputs, no fma; tests/kitti_eval_image_restatement.py follows it line by line):
//   camera corners  R = Tr_velo_to_cam[:, :3] (calib row 3); c_j = ((R[i][0] * x_j + R[i][1] * y_j) + R[i][2] * z_j), i = 0..2
//                   (the inverse of mv3d_gt_encode's inv(R), translation dropped as there).
//   image box       q_r = (((P[r][0] * c0 + P[r][1] * c1) + P[r][2] * c2) + P[r][3]) with P = P2 (calib row 0); u = q0 / q2,
//                   v = q1 / q2; x1 / x2 = min / max of the 8 u, y1 / y2 of the 8 v (k = 0 first, then strict < / >), each clipped
//                   to [0, W - 1] / [0, H - 1] (image_shape (H, W) of the frame).  All zeros if any corner, u or v is non-finite
//                   or any corner has c2 <= 0.
//   camera box      mean4(a, b, c, d) = ((a + b) + (c + d)) / 4; gt_encode's local corner order: front {0,1,4,5}, back {2,3,6,7},
//                   +w/2 side {0,3,4,7}, -w/2 side {1,2,5,6}, bottom {0,1,2,3}, top {4,5,6,7}.  (x, y, z) = mean4 of the bottom
//                   corners; d = mean4(front) - mean4(back), l = sqrt(d.x * d.x + d.z * d.z), ry = atan2(-d.z, d.x);
//                   e = mean4(+side) - mean4(-side), w = sqrt(e.x * e.x + e.z * e.z); h = mean4(bottom y) - mean4(top y);
//                   alpha = ry - atan2(x, z), then alpha >= pi: - 2 pi, else alpha < -pi: + 2 pi.
//   2D overlap      (the devkit's boxoverlap, no +1 pixel) iw = min(x2) - max(x1), ih = min(y2) - max(y1); iw <= 0 or ih <= 0 -> 0;
//                   inter = iw * ih; A = (x2 - x1) * (y2 - y1); IoU = inter / ((A_det + A_gt) - inter); DontCare overlap =
//                   inter / A_det.  Object boxes: the label's (x1, y1, x2, y2) in f32.
//   statistics      the flags and passes above with the 2D IoU; a detection is ignored when y2 - y1 of its image box < MIN_HEIGHT.
//                   Pass 2 then takes out of fp every counted fp detection whose DontCare overlap with any of the frame's DontCare
//                   boxes is > min_overlap, and sums, over the true positives in object order, s = s + (1 + cos(a_gt - a_det)) / 2
//                   (a_gt the label's alpha in f32) into S_f[t].
#include "box_iou.h"

#define KE_COUNT_WAVES 4
#define KE_LDS_IOU 4096     // doubles of one frame's IoU block staged in LDS by the count kernel (32 KiB)

__constant__ int c_min_height[3] = {40, 25, 25};
__constant__ int c_max_occ[3] = {0, 1, 2};
__constant__ float c_max_trunc[3] = {0.15f, 0.30f, 0.50f};

__global__ __launch_bounds__(KE_OVERLAP_THREADS) void kitti_overlap_kernel(
    int F, const int32_t *__restrict__ offs, const float *__restrict__ det_cnr, const float *__restrict__ calib,
    const float *__restrict__ gt_cnr, double img_hmax, double *__restrict__ iou, long long P, double *__restrict__ det_height)
{
    __shared__ double poly[2 * KE_MAXV * 2 * KE_OVERLAP_THREADS];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int32_t *det_off = offs, *gt_off = offs + (F + 1), *pair_off = offs + 2 * (F + 1);
    const int d0 = det_off[f], D = det_off[f + 1] - d0, g0 = gt_off[f], G = gt_off[f + 1] - g0;
    const long long p0 = pair_off[f];
    for (int p = lane; p < D * G; p += KE_OVERLAP_THREADS) {
        const int d = p / G, g = p - d * G;
        KeBox a, b;
        const bool fa = ke_load(det_cnr + 24 * (long long)(d0 + d), a);
        const bool fb = ke_load(gt_cnr + 24 * (long long)(g0 + g), b);
        double ib = 0.0, i3 = 0.0;
        if (fa && fb) ke_iou(a, b, poly, lane, ib, i3);
        iou[p0 + p] = ib;
        iou[P + p0 + p] = i3;
    }
    float M[12];
    proj_matrix(calib + 48 * (long long)f, M);
    for (int d = lane; d < D; d += KE_OVERLAP_THREADS) {
        const float *c = det_cnr + 24 * (long long)(d0 + d);
        bool fin = true;
        double lo = 0.0, hi = 0.0;
        for (int k = 0; k < 8; ++k) {
            fin = fin && isfinite(c[k]) && isfinite(c[8 + k]) && isfinite(c[16 + k]);
            double px, py;
            image_point(M, c[k], c[8 + k], c[16 + k], px, py);
            fin = fin && isfinite(py);
            if (k == 0) { lo = hi = py; }
            else {
                if (py < lo) lo = py;
                if (py > hi) hi = py;
            }
        }
        double h = 0.0;
        if (fin) {
            lo = lo < 0.0 ? 0.0 : (lo > img_hmax ? img_hmax : lo);
            hi = hi < 0.0 ? 0.0 : (hi > img_hmax ? img_hmax : hi);
            h = hi - lo;
        }
        det_height[d0 + d] = h;
    }
}

// GT flag of object g for difficulty `diff`: 0 counted, 1 ignored, -1 skipped
__device__ __forceinline__ int ke_gt_flag(const int32_t *__restrict__ gt_cls, const float *__restrict__ gt_attr, int g, int diff,
                                          int eval_class, int neighbor_class)
{
    const int cls = gt_cls[g];
    if (cls == eval_class) {
        const float *a = gt_attr + 4 * (long long)g;
        const double height = (double)a[3] - (double)a[2];
        return (a[1] > (float)c_max_occ[diff] || a[0] > c_max_trunc[diff] || height <= (double)c_min_height[diff]) ? 1 : 0;
    }
    return cls == neighbor_class ? 1 : -1;
}

__device__ __forceinline__ void ke_argmax(double &key, int &idx)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double k2 = __shfl_xor(key, o);
        const int i2 = __shfl_xor(idx, o);
        if (k2 > key || (k2 == key && i2 < idx)) { key = k2; idx = i2; }
    }
}

__device__ __forceinline__ int ke_min(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int v2 = __shfl_xor(v, o);
        v = v2 < v ? v2 : v;
    }
    return v;
}

// ------------------------------------------------------------------ the two statistics passes, one body each
// One wave runs one task: a frame (detections d0 .. d0 + D, objects g0 .. g0 + G) at one difficulty; `Src` is its overlap source
// (header comment, "Matching").  Wave-level operations only (shuffles, ballots, lane-0 stores): barriers stay in the kernels.
struct KeTask {
    int d0, D, g0, G, diff, eval_class, neighbor_class;
    const float *score; const int32_t *cls; const float *attr;     // det_score, gt_cls, gt_attr of the split
    double min_overlap, min_h;                                      // min_h: MIN_HEIGHT of the difficulty
    __device__ __forceinline__ int flag(int g) const { return ke_gt_flag(cls, attr, g0 + g, diff, eval_class, neighbor_class); }
};

// bit c: pred(j) of this lane's detection j = 64 c + lane of chunk c (0 past the frame's D detections)
template <class Pred>
__device__ __forceinline__ uint32_t ke_chunk_mask(int D, int lane, Pred pred)
{
    uint32_t m = 0u;
    for (int c = 0; c < (D + 63) >> 6; ++c)
        if (64 * c + lane < D && pred(64 * c + lane)) m |= 1u << c;
    return m;
}

template <class Src>
__device__ __forceinline__ void ke_match_wave(Src &src, const KeTask &k, int lane, float *__restrict__ out)
{
    const int nch = (k.D + 63) >> 6;
    uint32_t assigned = 0u;
    for (int g = 0; g < k.G; ++g) {
        const int flag = k.flag(g);
        float slot = -INFINITY;
        if (flag >= 0) {
            src.object(g);
            double best = -INFINITY;
            int bi = INT32_MAX;
            for (int c = 0; c < nch; ++c) {
                const int j = 64 * c + lane;
                if (j < k.D && !((assigned >> c) & 1u) && src.overlap(j) > k.min_overlap) {
                    const double sc = (double)k.score[k.d0 + j];
                    if (sc > -10000000.0 && sc > best) { best = sc; bi = j; }
                }
            }
            ke_argmax(best, bi);
            if (bi != INT32_MAX) {
                if (lane == (bi & 63)) assigned |= 1u << (bi >> 6);
                const bool ign_det = src.ignored(bi, k.min_h);
                if (flag == 0 && !ign_det) slot = k.score[k.d0 + bi];
            }
        }
        if (lane == 0) out[g] = slot;
    }
}

// pass 2 at one score threshold t (ign: the mask of src.ignored): the task's tp | fp | fn into o[0..2], integer atomics by lane 0
template <class Src>
__device__ __forceinline__ void ke_count_wave(Src &src, const KeTask &k, int lane, uint32_t ign, float t, int32_t *__restrict__ o)
{
    const int nch = (k.D + 63) >> 6;
    const uint32_t cand = ke_chunk_mask(k.D, lane, [&](int j) { return !(k.score[k.d0 + j] < t); });
    uint32_t assigned = 0u;
    int tp = 0, fp = 0, fn = 0;
    for (int g = 0; g < k.G; ++g) {
        const int flag = k.flag(g);
        if (flag < 0) continue;
        src.object(g);
        double best = -INFINITY;
        int bi = INT32_MAX, first_ign = INT32_MAX;
        for (int c = 0; c < nch; ++c) {
            if (!(((cand & ~assigned) >> c) & 1u)) continue;
            const int j = 64 * c + lane;
            const double o = src.overlap(j);
            if (!(o > k.min_overlap)) continue;
            if ((ign >> c) & 1u) {
                if (first_ign == INT32_MAX) first_ign = j;
            } else if (o > best) {
                best = o; bi = j;
            }
        }
        ke_argmax(best, bi);
        if (bi == INT32_MAX) bi = ke_min(first_ign);
        if (bi == INT32_MAX) {
            if (flag == 0) ++fn;
        } else {
            if (lane == (bi & 63)) assigned |= 1u << (bi >> 6);
            if (flag == 0 && !src.ignored(bi, k.min_h)) {
                ++tp;
                src.true_positive(g, bi);
            }
        }
    }
    for (int c = 0; c < nch; ++c)                       // every unassigned, not ignored candidate that the source keeps
        fp += __popcll(__ballot((((cand & ~assigned & ~ign) >> c) & 1u) != 0u && src.keeps_fp(64 * c + lane)));
    if (lane == 0) {
        if (tp) atomicAdd(o, tp);
        if (fp) atomicAdd(o + 1, fp);
        if (fn) atomicAdd(o + 2, fn);
    }
}

// BEV / 3D: the frame's D x G block of one metric (global memory or LDS) and the overlap kernel's image heights; no hooks
struct KeBlockSource {
    const double *blk, *height;
    int d0, G, g;
    __device__ __forceinline__ void object(int gi) { g = gi; }
    __device__ __forceinline__ double overlap(int j) const { return blk[(long long)j * G + g]; }
    __device__ __forceinline__ bool ignored(int j, double min_h) const { return height[d0 + j] < min_h; }
    __device__ __forceinline__ void true_positive(int, int) {}
    __device__ __forceinline__ bool keeps_fp(int) const { return true; }
};

__global__ __launch_bounds__(256) void kitti_match_kernel(
    int F, const int32_t *__restrict__ offs, const double *__restrict__ iou, long long P, const float *__restrict__ det_score,
    const double *__restrict__ det_height, const int32_t *__restrict__ gt_cls, const float *__restrict__ gt_attr, int Gtot,
    int eval_class, int neighbor_class, double min_overlap, float *__restrict__ matched)
{
    const int task = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (task >= F * 6) return;
    const int f = task / 6, metric = (task / 3) % 2, diff = task % 3;
    const int32_t *det_off = offs, *gt_off = offs + (F + 1), *pair_off = offs + 2 * (F + 1);
    const int d0 = det_off[f], D = det_off[f + 1] - d0, g0 = gt_off[f], G = gt_off[f + 1] - g0;
    const KeTask k{d0, D, g0, G, diff, eval_class, neighbor_class, det_score, gt_cls, gt_attr, min_overlap, (double)c_min_height[diff]};
    KeBlockSource src{iou + metric * P + pair_off[f], det_height, d0, G, 0};
    ke_match_wave(src, k, lane, matched + (long long)(metric * 3 + diff) * Gtot + g0);
}

__global__ __launch_bounds__(64 * KE_COUNT_WAVES) void kitti_count_kernel(
    int F, const int32_t *__restrict__ offs, const double *__restrict__ iou, long long P, const float *__restrict__ det_score,
    const double *__restrict__ det_height, const int32_t *__restrict__ gt_cls, const float *__restrict__ gt_attr,
    int eval_class, int neighbor_class, double min_overlap, const float *__restrict__ thresholds, const int32_t *__restrict__ num_thr,
    int32_t *__restrict__ counts)
{
    __shared__ double s_iou[KE_LDS_IOU];
    const int task = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = task / 6, metric = (task / 3) % 2, diff = task % 3, md = metric * 3 + diff;
    const int32_t *det_off = offs, *gt_off = offs + (F + 1), *pair_off = offs + 2 * (F + 1);
    const int d0 = det_off[f], D = det_off[f + 1] - d0, g0 = gt_off[f], G = gt_off[f + 1] - g0;
    int T = num_thr[md];
    T = T < 0 ? 0 : (T > MV3D_KITTI_NUM_SAMPLE_PTS ? MV3D_KITTI_NUM_SAMPLE_PTS : T);
    if (D == 0 && G == 0) return;
    const double *gblk = iou + metric * P + pair_off[f];
    const double *blk = gblk;
    if ((long long)D * G <= KE_LDS_IOU) {              // (workgroup-uniform) stage the frame's block in LDS
        for (int p = threadIdx.x; p < D * G; p += 64 * KE_COUNT_WAVES) s_iou[p] = gblk[p];
        __syncthreads();
        blk = s_iou;
    }
    const KeTask k{d0, D, g0, G, diff, eval_class, neighbor_class, det_score, gt_cls, gt_attr, min_overlap, (double)c_min_height[diff]};
    KeBlockSource src{blk, det_height, d0, G, 0};
    const uint32_t ign = ke_chunk_mask(D, lane, [&](int j) { return src.ignored(j, k.min_h); });
    for (int ti = wave; ti < T; ti += KE_COUNT_WAVES) {
        const int slot = md * MV3D_KITTI_NUM_SAMPLE_PTS + ti;
        ke_count_wave(src, k, lane, ign, thresholds[slot], counts + 3 * slot);
    }
}

// ------------------------------------------------------------------ 2D detection and orientation
#define KE2_MATCH_LDS 384   // detection boxes per wave staged in LDS by the 2D pass 1 (4 doubles each: 12 KiB per wave)
#define KE2_COUNT_LDS 1024  // detection boxes of one frame staged in LDS by the 2D pass 2 (32 KiB)

__device__ __forceinline__ double ke_mean4(double a, double b, double c, double d) { return ((a + b) + (c + d)) / 4.0; }

__global__ __launch_bounds__(256) void kitti_image_box_kernel(
    int F, int N, const int32_t *__restrict__ det_off, const float *__restrict__ det_cnr, const float *__restrict__ calib,
    const int32_t *__restrict__ image_shape, double *__restrict__ det_box, double *__restrict__ det_cam)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    int lo = 0, hi = F;                                 // the frame of detection i: det_off[lo] <= i < det_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (det_off[mid] <= i) lo = mid;
        else hi = mid;
    }
    const float *P = calib + 48 * (long long)lo, *Tr = P + 36;
    const float *c = det_cnr + 24 * (long long)i;
    double cx[8], cy[8], cz[8];
    double x1 = 0.0, y1 = 0.0, x2 = 0.0, y2 = 0.0;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float fx = c[k], fy = c[8 + k], fz = c[16 + k];
        ok = ok && isfinite(fx) && isfinite(fy) && isfinite(fz);
        const double px = fx, py = fy, pz = fz;
        cx[k] = ((double)Tr[0] * px + (double)Tr[1] * py) + (double)Tr[2] * pz;
        cy[k] = ((double)Tr[4] * px + (double)Tr[5] * py) + (double)Tr[6] * pz;
        cz[k] = ((double)Tr[8] * px + (double)Tr[9] * py) + (double)Tr[10] * pz;
        const double q0 = (((double)P[0] * cx[k] + (double)P[1] * cy[k]) + (double)P[2] * cz[k]) + (double)P[3];
        const double q1 = (((double)P[4] * cx[k] + (double)P[5] * cy[k]) + (double)P[6] * cz[k]) + (double)P[7];
        const double q2 = (((double)P[8] * cx[k] + (double)P[9] * cy[k]) + (double)P[10] * cz[k]) + (double)P[11];
        const double u = q0 / q2, v = q1 / q2;
        ok = ok && cz[k] > 0.0 && isfinite(u) && isfinite(v);
        if (k == 0) { x1 = x2 = u; y1 = y2 = v; }
        else {
            if (u < x1) x1 = u;
            if (u > x2) x2 = u;
            if (v < y1) y1 = v;
            if (v > y2) y2 = v;
        }
    }
    double *b = det_box + 4 * (long long)i;
    if (ok) {
        const double wm = (double)(image_shape[2 * lo + 1] - 1), hm = (double)(image_shape[2 * lo] - 1);
        b[0] = x1 < 0.0 ? 0.0 : (x1 > wm ? wm : x1);
        b[1] = y1 < 0.0 ? 0.0 : (y1 > hm ? hm : y1);
        b[2] = x2 < 0.0 ? 0.0 : (x2 > wm ? wm : x2);
        b[3] = y2 < 0.0 ? 0.0 : (y2 > hm ? hm : y2);
    } else {
        b[0] = b[1] = b[2] = b[3] = 0.0;
    }
    const double x = ke_mean4(cx[0], cx[1], cx[2], cx[3]), y = ke_mean4(cy[0], cy[1], cy[2], cy[3]);
    const double z = ke_mean4(cz[0], cz[1], cz[2], cz[3]);
    const double dx = ke_mean4(cx[0], cx[1], cx[4], cx[5]) - ke_mean4(cx[2], cx[3], cx[6], cx[7]);
    const double dz = ke_mean4(cz[0], cz[1], cz[4], cz[5]) - ke_mean4(cz[2], cz[3], cz[6], cz[7]);
    const double ex = ke_mean4(cx[0], cx[3], cx[4], cx[7]) - ke_mean4(cx[1], cx[2], cx[5], cx[6]);
    const double ez = ke_mean4(cz[0], cz[3], cz[4], cz[7]) - ke_mean4(cz[1], cz[2], cz[5], cz[6]);
    const double ry = atan2(-dz, dx);
    double alpha = ry - atan2(x, z);
    if (alpha >= M_PI) alpha -= 2.0 * M_PI;
    else if (alpha < -M_PI) alpha += 2.0 * M_PI;
    double *o = det_cam + 8 * (long long)i;
    o[0] = y - ke_mean4(cy[4], cy[5], cy[6], cy[7]);
    o[1] = sqrt(ex * ex + ez * ez);
    o[2] = sqrt(dx * dx + dz * dz);
    o[3] = x; o[4] = y; o[5] = z; o[6] = ry; o[7] = alpha;
}

// inter = iw * ih of detection box a (f64) and box (b0..b3) (f32 label values), 0 if they do not overlap
__device__ __forceinline__ double ke_inter2d(const double *a, double b0, double b1, double b2, double b3)
{
    const double iw = (a[2] < b2 ? a[2] : b2) - (a[0] > b0 ? a[0] : b0);
    const double ih = (a[3] < b3 ? a[3] : b3) - (a[1] > b1 ? a[1] : b1);
    if (iw <= 0.0 || ih <= 0.0) return 0.0;
    return iw * ih;
}

__device__ __forceinline__ double ke_iou2d(const double *a, double b0, double b1, double b2, double b3, double area_b)
{
    const double inter = ke_inter2d(a, b0, b1, b2, b3);
    if (inter == 0.0) return 0.0;
    return inter / (((a[2] - a[0]) * (a[3] - a[1]) + area_b) - inter);
}

// 2D: the overlap computed from the frame's detection image boxes (global memory or LDS) and the object's label box, loaded
// once per object; a detection is ignored by the height of its image box
struct KeBoxSource {
    const double *box;
    const float *gt_box;
    int g0;
    double b0, b1, b2, b3, area_b;
    __device__ __forceinline__ void object(int g)
    {
        const float *gb = gt_box + 4 * (long long)(g0 + g);
        b0 = gb[0]; b1 = gb[1]; b2 = gb[2]; b3 = gb[3]; area_b = (b2 - b0) * (b3 - b1);
    }
    __device__ __forceinline__ double overlap(int j) const { return ke_iou2d(box + 4 * j, b0, b1, b2, b3, area_b); }
    __device__ __forceinline__ bool ignored(int j, double min_h) const { return box[4 * j + 3] - box[4 * j + 1] < min_h; }
};

// 2D pass 2: a true positive adds its orientation similarity to s; a counted fp stays unless a DontCare box covers it
struct KeBoxCountSource : KeBoxSource {
    const float *gt_alpha, *dc_box;
    const double *det_cam;
    int d0, k0, K;
    double min_overlap, s;
    __device__ __forceinline__ void true_positive(int g, int j)
    {
        s = s + (1.0 + cos((double)gt_alpha[g0 + g] - det_cam[8 * (long long)(d0 + j) + 7])) / 2.0;
    }
    __device__ __forceinline__ bool keeps_fp(int j) const     // the devkit's DontCare ("stuff") rule
    {
        const double *a = box + 4 * j;
        const double area_a = (a[2] - a[0]) * (a[3] - a[1]);
        bool stuff = false;
        for (int k = 0; k < K && !stuff; ++k) {
            const float *q = dc_box + 4 * (long long)(k0 + k);
            const double inter = ke_inter2d(a, q[0], q[1], q[2], q[3]);
            stuff = inter > 0.0 && inter / area_a > min_overlap;
        }
        return !stuff;
    }
};

__global__ __launch_bounds__(256) void kitti_match_2d_kernel(
    int F, const int32_t *__restrict__ offs, const double *__restrict__ det_box, const float *__restrict__ det_score,
    const int32_t *__restrict__ gt_cls, const float *__restrict__ gt_attr, const float *__restrict__ gt_box, int Gtot,
    int eval_class, int neighbor_class, double min_overlap, float *__restrict__ matched)
{
    __shared__ double s_box[4][4 * KE2_MATCH_LDS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, task = blockIdx.x * 4 + wave;
    const bool active = task < F * 3;
    const int f = active ? task / 3 : 0, diff = task % 3;
    const int32_t *det_off = offs, *gt_off = offs + (F + 1);
    const int d0 = det_off[f], D = det_off[f + 1] - d0, g0 = gt_off[f], G = gt_off[f + 1] - g0;
    const double *box = det_box + 4 * (long long)d0;
    if (active && D <= KE2_MATCH_LDS) {
        for (int p = lane; p < 4 * D; p += 64) s_box[wave][p] = box[p];
        box = s_box[wave];
    }
    __syncthreads();
    if (!active) return;                               // only behind the barrier: the idle waves of the last workgroup reach it too
    const KeTask k{d0, D, g0, G, diff, eval_class, neighbor_class, det_score, gt_cls, gt_attr, min_overlap, (double)c_min_height[diff]};
    KeBoxSource src{box, gt_box, g0};
    ke_match_wave(src, k, lane, matched + (long long)diff * Gtot + g0);
}

__global__ __launch_bounds__(64 * KE_COUNT_WAVES) void kitti_count_2d_kernel(
    int F, const int32_t *__restrict__ offs, const double *__restrict__ det_box, const double *__restrict__ det_cam,
    const float *__restrict__ det_score, const int32_t *__restrict__ gt_cls, const float *__restrict__ gt_attr,
    const float *__restrict__ gt_box, const float *__restrict__ gt_alpha, const int32_t *__restrict__ dc_off,
    const float *__restrict__ dc_box, int eval_class, int neighbor_class, double min_overlap, const float *__restrict__ thresholds,
    const int32_t *__restrict__ num_thr, int32_t *__restrict__ counts, double *__restrict__ sim)
{
    __shared__ double s_box[4 * KE2_COUNT_LDS];
    const int task = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = task / 3, diff = task % 3;
    const int32_t *det_off = offs, *gt_off = offs + (F + 1);
    const int d0 = det_off[f], D = det_off[f + 1] - d0, g0 = gt_off[f], G = gt_off[f + 1] - g0;
    const int k0 = dc_off[f], K = dc_off[f + 1] - k0;
    int T = num_thr[diff];
    T = T < 0 ? 0 : (T > MV3D_KITTI_NUM_SAMPLE_PTS ? MV3D_KITTI_NUM_SAMPLE_PTS : T);
    if (D == 0 && G == 0) return;
    const double *box = det_box + 4 * (long long)d0;
    if (D <= KE2_COUNT_LDS) {                          // (workgroup-uniform) stage the frame's detection boxes in LDS
        for (int p = threadIdx.x; p < 4 * D; p += 64 * KE_COUNT_WAVES) s_box[p] = box[p];
        __syncthreads();
        box = s_box;
    }
    const KeTask k{d0, D, g0, G, diff, eval_class, neighbor_class, det_score, gt_cls, gt_attr, min_overlap, (double)c_min_height[diff]};
    KeBoxCountSource src{{box, gt_box, g0}, gt_alpha, dc_box, det_cam, d0, k0, K, min_overlap};
    const uint32_t ign = ke_chunk_mask(D, lane, [&](int j) { return src.ignored(j, k.min_h); });
    for (int ti = wave; ti < T; ti += KE_COUNT_WAVES) {
        const int slot = diff * MV3D_KITTI_NUM_SAMPLE_PTS + ti;
        src.s = 0.0;
        ke_count_wave(src, k, lane, ign, thresholds[slot], counts + 3 * slot);
        if (lane == 0) sim[(long long)task * MV3D_KITTI_NUM_SAMPLE_PTS + ti] = src.s;
    }
}

// ------------------------------------------------------------------ C-ABI
static int ke_validate_split(const mv3d_kitti_split *s, bool check_pairs, long long num_pairs)
{
    if (!s || s->num_frames < 0 || s->num_dets < 0 || s->num_gts < 0 || !s->det_off || !s->gt_off) return MV3D_ERR_INVALID_ARG;
    const int F = s->num_frames;
    if (s->det_off[0] != 0 || s->gt_off[0] != 0 || s->det_off[F] != s->num_dets || s->gt_off[F] != s->num_gts) return MV3D_ERR_INVALID_ARG;
    long long pairs = 0;
    for (int f = 0; f < F; ++f) {
        const long long D = (long long)s->det_off[f + 1] - s->det_off[f], G = (long long)s->gt_off[f + 1] - s->gt_off[f];
        if (D < 0 || G < 0 || D > MV3D_KITTI_MAX_DETS) return MV3D_ERR_INVALID_ARG;
        pairs += D * G;
    }
    if (check_pairs && (pairs != num_pairs || pairs > INT32_MAX)) return MV3D_ERR_INVALID_ARG;
    if (F > 0 && !s->offsets_dev) return MV3D_ERR_INVALID_ARG;
    if (s->num_dets > 0 && (!s->det_cnr_dev || !s->det_score_dev)) return MV3D_ERR_INVALID_ARG;
    if (s->num_gts > 0 && (!s->gt_cnr_dev || !s->gt_cls_dev || !s->gt_attr_dev)) return MV3D_ERR_INVALID_ARG;
    if (F > 0 && !s->calib_dev) return MV3D_ERR_INVALID_ARG;
    return MV3D_OK;
}

static int ke_validate(const mv3d_kitti_split *s, long long num_pairs) { return ke_validate_split(s, true, num_pairs); }

extern "C" int mv3d_kitti_eval_overlaps(const mv3d_kitti_split *split, long long num_pairs, double *iou_dev, double *det_height_dev,
                                        void *stream)
{
    const int rc = ke_validate(split, num_pairs);
    if (rc != MV3D_OK) return rc;
    if (split->img_height < 1) return MV3D_ERR_INVALID_ARG;
    if ((num_pairs > 0 && !iou_dev) || (split->num_dets > 0 && !det_height_dev)) return MV3D_ERR_INVALID_ARG;
    if (split->num_frames == 0) return MV3D_OK;
    hipLaunchKernelGGL(kitti_overlap_kernel, dim3(split->num_frames), dim3(KE_OVERLAP_THREADS), 0, (hipStream_t)stream,
                       split->num_frames, split->offsets_dev, split->det_cnr_dev, split->calib_dev, split->gt_cnr_dev,
                       (double)(split->img_height - 1), iou_dev, num_pairs, det_height_dev);
    return mv3d_launch_status();
}

extern "C" int mv3d_kitti_eval_match(const mv3d_kitti_split *split, long long num_pairs, const double *iou_dev,
                                     const double *det_height_dev, int eval_class, int neighbor_class, double min_overlap,
                                     float *matched_dev, void *stream)
{
    const int rc = ke_validate(split, num_pairs);
    if (rc != MV3D_OK) return rc;
    if (!(min_overlap >= 0.0) || (num_pairs > 0 && !iou_dev) || (split->num_dets > 0 && !det_height_dev) ||
        (split->num_gts > 0 && !matched_dev))
        return MV3D_ERR_INVALID_ARG;
    if (split->num_frames == 0 || split->num_gts == 0) return MV3D_OK;
    const int tasks = split->num_frames * 6;
    hipLaunchKernelGGL(kitti_match_kernel, dim3((tasks + 3) / 4), dim3(256), 0, (hipStream_t)stream, split->num_frames,
                       split->offsets_dev, iou_dev, num_pairs, split->det_score_dev, det_height_dev, split->gt_cls_dev,
                       split->gt_attr_dev, split->num_gts, eval_class, neighbor_class, min_overlap, matched_dev);
    return mv3d_launch_status();
}

extern "C" int mv3d_kitti_eval_count(const mv3d_kitti_split *split, long long num_pairs, const double *iou_dev,
                                     const double *det_height_dev, int eval_class, int neighbor_class, double min_overlap,
                                     const float *thresholds_dev, const int32_t *num_thresholds_dev, int32_t *counts_dev,
                                     void *stream)
{
    const int rc = ke_validate(split, num_pairs);
    if (rc != MV3D_OK) return rc;
    if (!(min_overlap >= 0.0) || (num_pairs > 0 && !iou_dev) || (split->num_dets > 0 && !det_height_dev) || !thresholds_dev ||
        !num_thresholds_dev || !counts_dev)
        return MV3D_ERR_INVALID_ARG;
    MV3D_HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(int32_t) * 6 * MV3D_KITTI_NUM_SAMPLE_PTS * 3, (hipStream_t)stream));
    if (split->num_frames == 0) return MV3D_OK;
    hipLaunchKernelGGL(kitti_count_kernel, dim3(split->num_frames * 6), dim3(64 * KE_COUNT_WAVES), 0, (hipStream_t)stream,
                       split->num_frames, split->offsets_dev, iou_dev, num_pairs, split->det_score_dev, det_height_dev,
                       split->gt_cls_dev, split->gt_attr_dev, eval_class, neighbor_class, min_overlap, thresholds_dev,
                       num_thresholds_dev, counts_dev);
    return mv3d_launch_status();
}

// ------------------------------------------------------------------ C-ABI: 2D detection and orientation
static int ke_validate_image(const mv3d_kitti_split *s, const mv3d_kitti_image_split *im)
{
    const int rc = ke_validate_split(s, false, 0);
    if (rc != MV3D_OK) return rc;
    if (!im || im->num_dontcare < 0 || !im->dc_off) return MV3D_ERR_INVALID_ARG;
    const int F = s->num_frames;
    if (im->dc_off[0] != 0 || im->dc_off[F] != im->num_dontcare) return MV3D_ERR_INVALID_ARG;
    for (int f = 0; f < F; ++f)
        if (im->dc_off[f + 1] < im->dc_off[f]) return MV3D_ERR_INVALID_ARG;
    if (F > 0 && (!im->dc_off_dev || !im->image_shape_dev)) return MV3D_ERR_INVALID_ARG;
    if (s->num_gts > 0 && (!im->gt_box_dev || !im->gt_alpha_dev)) return MV3D_ERR_INVALID_ARG;
    if (im->num_dontcare > 0 && !im->dc_box_dev) return MV3D_ERR_INVALID_ARG;
    return MV3D_OK;
}

extern "C" int mv3d_kitti_eval_image_boxes(const mv3d_kitti_split *split, const mv3d_kitti_image_split *image, double *det_box_dev,
                                           double *det_cam_dev, void *stream)
{
    const int rc = ke_validate_image(split, image);
    if (rc != MV3D_OK) return rc;
    if (split->num_dets > 0 && (!det_box_dev || !det_cam_dev)) return MV3D_ERR_INVALID_ARG;
    if (split->num_dets == 0) return MV3D_OK;
    hipLaunchKernelGGL(kitti_image_box_kernel, dim3((split->num_dets + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       split->num_frames, split->num_dets, split->offsets_dev, split->det_cnr_dev, split->calib_dev,
                       image->image_shape_dev, det_box_dev, det_cam_dev);
    return mv3d_launch_status();
}

extern "C" int mv3d_kitti_eval_match_2d(const mv3d_kitti_split *split, const mv3d_kitti_image_split *image, const double *det_box_dev,
                                        int eval_class, int neighbor_class, double min_overlap, float *matched_dev, void *stream)
{
    const int rc = ke_validate_image(split, image);
    if (rc != MV3D_OK) return rc;
    if (!(min_overlap >= 0.0) || (split->num_dets > 0 && !det_box_dev) || (split->num_gts > 0 && !matched_dev))
        return MV3D_ERR_INVALID_ARG;
    if (split->num_frames == 0 || split->num_gts == 0) return MV3D_OK;
    const int tasks = split->num_frames * 3;
    hipLaunchKernelGGL(kitti_match_2d_kernel, dim3((tasks + 3) / 4), dim3(256), 0, (hipStream_t)stream, split->num_frames,
                       split->offsets_dev, det_box_dev, split->det_score_dev, split->gt_cls_dev, split->gt_attr_dev,
                       image->gt_box_dev, split->num_gts, eval_class, neighbor_class, min_overlap, matched_dev);
    return mv3d_launch_status();
}

extern "C" int mv3d_kitti_eval_count_2d(const mv3d_kitti_split *split, const mv3d_kitti_image_split *image, const double *det_box_dev,
                                        const double *det_cam_dev, int eval_class, int neighbor_class, double min_overlap,
                                        const float *thresholds_dev, const int32_t *num_thresholds_dev, int32_t *counts_dev,
                                        double *similarity_dev, void *stream)
{
    const int rc = ke_validate_image(split, image);
    if (rc != MV3D_OK) return rc;
    if (!(min_overlap >= 0.0) || (split->num_dets > 0 && (!det_box_dev || !det_cam_dev)) || !thresholds_dev || !num_thresholds_dev ||
        !counts_dev || (split->num_frames > 0 && !similarity_dev))
        return MV3D_ERR_INVALID_ARG;
    MV3D_HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(int32_t) * 3 * MV3D_KITTI_NUM_SAMPLE_PTS * 3, (hipStream_t)stream));
    if (split->num_frames == 0) return MV3D_OK;
    MV3D_HIP_TRY(hipMemsetAsync(similarity_dev, 0, sizeof(double) * 3 * MV3D_KITTI_NUM_SAMPLE_PTS * (size_t)split->num_frames,
                                (hipStream_t)stream));
    hipLaunchKernelGGL(kitti_count_2d_kernel, dim3(split->num_frames * 3), dim3(64 * KE_COUNT_WAVES), 0, (hipStream_t)stream,
                       split->num_frames, split->offsets_dev, det_box_dev, det_cam_dev, split->det_score_dev, split->gt_cls_dev,
                       split->gt_attr_dev, image->gt_box_dev, image->gt_alpha_dev, image->dc_off_dev, image->dc_box_dev, eval_class,
                       neighbor_class, min_overlap, thresholds_dev, num_thresholds_dev, counts_dev, similarity_dev);
    return mv3d_launch_status();
}
