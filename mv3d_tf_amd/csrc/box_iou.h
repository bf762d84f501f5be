// The oriented-box overlap shared by the KITTI evaluator (kitti_eval.hip) and the 3D proposal recall (proposal_recall_3d.hip):
// BEV and 3D IoU of two LIDAR-corner boxes, all f64 from the f32 corners.  The operation order is the one written out in the
// header comment of kitti_eval.hip ("Operation order of the overlap"); tests/kitti_eval_restatement.py::iou_pair follows it line
// by line.  One lane clips one pair; its polygon buffers live in LDS, `poly` = 2 * KE_MAXV * 2 * KE_OVERLAP_THREADS doubles
// (32 KiB) per wave, laid out [buffer][vertex][x|y][lane].
#pragma once
#include "geometry.h"

#define KE_MAXV 16
#define KE_OVERLAP_THREADS 64

struct KeBox {
    double x[4], y[4], area, lo, hi;
};

__device__ __forceinline__ bool ke_load(const float *__restrict__ c, KeBox &b)
{
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 24; ++k) fin = fin && isfinite(c[k]);
    double x[4], y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { x[k] = (double)c[k]; y[k] = (double)c[8 + k]; }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int n = (k + 1) & 3;
        s = s + (x[k] * y[n] - x[n] * y[k]);
    }
    double a = 0.5 * s;
    const bool rev = a < 0.0;
    if (rev) a = -a;
#pragma unroll
    for (int k = 0; k < 4; ++k) { b.x[k] = rev ? x[3 - k] : x[k]; b.y[k] = rev ? y[3 - k] : y[k]; }
    b.area = a;
    double lo = (double)c[16], hi = lo;
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        const double z = (double)c[16 + k];
        if (z < lo) lo = z;
        if (z > hi) hi = z;
    }
    b.lo = lo; b.hi = hi;
    return fin;
}

// this lane's vertex v of polygon buffer `buf` (LDS, [buf][vertex][x|y][lane])
#define KE_V(buf, v, comp) poly[(((buf) * KE_MAXV + (v)) * 2 + (comp)) * KE_OVERLAP_THREADS + lane]

__device__ __forceinline__ void ke_iou(const KeBox &a, const KeBox &b, double *poly, int lane, double &iou_bev, double &iou_3d)
{
    int n = 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) { KE_V(0, k, 0) = a.x[k]; KE_V(0, k, 1) = a.y[k]; }
    double s = 0.0, fx = 0.0, fy = 0.0, lx = 0.0, ly = 0.0;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int src = i & 1, dst = src ^ 1;
        const double b0x = b.x[i], b0y = b.y[i], ex = b.x[(i + 1) & 3] - b0x, ey = b.y[(i + 1) & 3] - b0y;
        int m = 0;
        for (int j = 0; j < n; ++j) {
            const int jn = (j + 1 == n) ? 0 : j + 1;
            const double px = KE_V(src, j, 0), py = KE_V(src, j, 1), qx = KE_V(src, jn, 0), qy = KE_V(src, jn, 1);
            const double cp = ex * (py - b0y) - ey * (px - b0x);
            const double cq = ex * (qy - b0y) - ey * (qx - b0x);
            auto emit = [&](double vx, double vy) {
                if (i < 3) {
                    if (m < KE_MAXV) { KE_V(dst, m, 0) = vx; KE_V(dst, m, 1) = vy; }
                    ++m;
                } else {                                   // last stage: shoelace as the vertices come out
                    if (cnt == 0) { fx = vx; fy = vy; }
                    else s = s + (lx * vy - vx * ly);
                    lx = vx; ly = vy;
                    ++cnt;
                }
            };
            if (cp >= 0.0) emit(px, py);
            if ((cp >= 0.0) != (cq >= 0.0)) {
                const double t = cp / (cp - cq);
                emit(px + t * (qx - px), py + t * (qy - py));
            }
        }
        n = m < KE_MAXV ? m : KE_MAXV;
    }
    if (cnt > 0) s = s + (lx * fy - fx * ly);
    double inter = 0.5 * s;
    if (!(inter > 0.0)) inter = 0.0;
    const double u = (a.area + b.area) - inter;
    iou_bev = u > 0.0 ? inter / u : 0.0;
    const double top = a.hi < b.hi ? a.hi : b.hi, bot = a.lo > b.lo ? a.lo : b.lo;
    double h = top - bot;
    if (h < 0.0) h = 0.0;
    const double vi = inter * h;
    const double u3 = (a.area * (a.hi - a.lo) + b.area * (b.hi - b.lo)) - vi;
    iou_3d = u3 > 0.0 ? vi / u3 : 0.0;
}
