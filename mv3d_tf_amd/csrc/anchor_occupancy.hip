// Empty-anchor removal of the MV3D paper (section 3.2: "we remove all the empty anchors during both training and testing ...
// by computing an integral image over the point occupancy map") for gfx950.  Not in the reference; the rule is stated in
// include/mv3d_hip.h (mv3d_anchor_occupancy) and restated in numpy by tests/empty_anchor_restatement.py.
//
//  occ_row_prefix_kernel   one workgroup per map row (y, frame): the row's Wm * C floats are read ONCE, as aligned 16-byte
//                          loads over the flat batch buffer (a row of a 601 x 601 x 9 map starts on no 16-byte boundary:
//                          the loads are aligned on the buffer, the floats of neighbouring rows they bring along are
//                          dropped), a cell's flag is raised in LDS by whichever of its channels is not +-0, the flags are
//                          scanned and the row's EXCLUSIVE prefix counts (Wm + 1 x u16) are written to the workspace.
//  occ_anchor_kernel       eight lanes per anchor: its grid_anchor() box clipped to the map, the count = the sum over its
//                          <= 40 rows of prefix[x2 + 1] - prefix[x1] (five rows per lane, three shuffles), mask = count >= min_cells.
//
// Why row prefixes and not the full integral image: the column pass of an integral image is a second dependent sweep over the
// table (or a transposition), i.e. one more launch on the serving step, to save an anchor at most 76 of its 80 two-byte reads
// of a table that sits in the L2 (0.7 MB per 601 x 601 frame against 13 MB of map): DESIGN.md section 3.18.
#include "geometry.h"

#define OCC_THREADS 256
#define OCC_MAX_W 4096
#define OCC_DEPTH 8                  // 16-byte loads a thread of the row kernel keeps in flight
#define OCC_LANES 8                  // lanes that share an anchor's rows in the anchor kernel

struct OccDev {
    const float *bev;                // (batch, Hm, Wm, C)
    int Hm, Wm, C;
    int mis;                         // floats between the 16-byte boundary below `bev` and `bev`
    long long total;                 // floats in the batch
    uint16_t *prefix;                // (batch, Hm, Wm + 1)
    int H, W, N, stride, min_cells;
    uint8_t *mask;                   // (batch, N)
    int32_t *count;                  // (batch, N) or NULL
};

__device__ __forceinline__ bool occ_nonzero(uint32_t bits) { return (bits & 0x7FFFFFFFu) != 0u; }    // !(v == 0.0f): NaN, subnormals count

__global__ __launch_bounds__(OCC_THREADS) void occ_row_prefix_kernel(OccDev d)
{
    __shared__ uint8_t s_occ[OCC_MAX_W];
    __shared__ uint16_t s_pre[OCC_MAX_W + 1];
    __shared__ int s_wave[OCC_THREADS / 64];
    const int y = blockIdx.x, f = blockIdx.y, C = d.C, Wm = d.Wm;
    for (int x = threadIdx.x; x < Wm; x += OCC_THREADS) s_occ[x] = 0;
    __syncthreads();
    // the row's floats [beg, end) of the flat buffer; "virtual" index = flat index + mis, so that virtual multiples of 4 are
    // the 16-byte boundaries
    const long long beg = ((long long)f * d.Hm + y) * (long long)Wm * C, end = beg + (long long)Wm * C;
    const long long q0 = (beg + d.mis) >> 2, q1 = (end - 1 + d.mis) >> 2;
    const uint32_t *base = reinterpret_cast<const uint32_t *>(d.bev);
    // OCC_DEPTH independent 16-byte loads per thread are issued before any is consumed: a KITTI row (5 409 floats = 1 353 groups) is one
    // round of loads for the workgroup
    for (long long qb = q0 + threadIdx.x; qb <= q1; qb += OCC_DEPTH * OCC_THREADS) {
        uint32_t v[OCC_DEPTH][4];
#pragma unroll
        for (int j = 0; j < OCC_DEPTH; ++j) {
            const long long q = qb + j * OCC_THREADS, g = 4 * q - d.mis;     // g: flat index of the group's first float
            v[j][0] = v[j][1] = v[j][2] = v[j][3] = 0u;
            if (q > q1) continue;
            if (g >= 0 && g + 3 < d.total) {
                const uint4 u = *reinterpret_cast<const uint4 *>(base + g);
                v[j][0] = u.x; v[j][1] = u.y; v[j][2] = u.z; v[j][3] = u.w;
            } else {                                                         // the first / last group of the whole buffer
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (g + k >= 0 && g + k < d.total) v[j][k] = base[g + k];
            }
        }
#pragma unroll
        for (int j = 0; j < OCC_DEPTH; ++j) {
            const long long q = qb + j * OCC_THREADS, g = 4 * q - d.mis;
            if (q > q1 || !((v[j][0] | v[j][1] | v[j][2] | v[j][3]) & 0x7FFFFFFFu)) continue;
            const long long lo = g < beg ? beg : g;                          // first float of the group that belongs to this row
            int cell = (int)((lo - beg) / C), rem = (int)((lo - beg) - (long long)cell * C);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long i = g + k;
                if (i < lo || i >= end) continue;
                if (occ_nonzero(v[j][k])) s_occ[cell] = 1;                   // (every writer of a cell stores the same value)
                if (++rem == C) { rem = 0; ++cell; }
            }
        }
    }
    __syncthreads();
    // exclusive scan of the flags: a thread sums `per` consecutive cells, the workgroup scans the 256 sums
    const int per = (Wm + OCC_THREADS - 1) / OCC_THREADS;
    const int x0 = threadIdx.x * per, x1 = min(Wm, x0 + per);
    int sum = 0;
    for (int x = x0; x < x1; ++x) sum += s_occ[x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int run = inc - sum;
    for (int w = 0; w < wave; ++w) run += s_wave[w];
    for (int x = x0; x < x1; ++x) { s_pre[x] = (uint16_t)run; run += s_occ[x]; }
    if (x1 == Wm && x0 < Wm) s_pre[Wm] = (uint16_t)run;          // (the thread that owns the last cell)
    __syncthreads();
    uint16_t *row = d.prefix + ((long long)f * d.Hm + y) * (Wm + 1);
    for (int x = threadIdx.x; x <= Wm; x += OCC_THREADS) row[x] = s_pre[x];
}

__global__ __launch_bounds__(OCC_THREADS) void occ_anchor_kernel(OccDev d)
{
    // OCC_LANES consecutive lanes per anchor: lane s takes rows y1 + s, y1 + s + 8, ... (an anchor is at most 40 rows high: five
    // independent pairs of loads per lane instead of a chain of 40), the partial counts meet in three shuffles
    const int f = blockIdx.y;
    const int t = blockIdx.x * OCC_THREADS + threadIdx.x;
    const int n = t / OCC_LANES, sub = t % OCC_LANES;
    int cnt = 0;
    if (n < d.N) {
        int x1, y1, x2, y2;
        grid_anchor(n, d.W, d.stride, x1, y1, x2, y2);
        x1 = max(x1, 0); y1 = max(y1, 0); x2 = min(x2, d.Wm - 1); y2 = min(y2, d.Hm - 1);
        if (x1 <= x2) {
            const uint16_t *rows = d.prefix + (long long)f * d.Hm * (d.Wm + 1);
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int y = y1 + sub + OCC_LANES * k;
                if (y <= y2) { const uint16_t *row = rows + (long long)y * (d.Wm + 1); cnt += (int)row[x2 + 1] - (int)row[x1]; }
            }
            for (int y = y1 + sub + OCC_LANES * 5; y <= y2; y += OCC_LANES) {   // (no anchor of the grid is that high)
                const uint16_t *row = rows + (long long)y * (d.Wm + 1);
                cnt += (int)row[x2 + 1] - (int)row[x1];
            }
        }
    }
#pragma unroll
    for (int o = 1; o < OCC_LANES; o <<= 1) cnt += __shfl_xor(cnt, o);
    if (n < d.N && sub == 0) {
        const long long o = (long long)f * d.N + n;
        d.mask[o] = cnt >= d.min_cells ? 1 : 0;
        if (d.count) d.count[o] = cnt;
    }
}

extern "C" size_t mv3d_anchor_occupancy_workspace_bytes(int batch, int map_h, int map_w)
{
    if (batch < 1 || batch > 65535 || map_h < 1 || map_h > OCC_MAX_W || map_w < 1 || map_w > OCC_MAX_W) return 0;
    return mv3d_align_up((size_t)batch * map_h * (map_w + 1) * sizeof(uint16_t));
}

extern "C" int mv3d_anchor_occupancy(const float *bev_dev, int batch, int map_h, int map_w, int channels, int H, int W,
                                     int feat_stride, int min_cells, uint8_t *mask_dev, int32_t *count_dev, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    if (!bev_dev || !mask_dev || !workspace || batch < 1 || batch > 65535 || map_h < 1 || map_h > OCC_MAX_W || map_w < 1 ||
        map_w > OCC_MAX_W || channels < 1 || channels > 64 || feat_stride < 1 || min_cells < 1 || H < 1 || W < 1 ||
        (long long)H * W * 4 > 65536 || ((uintptr_t)bev_dev % sizeof(float)))
        return MV3D_ERR_INVALID_ARG;
    // grid_anchor() works in int: the far corner of the last cell's anchors must fit
    if ((long long)((H > W ? H : W) - 1) * feat_stride + 20 > 0x7FFFFFFFll) return MV3D_ERR_INVALID_ARG;
    if (workspace_bytes < mv3d_anchor_occupancy_workspace_bytes(batch, map_h, map_w) || ((uintptr_t)workspace % MV3D_ALIGN))
        return MV3D_ERR_WORKSPACE;
    OccDev d;
    d.bev = bev_dev; d.Hm = map_h; d.Wm = map_w; d.C = channels;
    d.mis = (int)(((uintptr_t)bev_dev % 16) / sizeof(float));
    d.total = (long long)batch * map_h * map_w * channels;
    d.prefix = (uint16_t *)workspace;
    d.H = H; d.W = W; d.N = H * W * 4; d.stride = feat_stride; d.min_cells = min_cells;
    d.mask = mask_dev; d.count = count_dev;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(occ_row_prefix_kernel, dim3(map_h, batch), dim3(OCC_THREADS), 0, s, d);
    hipLaunchKernelGGL(occ_anchor_kernel, dim3((d.N * OCC_LANES + OCC_THREADS - 1) / OCC_THREADS, batch), dim3(OCC_THREADS), 0, s, d);
    return mv3d_launch_status();
}
