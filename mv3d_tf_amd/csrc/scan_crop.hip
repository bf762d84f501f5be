// Crop to the camera image: the MV3D paper's §3.4 "we also remove points that are out of the image boundaries when
// projected to the image plane", as a stable compaction of `num_frames` Velodyne clouds laid back to back.  A (points, offsets) batch
// goes in, a (points, offsets) batch of the kept rows comes out, frames back to back in their order and rows in theirs, which the
// rasterisers (bev_raster.hip, bev_paper.hip, front_view_raster.hip) take as they take any other.  PARITY UNPINNED: the reference has
// no such code; tests/scan_crop_restatement.py states the rule.
//   keep     a row [x, y, z, r] of frame b is kept iff x, y, z are finite and, with M = proj_matrix of the frame's table (geometry.h)
//            and v = M . [x, y, z, 1] in f64 (scan_image_point: image_point's accumulation order with homogeneous w = 1),
//            v[2] > 0 and 0 <= v[0] / v[2] < width and 0 <= v[1] / v[2] < height of the frame's image.  No margin, no minimum depth;
//            the reflectance is never looked at.  A row that no frame owns (frame_rows.h) is dropped.
//   launches three, whatever the batch, ordered by the stream alone -- no workgroup waits for another one of its launch:
//            flags    a workgroup of 256 owns a TILE of SCAN_CROP_TILE consecutive rows, 4 per thread; every wave stores the 64-bit
//                     ballot of its 64 rows' predicate as one word, the workgroup stores the tile's kept count
//            scan     ONE workgroup: exclusive scan of the tile counts in place (1024 tiles per round), then offsets_out
//            copy     rank of a kept row = tile base + popcount of the tile's words in front + popcount of the lanes in front;
//                     the row is copied as one 16-byte vector
//   offsets  frame_of_row(p) never decreases with p, whatever the offsets hold (every step of its binary search is the test
//            offsets[mid] <= p, which only turns from false to true as p grows), so the kept rows of frame b follow those of the frames
//            < b in the output, and offsets_out[b] = rank of t_b, the first row whose search ends at a frame >= b (t_0 = 0, t_nf = P):
//            Under ascending offsets t_b is offsets[b] clamped to [0, P], which two searches confirm (the row in front ends below b,
//            the row itself at b or above); under any other offsets t_b is found by bisection over p.
//   bounds   flags reads rows p < P of points_dev only, and the tables of frames in [0, nf): the frame comes from frame_of_row,
//            which answers "none" or a frame in [0, nf) whatever offsets_dev holds; calib and image_hw values enter arithmetic only,
//            never an address.  It writes words w < ceil(P / 64) and one count per tile.  scan reads and writes those counts and
//            reads words below ceil(P / 64) (a boundary row is clamped to [0, P]).  copy reads the words and bases of its own tile:
//            a bit is set only for a row p < P that flags of the SAME call kept, the counts are the popcounts of those words, so a
//            rank is below the number of kept rows <= P; both p < P and rank < P are tested again where the row is copied.  So
//            nothing in offsets_dev, calib_dev or image_hw_dev can make the call read or write out of bounds.
// HBM-bound by construction: 16 P bytes read by flags, at most 16 P by copy (a row whose bit is clear is not loaded), 16 K written.
#include "common.h"
#include "frame_rows.h"
#include "geometry.h"

#define SCAN_CROP_TILE 1024          // rows a workgroup owns: 4 waves x 4 words of 64 rows
#define SCAN_CROP_WORDS 16           // ballot words per tile
#define SCAN_CROP_STAGED 8           // frames whose matrix a workgroup stages in LDS: the frame of its first row and the 7 behind it

__device__ __forceinline__ bool scan_crop_keep(const float4 v, const float *M, int height, int width)
{
    const unsigned inf = 0x7f800000u;
    if ((__float_as_uint(v.x) & inf) == inf || (__float_as_uint(v.y) & inf) == inf || (__float_as_uint(v.z) & inf) == inf) return false;
    double q[3];
    scan_image_point(M, v.x, v.y, v.z, q);
    if (!(q[2] > 0.0) || height <= 0 || width <= 0) return false;
    const double u = q[0] / q[2], w = q[1] / q[2];
    return u >= 0.0 && u < (double)width && w >= 0.0 && w < (double)height;
}

__global__ __launch_bounds__(256) void scan_crop_flags_kernel(const float *__restrict__ pts, const int *__restrict__ offsets, int nf, int P,
                                                              const float *__restrict__ calib, const int *__restrict__ image_hw,
                                                              unsigned long long *__restrict__ words, int *__restrict__ counts)
{
    __shared__ int s_off[MV3D_FV_MAX_FRAMES + 1];
    __shared__ float s_M[SCAN_CROP_STAGED][12];
    __shared__ int s_hw[SCAN_CROP_STAGED][2];
    __shared__ int s_cnt[4];
    frame_rows_stage(s_off, offsets, nf, P);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned first = blockIdx.x * (unsigned)SCAN_CROP_TILE;
    int f0;
    frame_of_row(s_off, nf, first, f0);                                  // (a frame in [0, nf) whether or not it owns the row)
    if (threadIdx.x < SCAN_CROP_STAGED && f0 + (int)threadIdx.x < nf) {
        const int f = f0 + threadIdx.x;
        proj_matrix(calib + 48 * f, s_M[threadIdx.x]);
        s_hw[threadIdx.x][0] = image_hw[2 * f];
        s_hw[threadIdx.x][1] = image_hw[2 * f + 1];
    }
    __syncthreads();
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned p = first + wave * 256u + u * 64u + lane;
        bool keep = false;
        int f;
        if (p < (unsigned)P && frame_of_row(s_off, nf, p, f)) {
            const float4 v = reinterpret_cast<const float4 *>(pts)[p];
            const unsigned j = (unsigned)(f - f0);
            if (j < SCAN_CROP_STAGED) {
                keep = scan_crop_keep(v, s_M[j], s_hw[j][0], s_hw[j][1]);
            } else {                                                     // more than 8 frames in one tile: the matrix from the table
                float M[12];
                proj_matrix(calib + 48 * f, M);
                keep = scan_crop_keep(v, M, image_hw[2 * f], image_hw[2 * f + 1]);
            }
        }
        const unsigned long long word = __ballot(keep);
        if (lane == 0 && first + wave * 256u + u * 64u < (unsigned)P) words[(size_t)blockIdx.x * SCAN_CROP_WORDS + wave * 4 + u] = word;
        cnt += __popcll(word);
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// kept rows in front of row r of [0, P]: bases = the scanned tile counts, total = their sum
__device__ __forceinline__ int scan_crop_rank(const unsigned long long *__restrict__ words, const int *bases, int total, int P, int r)
{
    if (r >= P) return total;
    const int tile = r / SCAN_CROP_TILE, word = r >> 6;
    int rank = bases[tile];
    for (int w = tile * SCAN_CROP_WORDS; w < word; ++w) rank += __popcll(words[w]);
    return rank + __popcll(words[word] & ((1ull << (r & 63)) - 1ull));
}

// ONE workgroup.  counts[0 .. ntiles) -> their exclusive scan, in place; offsets_out[0 .. nf].
__global__ __launch_bounds__(256) void scan_crop_scan_kernel(const int *__restrict__ offsets, int nf, int P,
                                                             const unsigned long long *__restrict__ words, int *counts, int ntiles,
                                                             int *__restrict__ offsets_out)
{
    __shared__ int s_off[MV3D_FV_MAX_FRAMES + 1];
    __shared__ int s_wave[4];
    __shared__ int s_carry;
    frame_rows_stage(s_off, offsets, nf, P);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < ntiles; base += 1024) {                    // (ntiles <= 2^21: base + 1023 + 3 stays an int)
        const int i0 = base + 4 * (int)threadIdx.x;
        int c[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { c[k] = i0 + k < ntiles ? counts[i0 + k] : 0; sum += c[k]; }
        int incl = sum;                                                  // inclusive scan of the threads' sums over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int excl = s_carry + incl - sum;
        for (int w = 0; w < wave; ++w) excl += s_wave[w];
#pragma unroll
        for (int k = 0; k < 4; ++k) { if (i0 + k < ntiles) counts[i0 + k] = excl; excl += c[k]; }
        __syncthreads();                                                 // every thread has read s_carry and s_wave
        if (threadIdx.x == 0) s_carry += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();                                                 // (and the bases written so far are visible to the workgroup)
    }
    const int total = s_carry;
    auto frame_at = [&](int p) { int f; frame_of_row(s_off, nf, (unsigned)p, f); return f; };      // (where the search ends, owner or not)
    for (int b = threadIdx.x; b <= nf; b += 256) {
        int lo = 0, hi = P;                                              // t_b: the first row of [0, P] whose search ends at a frame >= b
        const int c = min(max(s_off[b], 0), P);                          // under ascending offsets that is offsets[b]: two searches say so
        if ((c == P || frame_at(c) >= b) && (c == 0 || frame_at(c - 1) < b)) lo = hi = c;
        while (lo < hi) {                                                // (any other offsets: bisection over the rows)
            const int mid = lo + ((hi - lo) >> 1);
            if (frame_at(mid) >= b) hi = mid; else lo = mid + 1;
        }
        offsets_out[b] = b == 0 ? 0 : scan_crop_rank(words, counts, total, P, lo);
    }
}

__global__ __launch_bounds__(256) void scan_crop_copy_kernel(const float *__restrict__ pts, int P, const unsigned long long *__restrict__ words,
                                                             const int *__restrict__ bases, float *__restrict__ out)
{
    __shared__ unsigned long long s_word[SCAN_CROP_WORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned first = blockIdx.x * (unsigned)SCAN_CROP_TILE;
    if (threadIdx.x < SCAN_CROP_WORDS)
        s_word[threadIdx.x] = first + threadIdx.x * 64u < (unsigned)P ? words[(size_t)blockIdx.x * SCAN_CROP_WORDS + threadIdx.x] : 0ull;
    __syncthreads();
    int rank = bases[blockIdx.x];
    for (int w = 0; w < wave * 4; ++w) rank += __popcll(s_word[w]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned long long word = s_word[wave * 4 + u];
        const unsigned p = first + wave * 256u + u * 64u + lane;
        const unsigned at = (unsigned)rank + __popcll(word & ((1ull << lane) - 1ull));
        if (((word >> lane) & 1ull) && p < (unsigned)P && at < (unsigned)P)
            reinterpret_cast<float4 *>(out)[at] = reinterpret_cast<const float4 *>(pts)[p];
        rank += __popcll(word);
    }
}

static inline long long scan_crop_tiles(int total_points) { return ((long long)total_points + SCAN_CROP_TILE - 1) / SCAN_CROP_TILE; }
// the workspace: ceil(P / 64) ballot words, then one int32 per tile (count, then base), each part rounded up to MV3D_ALIGN
static inline size_t scan_crop_words_bytes(int total_points) { return mv3d_align_up((((size_t)total_points + 63) / 64) * 8); }

extern "C" size_t mv3d_scan_crop_workspace(int total_points)
{
    if (total_points <= 0) return 0;
    return scan_crop_words_bytes(total_points) + mv3d_align_up((size_t)scan_crop_tiles(total_points) * 4);
}

extern "C" int mv3d_scan_crop_tile_rows(void) { return SCAN_CROP_TILE; }

extern "C" int mv3d_scan_crop_to_image(const float *points_dev, const int32_t *offsets_dev, int num_frames, int total_points,
                                       const float *calib_dev, const int32_t *image_hw_dev, float *points_out_dev, int32_t *offsets_out_dev,
                                       void *workspace_dev, size_t workspace_bytes, void *stream)
{
    if (num_frames < 0 || num_frames > MV3D_FV_MAX_FRAMES || total_points < 0) return MV3D_ERR_INVALID_ARG;
    if (num_frames == 0) return MV3D_OK;
    if ((!offsets_dev && num_frames != 1) || !calib_dev || !image_hw_dev || !offsets_out_dev) return MV3D_ERR_INVALID_ARG;
    if (total_points > 0 && (!points_dev || !points_out_dev || !workspace_dev)) return MV3D_ERR_INVALID_ARG;
    if (((uintptr_t)points_dev & 15) != 0 || ((uintptr_t)points_out_dev & 15) != 0 || ((uintptr_t)workspace_dev & 15) != 0 ||
        ((uintptr_t)offsets_dev & 3) != 0 || ((uintptr_t)calib_dev & 3) != 0 || ((uintptr_t)image_hw_dev & 3) != 0 ||
        ((uintptr_t)offsets_out_dev & 3) != 0)
        return MV3D_ERR_INVALID_ARG;
    if (workspace_bytes < mv3d_scan_crop_workspace(total_points)) return MV3D_ERR_INVALID_ARG;
    const uintptr_t in = (uintptr_t)points_dev, out = (uintptr_t)points_out_dev, bytes = (uintptr_t)total_points * 16;
    if (in < out + bytes && out < in + bytes) return MV3D_ERR_INVALID_ARG;                 // (no bytes, no overlap)
    hipStream_t s = (hipStream_t)stream;
    const int ntiles = (int)scan_crop_tiles(total_points);
    unsigned long long *words = reinterpret_cast<unsigned long long *>(workspace_dev);
    int *counts = reinterpret_cast<int *>(reinterpret_cast<char *>(workspace_dev) + scan_crop_words_bytes(total_points));
    if (ntiles > 0)
        hipLaunchKernelGGL(scan_crop_flags_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, points_dev, offsets_dev, num_frames, total_points,
                           calib_dev, image_hw_dev, words, counts);
    hipLaunchKernelGGL(scan_crop_scan_kernel, dim3(1), dim3(256), 0, s, offsets_dev, num_frames, total_points, words, counts, ntiles,
                       offsets_out_dev);
    if (ntiles > 0)
        hipLaunchKernelGGL(scan_crop_copy_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, points_dev, total_points, words, counts,
                           points_out_dev);
    return mv3d_launch_status();
}
