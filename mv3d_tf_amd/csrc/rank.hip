// Score sort of proposal_layer_3d (lib/rpn_msr/proposal_layer_tf.py:161-167:
// scores.argsort()[::-1][:pre_nms_topN]).  order[rank(i)] = i for rank(i) < cap with
//
//   rank(i) = #{ j : key_j > key_i  or (key_j == key_i and j > i) }
//
// (descending score, ties by descending index = stable ascending sort reversed; the reference
// leaves ties to numpy's unstable sort).  Two implementations, both exact and deterministic:
//
//  A. merge-rank (key_stride <= 24576 keys per frame, i.e. every KITTI-sized grid; 2 kernels)
//     rank_local_kernel   sorts runs of 1024 keys by counting inside the run (keys wave-uniform
//                         through scalar loads, 2 VALU per pair) and writes each run sorted.
//     rank_merge_kernel   each workgroup stages ALL sorted runs of its frame in LDS (<= 96 KB of
//                         the CU's 160 KB) and every thread binary-searches its key in each other
//                         run: 11 LDS reads per run instead of 1024 compares.  Because runs own
//                         disjoint index ranges, the tie-break reduces to searching with `>` in
//                         runs of smaller index and `>=` in runs of larger index.  Scatters the
//                         order and totals n_valid (no atomics, no memset).
//  B. counting (any size; fallback): rank_partial_kernel + rank_scatter_kernel, O(N^2) pairs at two
//     VALU instructions per pair.
#include "rank.h"

// The sizes that choose between A and B and shape both, as rank.h (the merge-rank bodies) compiles them: restated here, next to
// the rules of this file that use them, token for token -- any other value is a redefinition, which does not compile.
#pragma clang diagnostic error "-Wmacro-redefined"
#define RANK_SEG 1024
#define RANK_LDS_KEYS 24576
#define RANK_RUN 1024

// keys: (batch, key_stride) with key_stride a multiple of RANK_SEG and keys[N..key_stride) == 0,
// so every segment is full.  The keys of a segment are wave-uniform: they are read with scalar
// loads (s_load_dwordx16 through the scalar cache) and never touch LDS or the vector path.
__global__ __launch_bounds__(256) void rank_partial_kernel(const uint32_t *__restrict__ keys, int N, int key_stride,
                                                           int S, uint32_t *__restrict__ partial)
{
    const int f = blockIdx.z, s = blockIdx.y;
    const uint32_t *__restrict__ k = keys + (long long)f * key_stride;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ki = k[i];                       // i < key_stride always (grid covers the padding)
    const int my_sub = blockIdx.x;                  // 256-key sub-tile holding this block's own keys
    const int t0 = s * RANK_SEG;
    unsigned cnt = 0, cnt2 = 0;
    for (int q4 = 0; q4 < RANK_SEG / 256; ++q4) {
        const int sub = t0 / 256 + q4;
        const u32x16 *__restrict__ q = reinterpret_cast<const u32x16 *>(k + sub * 256);
        if (sub < my_sub) {                         // all j < i : only a strictly larger key precedes
#pragma unroll 4
            for (int u = 0; u < 16; ++u) count16<false>(cnt, cnt2, ki, q[u]);
        } else if (sub > my_sub) {                  // all j > i : an equal key precedes too
#pragma unroll 4
            for (int u = 0; u < 16; ++u) count16<true>(cnt, cnt2, ki, q[u]);
        } else {                                    // own sub-tile: full rule
            const int jb = sub * 256;
            for (int u = 0; u < 256; ++u) {
                const uint32_t kj = k[jb + u];
                cnt += (kj > ki) || (kj == ki && jb + u > i);
            }
        }
    }
    if (i < N) partial[((long long)f * S + s) * N + i] = cnt + cnt2;
}

// ---------------------------------------------------------------------------- A. merge-rank (bodies: rank.h)
__global__ __launch_bounds__(RANK_NSUB * RANK_LK) void rank_local_kernel(RankMergeArgs a) { rank_local_body(a, blockIdx.y, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(256) void rank_merge_kernel(RankMergeArgs a) { rank_merge_body(a, blockIdx.y, blockIdx.x); }

// ---------------------------------------------------------------------------- B. counting (scatter)
__global__ __launch_bounds__(256) void rank_scatter_kernel(const uint32_t *__restrict__ keys, int N, int key_stride, int S,
                                                           const uint32_t *__restrict__ partial, int32_t *order, int cap,
                                                           const int32_t *part_counts, int n_parts, int32_t *n_valid,
                                                           const float4 *__restrict__ gsrc, float4 *gdst)
{
    const int f = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        const uint32_t ki = keys[(long long)f * key_stride + i];
        if (ki != 0u) {
            unsigned cnt = 0;
            for (int s = 0; s < S; ++s) cnt += partial[((long long)f * S + s) * N + i];
            if ((int)cnt < cap) {
                order[(long long)f * cap + cnt] = i;
                if (gdst) gdst[(long long)f * cap + cnt] = gsrc[(long long)f * N + i];
            }
        }
    }
    if (n_valid && blockIdx.x == 0 && threadIdx.x < 64) {
        int v = 0;
        for (int p = threadIdx.x; p < n_parts; p += 64) v += part_counts[(long long)f * n_parts + p];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if (threadIdx.x == 0) n_valid[f] = v;
    }
}

int mv3d_rank_key_stride(int N) { return (N + RANK_SEG - 1) / RANK_SEG * RANK_SEG; }

size_t mv3d_rank_ws_bytes(int N, int batch)
{
    const size_t ks = (size_t)mv3d_rank_key_stride(N);
    if (ks <= RANK_LDS_KEYS)
        return mv3d_align_up((size_t)batch * ks * 4) + mv3d_align_up((size_t)batch * ks * 2) + mv3d_align_up((size_t)batch * (ks / 128) * 4);
    const size_t S = ks / RANK_SEG;
    return mv3d_align_up((size_t)batch * S * N * 4);
}

int mv3d_launch_rank(const uint32_t *keys, int N, int key_stride, int batch, int32_t *order, int cap,
                     const int32_t *part_counts, int n_parts, int32_t *n_valid, void *workspace, hipStream_t stream,
                     const float4 *gather_src, float4 *gather_dst)
{
    if (N <= 0 || batch <= 0 || cap <= 0 || !workspace || key_stride != mv3d_rank_key_stride(N)) return MV3D_ERR_INVALID_ARG;
    if (key_stride <= RANK_LDS_KEYS) {
        const RankMergeArgs a = rank_merge_args(keys, N, key_stride, batch, order, cap, part_counts, n_parts, n_valid, workspace, gather_src,
                                                gather_dst);
        hipLaunchKernelGGL(rank_local_kernel, dim3(key_stride / 128, batch), dim3(RANK_NSUB * RANK_LK), 0, stream, a);
        hipLaunchKernelGGL(rank_merge_kernel, dim3(key_stride / 128, batch), dim3(256), 0, stream, a);
        return mv3d_launch_status();
    }
    const int S = key_stride / RANK_SEG, IB = (N + 255) / 256;
    uint32_t *partial = (uint32_t *)workspace;
    hipLaunchKernelGGL(rank_partial_kernel, dim3(IB, S, batch), dim3(256), 0, stream, keys, N, key_stride, S, partial);
    hipLaunchKernelGGL(rank_scatter_kernel, dim3(IB, batch), dim3(256), 0, stream, keys, N, key_stride, S, partial, order,
                       cap, part_counts, n_parts, n_valid, gather_src, gather_dst);
    return mv3d_launch_status();
}
