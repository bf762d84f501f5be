// The merge-rank bodies of the score sort (rank.hip has the kernels, the counting path and the launcher; train_stream.hip runs
// rank_local_body / rank_merge_body side by side with anchor_target.h's at_label_body / at_compact_body in one grid -- see
// anchor_target.h why the bodies are __device__ functions of a header).
#pragma once
#include "kernels.h"

typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));

// cnt += (kj > ki) resp. (kj >= ki) for 16 wave-uniform keys kj held in SGPRs: exactly two VALU
// instructions per pair (compare into VCC, add-with-carry); hipcc's own lowering of the C form
// mixes in v_cndmask/v_add sequences.  No manual wait states are needed between a VALU write of
// VCC and a VALU carry-in read (CDNA3/4 ISA, "manually inserted wait states").
// 4 compares into 4 different SGPR pairs, then 4 add-with-carry into two accumulators: the
// VALU -> SGPR -> VALU carry path is ~8 cycles deep, so a single VCC chain (cmp, addc, cmp, addc ...)
// runs at a third of the issue rate when a SIMD holds only one or two waves.
#define RANK_C(OP, M, I) "v_cmp_" OP "_u32 %[" #M "], %" #I ", %[ki]\n\t"
#define RANK_A(ACC, M) "v_addc_co_u32 %[" #ACC "], %[" #M "], 0, %[" #ACC "], %[" #M "]\n\t"
#define RANK_G(OP, I0, I1, I2, I3)                                                         \
    RANK_C(OP, m0, I0) RANK_C(OP, m1, I1) RANK_C(OP, m2, I2) RANK_C(OP, m3, I3)            \
    RANK_A(a, m0) RANK_A(b, m1) RANK_A(a, m2) RANK_A(b, m3)
#define RANK_16(OP)                                                                                        \
    asm(RANK_G(OP, 7, 8, 9, 10) RANK_G(OP, 11, 12, 13, 14) RANK_G(OP, 15, 16, 17, 18) RANK_G(OP, 19, 20, 21, 22) \
        : [a] "+v"(cnt), [b] "+v"(cnt2), [m0] "=&s"(m0), [m1] "=&s"(m1), [m2] "=&s"(m2), [m3] "=&s"(m3)     \
        : [ki] "v"(ki), "s"(v.s0), "s"(v.s1), "s"(v.s2), "s"(v.s3), "s"(v.s4), "s"(v.s5), "s"(v.s6), "s"(v.s7), \
          "s"(v.s8), "s"(v.s9), "s"(v.sa), "s"(v.sb), "s"(v.sc), "s"(v.sd), "s"(v.se), "s"(v.sf))
template <bool GE>
__device__ __forceinline__ void count16(unsigned &cnt, unsigned &cnt2, const uint32_t ki, const u32x16 v)
{
    unsigned long long m0, m1, m2, m3;
    if (GE) RANK_16("ge");
    else RANK_16("gt");
}

#define RANK_SEG 1024

// ---------------------------------------------------------------------------- A. merge-rank
#define RANK_LDS_KEYS 24576
#define RANK_RUN 1024            // sorted run length (= RANK_SEG: one scalar-load segment)

// grid (key_stride/128, batch).  Workgroup bi owns 128 keys of run R = bi/8 and ranks them inside
// the run by counting over its 1024 keys (wave-uniform, scalar loads; `>` / `>=` per 256-key
// sub-tile as in rank_partial_kernel).  Candidates are written to their run position:
// sorted[f][R*1024 + r] = key, sidx = index inside the run.  Non-candidates (key 0) are not
// written at all; cnt128[f][run] = candidates of the run (counted by the run's first workgroup) lets the
// consumer treat the tail of every run as zeros.  (128 keys per workgroup: 184 workgroups for a KITTI frame, so the counting --
// the kernel is VALU-bound -- spreads over most of the 256 CUs.)
#define RANK_LK 128                                 // keys per workgroup
#define RANK_SUBW 128                               // keys per sub-tile
#define RANK_NSUB (RANK_RUN / RANK_SUBW)            // sub-tiles = thread groups of the workgroup (8)
// (body: workgroup bi of frame f, nwg workgroups per frame; one barrier -- a larger workgroup's other waves must have returned)
__device__ __forceinline__ void rank_local_body(const uint32_t *__restrict__ keys, int key_stride, uint32_t *__restrict__ sorted,
                                                uint16_t *__restrict__ sidx, int32_t *__restrict__ cnt128, const int f, const int bi,
                                                const int nwg)
{
    // 1024 threads = 128 keys x 8 sub-tiles of the run: thread (t, sub) counts its key against the 128 keys of
    // sub-tile `sub` (the kernel is VALU-bound: 16 waves of 260 instructions finish sooner than 8 of 520).
    __shared__ unsigned s_part[RANK_NSUB][RANK_LK];
    __shared__ int s_wc[RANK_NSUB * RANK_LK / 64];
    const int t = threadIdx.x & (RANK_LK - 1), sub = __builtin_amdgcn_readfirstlane(threadIdx.x / RANK_LK);
    const int run = bi >> 3, kb = bi & 7;
    const int i = kb * RANK_LK + t;                 // key index inside the run
    const int my_sub = i / RANK_SUBW;               // its sub-tile (workgroup-uniform)
    const uint32_t *__restrict__ k = keys + (long long)f * key_stride + run * RANK_RUN;
    const uint32_t ki = k[i];
    const uint32_t kim1 = ki - 1u;                  // kj >= ki  <=>  kj > ki - 1   (ki >= 1 for candidates)
    unsigned cnt = 0, cnt2 = 0;
    const u32x16 *__restrict__ q = reinterpret_cast<const u32x16 *>(k + sub * RANK_SUBW);
    if (sub < my_sub) {                             // all j < i : only a strictly larger key precedes
#pragma unroll 4
        for (int u = 0; u < RANK_SUBW / 16; ++u) count16<false>(cnt, cnt2, ki, q[u]);
    } else if (sub > my_sub) {                      // all j > i : an equal key precedes too
#pragma unroll 4
        for (int u = 0; u < RANK_SUBW / 16; ++u) count16<true>(cnt, cnt2, ki, q[u]);
    } else {
        // own sub-tile: per 64-key part the rule is again uniform for a whole wave, except for the wave's own
        // part, where the later index wins a tie lane by lane
        const int il = i & (RANK_SUBW - 1);         // index inside the sub-tile
        const int wq = __builtin_amdgcn_readfirstlane(il >> 6);
        for (int qq = 0; qq < RANK_SUBW / 64; ++qq) {
            if (qq < wq) {
#pragma unroll
                for (int u = 0; u < 4; ++u) count16<false>(cnt, cnt2, ki, q[qq * 4 + u]);
            } else if (qq > wq) {
#pragma unroll
                for (int u = 0; u < 4; ++u) count16<true>(cnt, cnt2, ki, q[qq * 4 + u]);
            } else {
#pragma unroll 16
                for (int j = qq * 64; j < qq * 64 + 64; ++j) {
                    const uint32_t kj = k[sub * RANK_SUBW + j];  // wave-uniform: scalar load
                    const uint32_t thr = (j > il) ? kim1 : ki;   // kj >= ki  <=>  kj > ki - 1
                    cnt += (kj > thr) ? 1u : 0u;
                }
            }
        }
    }
    s_part[sub][t] = cnt + cnt2;
    if (kb == 0) {                                  // candidates of the whole run: one key per thread
        const int c = __popcll(__ballot(k[threadIdx.x] != 0u));
        if ((threadIdx.x & 63) == 0) s_wc[threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (sub == 0) {
        if (kb == 0 && t == 0) {
            int c = 0;
#pragma unroll
            for (int w = 0; w < RANK_NSUB * RANK_LK / 64; ++w) c += s_wc[w];
            cnt128[(long long)f * (nwg >> 3) + run] = c;
        }
        if (ki != 0u) {
            unsigned r = 0;
#pragma unroll
            for (int s2 = 0; s2 < RANK_NSUB; ++s2) r += s_part[s2][t];
            const long long o = (long long)f * key_stride + run * RANK_RUN + r;
            sorted[o] = ki;
            sidx[o] = (uint16_t)i;
        }
    }
}

template <bool GE>
__device__ __forceinline__ int count_before(const uint32_t *sb, const uint32_t ki)
{
    // sb: RANK_RUN keys in descending order; number of keys kj with kj > ki (GE: kj >= ki)
    int pos = 0;
#pragma unroll
    for (int step = RANK_RUN / 2; step >= 1; step >>= 1) {
        const uint32_t v = sb[pos + step - 1];
        if (GE ? (v >= ki) : (v > ki)) pos += step;
    }
    const uint32_t v = sb[pos];                     // pos <= RANK_RUN - 1
    if (GE ? (v >= ki) : (v > ki)) pos += 1;
    return pos;
}

// grid (key_stride/128, batch), 256 threads: the thread pair (t & 127, half t >> 7) of workgroup bi owns
// position (bi&7)*128 + (t&127) of run bi/8 -- half h searches the runs of parity h -- so that the LDS
// traffic of the searches spreads over twice as many CUs.  All runs of the frame are staged in LDS (<= 96 KB).
// (body: workgroup bi of frame f; 256 threads, two barriers)
__device__ __forceinline__ void rank_merge_body(const uint32_t *__restrict__ sorted, const uint16_t *__restrict__ sidx,
                                                const int32_t *__restrict__ cnt128, int N, int key_stride, int32_t *order, int cap,
                                                const int32_t *part_counts, int n_parts, int32_t *n_valid,
                                                const float4 *__restrict__ gsrc, float4 *gdst, const int f, const int bi)
{
    __shared__ uint32_t s_keys[RANK_LDS_KEYS];
    __shared__ int s_half[128];
    const int t = threadIdx.x;
    const int nrun = key_stride / RANK_RUN;
    const int R = bi >> 3, pos = (bi & 7) * 128 + (t & 127), h = __builtin_amdgcn_readfirstlane(t >> 7);
    // the scatter index of the own key is requested first: its latency hides under everything else
    const int own = (int)sidx[(long long)f * key_stride + R * RANK_RUN + pos];
    // ... and, when the caller wants its records in rank order too, the record of the own key (a slot past the
    // run's candidates holds a stale index: the address is clamped and the value unused)
    float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gsrc && h == 0) rec = gsrc[(long long)f * N + min(R * RANK_RUN + own, N - 1)];
    const uint4 *__restrict__ src4 = reinterpret_cast<const uint4 *>(sorted + (long long)f * key_stride);
    const int32_t *__restrict__ crun = cnt128 + (long long)f * nrun;
    // staging: thread t owns keys 4t..4t+3 of every run; all loads are issued before the first use
    constexpr int MAXRUN = RANK_LDS_KEYS / RANK_RUN;
    uint4 v[MAXRUN];
#pragma unroll
    for (int r = 0; r < MAXRUN; ++r) v[r] = src4[t + 256 * min(r, nrun - 1)];
#pragma unroll
    for (int r = 0; r < MAXRUN; ++r) {
        if (r < nrun) {
            const int nc = crun[r] - 4 * t;          // candidates of the run (wave-uniform load)
            uint4 w = v[r];
            if (nc <= 0) w.x = 0u;                   // slots past the run's candidates were never written
            if (nc <= 1) w.y = 0u;
            if (nc <= 2) w.z = 0u;
            if (nc <= 3) w.w = 0u;
            reinterpret_cast<uint4 *>(s_keys)[t + 256 * r] = w;
        }
    }
    __syncthreads();
    const uint32_t ki = s_keys[R * RANK_RUN + pos];
    // count_r = #{keys of run r that precede ki}: runs of smaller index `>`; runs of larger index `>=`,
    // i.e. `> ki - 1` (ki >= 1); the own run and the runs that do not exist get a threshold nothing
    // exceeds.  The binary searches of all runs advance in lock-step, so every step is one batch of
    // independent LDS reads instead of a chain of dependent ones.
    constexpr int HR = MAXRUN / 2;
    int part = 0;
    if (ki != 0u) {
        uint32_t thr[HR];
        int cnt[HR];
#pragma unroll
        for (int i = 0; i < HR; ++i) {
            const int r = 2 * i + h;
            thr[i] = (r == R || r >= nrun) ? 0xffffffffu : (r > R ? ki - 1u : ki);
            cnt[i] = 0;
        }
        const uint32_t *base = s_keys + h * RANK_RUN;
#pragma unroll
        for (int step = RANK_RUN / 2; step >= 1; step >>= 1) {
            uint32_t q[HR];
#pragma unroll
            for (int i = 0; i < HR; ++i) q[i] = base[2 * i * RANK_RUN + cnt[i] + step - 1];
#pragma unroll
            for (int i = 0; i < HR; ++i) cnt[i] += (q[i] > thr[i]) ? step : 0;
        }
#pragma unroll
        for (int i = 0; i < HR; ++i) part += cnt[i] + ((base[2 * i * RANK_RUN + cnt[i]] > thr[i]) ? 1 : 0);
    }
    if (h == 1) s_half[t & 127] = part;
    __syncthreads();
    if (h == 0 && ki != 0u) {
        const int rank = pos + part + s_half[t];    // pos = position inside the own sorted run
        if (rank < cap) {
            order[(long long)f * cap + rank] = R * RANK_RUN + own;
            if (gdst) gdst[(long long)f * cap + rank] = rec;
        }
    }
    if (n_valid && bi == 0 && t < 64) {
        int nv = 0;
        for (int p = t; p < n_parts; p += 64) nv += part_counts[(long long)f * n_parts + p];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nv += __shfl_down(nv, o);
        if (t == 0) n_valid[f] = nv;
    }
}

// the merge-rank launches' arguments from the arguments of mv3d_launch_rank (key_stride <= RANK_LDS_KEYS)
struct RankMergeArgs {
    const uint32_t *keys;
    uint32_t *sorted;
    uint16_t *sidx;
    int32_t *cnt128;
    int N, key_stride, cap, n_parts;
    int32_t *order, *n_valid;
    const int32_t *part_counts;
    const float4 *gsrc;
    float4 *gdst;
};
static inline RankMergeArgs rank_merge_args(const uint32_t *keys, int N, int key_stride, int batch, int32_t *order, int cap,
                                            const int32_t *part_counts, int n_parts, int32_t *n_valid, void *workspace,
                                            const float4 *gather_src, float4 *gather_dst)
{
    RankMergeArgs a;
    a.keys = keys; a.sorted = (uint32_t *)workspace;
    a.sidx = (uint16_t *)((char *)workspace + mv3d_align_up((size_t)batch * key_stride * 4));
    a.cnt128 = (int32_t *)((char *)a.sidx + mv3d_align_up((size_t)batch * key_stride * 2));
    a.N = N; a.key_stride = key_stride; a.cap = cap; a.n_parts = n_parts; a.order = order; a.n_valid = n_valid;
    a.part_counts = part_counts; a.gsrc = gather_src; a.gdst = gather_dst;
    return a;
}
__device__ __forceinline__ void rank_local_body(const RankMergeArgs &a, const int f, const int bi, const int nwg)
{
    rank_local_body(a.keys, a.key_stride, a.sorted, a.sidx, a.cnt128, f, bi, nwg);
}
__device__ __forceinline__ void rank_merge_body(const RankMergeArgs &a, const int f, const int bi)
{
    rank_merge_body(a.sorted, a.sidx, a.cnt128, a.N, a.key_stride, a.order, a.cap, a.part_counts, a.n_parts, a.n_valid, a.gsrc, a.gdst, f, bi);
}
