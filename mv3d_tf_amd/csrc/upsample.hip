// Bilinear 2x / 4x upsampling of the feature maps in front of RoiPool (MV3D paper §3.2), forward and backward, for up
// to MV3D_MAX_ROI_VIEWS views in ONE launch each (the views' workgroups share the grid, as in mv3d_maxpool2x2_views_*).
// The coordinate rule is TensorFlow 1's resize_bilinear(align_corners=False): up-pixel o sits at source coordinate o / s, so up-pixel
// s*i IS source pixel i and RoiPool's scale after the upsampling is s / 8 with no half-pixel shift.  Per axis up-index o has the taps
//     i0 = o / s                 weight (s - o % s) / s
//     i1 = min(i0 + 1, n - 1)    weight (o % s) / s
// a tap of weight 0 is dropped (its value never enters the arithmetic: a NaN neighbour does not reach an aligned up-pixel) and two taps
// on the same source index (the clamped last rows / columns) merge into one tap of weight 1: every up-index has ONE tap of weight 1 or
// TWO taps with dyadic weights.
//   forward    f32, every operation rounded on its own: horizontally on each source row t = a (one tap) or fadd(fmul(w0, a), fmul(w1, b)),
//              then the same rule vertically on the one or two t.  16-bit inputs are converted to f32 first (exact); the output is f32.
//   backward   the exact transpose: g_x[iy][ix] = sum of fmul(wy * wx, g_y[oy][ox]) over the up-pixels with a tap on (iy, ix), added to
//              0.0f in raster order (oy ascending, then ox ascending); wy * wx is exact.  At most (2s - 1)^2 terms.
// Forward: a thread owns one 16-byte vector of the channel axis of one SOURCE pixel (4 f32 / 8 16-bit elements in) and writes the s x s
// up-pixels whose first tap is that pixel: the 2 x 2 source taps are loaded once for s^2 outputs and stay in registers; consecutive
// lanes walk the channel axis, so every load and store instruction moves 16 B x 64 lanes of consecutive addresses.  The kernel is bound
// by its stores (s^2 output bytes per input byte; the neighbours' re-reads of a source pixel hit L2).
// Backward: a thread owns one vector of g_x and walks its (2s - 1)^2 terms in registers -- no atomics, no workspace, the same bits on
// every run.  Neighbouring outputs share most of their reads; they meet in L2 (no LDS staging): the workgroups are dealt out so that
// every XCD owns a contiguous eighth of a view, see the kernel.
// A view runs with vectors when its channel count is a multiple of the vector width and its pointers and strides are 16-byte aligned;
// otherwise the WHOLE view runs the scalar instantiation of the same body (no vector body with a scalar tail, the rule of
// fusion_join.hip).  Offsets are 64-bit; 256 threads, a view's workgroups are capped and stride over its items beyond the cap.
#include "common.h"

#define UP_BLOCK 256
#define UP_MAX_VIEW_BLOCKS (1 << 20)

struct UpView {
    const void *in;
    float *out;
    long long fs, rs, ps;          // input strides in elements: frame, row, pixel (forward only)
    long long items;               // batch * height * width * (channels / vector)
    int H, W, C, s;
    int kind;                      // 0 = f32, 1 = f16, 2 = bf16
    int vec;                       // 1: the vector body
    unsigned blocks;               // workgroups of this view
};
struct UpGroup { UpView v[MV3D_MAX_ROI_VIEWS]; unsigned first[MV3D_MAX_ROI_VIEWS + 1]; int n; };

template <int KIND> struct UpType;
template <> struct UpType<0> {
    typedef float word; enum { VEC = 4 };
    static __device__ __forceinline__ float load(word w) { return w; }
};
template <> struct UpType<1> {
    typedef unsigned short word; enum { VEC = 8 };
    static __device__ __forceinline__ float load(word w) { return (float)__builtin_bit_cast(_Float16, w); }
};
template <> struct UpType<2> {
    typedef unsigned short word; enum { VEC = 8 };
    static __device__ __forceinline__ float load(word w) { return __builtin_bit_cast(float, (unsigned)w << 16); }
};
template <typename W, int N> struct alignas(sizeof(W) * N) UpVec { W w[N]; };

template <int KIND, int N>
__device__ __forceinline__ void up_load(const typename UpType<KIND>::word *p, float (&x)[N])
{
    typedef UpVec<typename UpType<KIND>::word, N> V;
    const V v = *reinterpret_cast<const V *>(p);
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] = UpType<KIND>::load(v.w[j]);
}

template <int N>
__device__ __forceinline__ void up_store(float *p, const float (&x)[N])
{
    if constexpr (N == 1) {
        p[0] = x[0];
    } else {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {                        // 16 bytes per store instruction
            UpVec<float, 4> o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o.w[j] = x[4 * q + j];
            *reinterpret_cast<UpVec<float, 4> *>(p + 4 * q) = o;
        }
    }
}

// one tap of weight 1, or two taps with the dyadic weights (S - d) / S and d / S
template <int S, int N>
__device__ __forceinline__ void up_mix(const bool two, const int d, const float (&a)[N], const float (&b)[N], float (&t)[N])
{
    const float w1 = (float)d * (1.0f / S), w0 = (float)(S - d) * (1.0f / S);
#pragma unroll
    for (int j = 0; j < N; ++j) t[j] = two ? __fadd_rn(__fmul_rn(w0, a[j]), __fmul_rn(w1, b[j])) : a[j];
}

template <int KIND, int N, int S>
__device__ __forceinline__ void up_forward_view(const UpView &v, const unsigned block, const unsigned nblocks)
{
    typedef typename UpType<KIND>::word W;
    const W *in = (const W *)v.in;
    const int CV = v.C / N, H = v.H, Wd = v.W, C = v.C;
    for (long long item = (long long)block * UP_BLOCK + threadIdx.x; item < v.items; item += (long long)nblocks * UP_BLOCK) {
        const int cv = (int)(item % CV);
        long long p = item / CV;
        const int ix = (int)(p % Wd);
        p /= Wd;
        const int iy = (int)(p % H);
        const long long b = p / H;
        const bool hx = ix + 1 < Wd, hy = iy + 1 < H;            // a second tap exists (else the clamped tap merges into the first)
        const W *r0 = in + b * v.fs + (long long)iy * v.rs + (long long)ix * v.ps + (long long)cv * N;
        float x00[N], x01[N], x10[N], x11[N];
        up_load<KIND, N>(r0, x00);
        if (hx) up_load<KIND, N>(r0 + v.ps, x01);
        if (hy) up_load<KIND, N>(r0 + v.rs, x10);
        if (hx && hy) up_load<KIND, N>(r0 + v.rs + v.ps, x11);
        if (!hx) {
#pragma unroll
            for (int j = 0; j < N; ++j) x01[j] = x00[j];         // (never mixed in: up_mix selects the single tap)
        }
        if (!hy) {
#pragma unroll
            for (int j = 0; j < N; ++j) x10[j] = x00[j];
        }
        if (!(hx && hy)) {
#pragma unroll
            for (int j = 0; j < N; ++j) x11[j] = x00[j];
        }
        const long long up_row = (long long)Wd * S * C;
        float *o = v.out + ((b * H + iy) * S) * up_row + ((long long)ix * S) * C + (long long)cv * N;
#pragma unroll
        for (int dx = 0; dx < S; ++dx) {
            float t0[N], t1[N];
            up_mix<S, N>(hx && dx > 0, dx, x00, x01, t0);        // horizontal first, on each source row
            up_mix<S, N>(hx && dx > 0, dx, x10, x11, t1);
#pragma unroll
            for (int dy = 0; dy < S; ++dy) {
                float r[N];
                up_mix<S, N>(hy && dy > 0, dy, t0, t1, r);       // then vertically
                up_store<N>(o + dy * up_row + (long long)dx * C, r);
            }
        }
    }
}

template <int N, int S>
__device__ __forceinline__ void up_backward_view(const UpView &v, const unsigned block, const unsigned nblocks)
{
    const float *g = (const float *)v.in;
    const int CV = v.C / N, H = v.H, Wd = v.W, C = v.C;
    const long long up_row = (long long)Wd * S * C;
    for (long long item = (long long)block * UP_BLOCK + threadIdx.x; item < v.items; item += (long long)nblocks * UP_BLOCK) {
        const int cv = (int)(item % CV);
        long long p = item / CV;
        const int ix = (int)(p % Wd);
        p /= Wd;
        const int iy = (int)(p % H);
        const long long b = p / H;
        const float *gb = g + b * H * S * up_row + (long long)cv * N;
        float acc[N];
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = 0.0f;
        // per axis, ascending: the up-indices whose SECOND tap is this pixel (S (i - 1) + d, d = 1 .. S - 1, weight d / S), then those
        // whose first tap it is (S i + d, d = 0 .. S - 1, weight (S - d) / S, or 1 where the clamped second tap merged into it)
#pragma unroll
        for (int ky = 0; ky < 2 * S - 1; ++ky) {
            if (ky < S - 1 && iy == 0) continue;
            const int oy = S * (iy - 1) + 1 + ky;
            const float wy = ky < S - 1 ? (float)(ky + 1) * (1.0f / S) : (iy == H - 1 ? 1.0f : (float)(2 * S - 1 - ky) * (1.0f / S));
#pragma unroll
            for (int kx = 0; kx < 2 * S - 1; ++kx) {
                if (kx < S - 1 && ix == 0) continue;
                const int ox = S * (ix - 1) + 1 + kx;
                const float wx = kx < S - 1 ? (float)(kx + 1) * (1.0f / S) : (ix == Wd - 1 ? 1.0f : (float)(2 * S - 1 - kx) * (1.0f / S));
                const float w = __fmul_rn(wy, wx);                // exact: a product of dyadic weights
                float t[N];
                up_load<0, N>(gb + (long long)oy * up_row + (long long)ox * C, t);
#pragma unroll
                for (int j = 0; j < N; ++j) acc[j] = __fadd_rn(acc[j], __fmul_rn(w, t[j]));
            }
        }
        up_store<N>(v.out + (((b * H + iy) * Wd + ix) * (long long)C) + (long long)cv * N, acc);
    }
}

__device__ __forceinline__ int up_view_of(const UpGroup &g)
{
    int k = 0;
#pragma unroll
    for (int i = 1; i < MV3D_MAX_ROI_VIEWS; ++i)
        if (i < g.n && blockIdx.x >= g.first[i]) k = i;
    return k;
}

template <int KIND>
__device__ __forceinline__ void up_forward_kind(const UpView &v, const unsigned block)
{
    if (v.vec) {
        if (v.s == 2) up_forward_view<KIND, UpType<KIND>::VEC, 2>(v, block, v.blocks);
        else up_forward_view<KIND, UpType<KIND>::VEC, 4>(v, block, v.blocks);
    } else {
        if (v.s == 2) up_forward_view<KIND, 1, 2>(v, block, v.blocks);
        else up_forward_view<KIND, 1, 4>(v, block, v.blocks);
    }
}

__global__ __launch_bounds__(UP_BLOCK) void upsample_bilinear_forward_kernel(const UpGroup g)
{
    const int k = up_view_of(g);
    const UpView &v = g.v[k];
    const unsigned block = blockIdx.x - g.first[k];
    if (v.kind == 0) up_forward_kind<0>(v, block);
    else if (v.kind == 1) up_forward_kind<1>(v, block);
    else up_forward_kind<2>(v, block);
}

__global__ __launch_bounds__(UP_BLOCK) void upsample_bilinear_backward_kernel(const UpGroup g)
{
    const int k = up_view_of(g);
    const UpView &v = g.v[k];
    // Workgroups b and b + 8 share an XCD and its L2 (observed dispatch order; used for speed only, the results do not depend on it).
    // Neighbouring outputs share most of their reads, so every XCD gets a contiguous eighth of the view's items instead of every
    // eighth workgroup: the shared g_y vectors then meet in ONE L2 instead of being fetched by up to four of them.  A view's
    // workgroup count and first workgroup are multiples of 8 (up_group), so the map is a bijection.
    const unsigned b = blockIdx.x - g.first[k];
    const unsigned block = (b & 7u) * (v.blocks >> 3) + (b >> 3);
    if (v.vec) {
        if (v.s == 2) up_backward_view<4, 2>(v, block, v.blocks);
        else up_backward_view<4, 4>(v, block, v.blocks);
    } else {
        if (v.s == 2) up_backward_view<1, 2>(v, block, v.blocks);
        else up_backward_view<1, 4>(v, block, v.blocks);
    }
}

static inline bool up_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// the argument rules both entries share; fills the group the kernels take by value.  Returns the grid size in *blocks.
static int up_group(int num_views, const mv3d_upsample_view *views, bool backward, UpGroup *g, unsigned *blocks)
{
    if (num_views < 1 || num_views > MV3D_MAX_ROI_VIEWS || !views) return MV3D_ERR_INVALID_ARG;
    unsigned total = 0;
    g->n = 0;
    for (int k = 0; k < num_views; ++k) {
        const mv3d_upsample_view &w = views[k];
        if (w.dtype < 0 || w.dtype > 2 || (backward && w.dtype != 0)) return MV3D_ERR_INVALID_ARG;
        if (w.factor != 2 && w.factor != 4) return MV3D_ERR_INVALID_ARG;
        if (w.batch < 0 || w.height < 1 || w.width < 1 || w.channels < 1) return MV3D_ERR_INVALID_ARG;
        const __int128 up = (__int128)w.factor * w.height * w.factor * w.width * w.channels;      // elements of one up-sampled frame
        if (up >= ((__int128)1 << 31)) return MV3D_ERR_INVALID_ARG;
        if (!backward) {
            if (w.pixel_stride < w.channels || w.row_stride / w.pixel_stride < w.width || w.frame_stride / w.row_stride < w.height)
                return MV3D_ERR_INVALID_ARG;
        }
        if (w.batch == 0) continue;
        if (!w.in || !w.out) return MV3D_ERR_INVALID_ARG;
        UpView &v = g->v[g->n];
        v.in = w.in;
        v.out = (float *)w.out;
        v.H = w.height; v.W = w.width; v.C = w.channels; v.s = w.factor;
        v.kind = w.dtype;
        const int N = w.dtype == 0 ? 4 : 8;
        const long long esz = w.dtype == 0 ? 4 : 2;
        v.vec = w.channels % N == 0 && up_aligned16(w.in) && up_aligned16(w.out);
        if (backward) {
            v.fs = v.rs = v.ps = 0;
        } else {
            v.fs = w.frame_stride; v.rs = w.row_stride; v.ps = w.pixel_stride;
            v.vec = v.vec && (v.fs * esz) % 16 == 0 && (v.rs * esz) % 16 == 0 && (v.ps * esz) % 16 == 0;
        }
        v.items = (long long)w.batch * w.height * w.width * (w.channels / (v.vec ? N : 1));
        const long long nb = (v.items + UP_BLOCK - 1) / UP_BLOCK;
        v.blocks = (unsigned)(nb < UP_MAX_VIEW_BLOCKS ? nb : UP_MAX_VIEW_BLOCKS);
        if (backward) v.blocks = (v.blocks + 7u) & ~7u;          // (the backward deals its workgroups out per XCD; the extra ones find no item)
        g->first[g->n] = total;
        total += v.blocks;
        ++g->n;
    }
    for (int k = g->n; k <= MV3D_MAX_ROI_VIEWS; ++k) g->first[k] = total;
    *blocks = total;
    return MV3D_OK;
}

extern "C" int mv3d_upsample_bilinear_views(int num_views, const mv3d_upsample_view *views, void *stream)
{
    UpGroup g;
    unsigned blocks = 0;
    const int st = up_group(num_views, views, false, &g, &blocks);
    if (st != MV3D_OK) return st;
    if (blocks == 0) return MV3D_OK;
    hipLaunchKernelGGL(upsample_bilinear_forward_kernel, dim3(blocks), dim3(UP_BLOCK), 0, (hipStream_t)stream, g);
    return mv3d_launch_status();
}

extern "C" int mv3d_upsample_bilinear_backward_views(int num_views, const mv3d_upsample_view *views, void *stream)
{
    UpGroup g;
    unsigned blocks = 0;
    const int st = up_group(num_views, views, true, &g, &blocks);
    if (st != MV3D_OK) return st;
    if (blocks == 0) return MV3D_OK;
    hipLaunchKernelGGL(upsample_bilinear_backward_kernel, dim3(blocks), dim3(UP_BLOCK), 0, (hipStream_t)stream, g);
    return mv3d_launch_status();
}
