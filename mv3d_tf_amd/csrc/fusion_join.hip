// The deep-fusion join: after a fully connected layer of the head the views' activations are joined by an
// element-wise mean (MV3D paper §3.3, Fig. 3c), for the main network and every auxiliary path in ONE launch each way:
//     forward    out[p][e] = dropout_p( (sum over the kept views v of path p, ascending, of relu(h[s][v][e])) / n_p )
//     backward   g_h[s][v][e] = sum over the paths p that read set s, ascending, of (keep[p][v] && h > 0) ? t_p[e] / n_p : 0
// h is the layer's pre-ReLU GEMM output (sets_in, views, E) with E = rows * channels, out / g_out are (paths, E); s = p when
// sets_in == paths, 0 when every path reads the same h.  The operation is elementwise over e, so a thread owns ONE 16-byte vector
// of a plane (4 f32 / 8 16-bit elements) and walks the views and paths in registers: with sets_in == 1 every view is loaded once
// for all paths (forward) and the paths' gradients meet in a register in ascending p (backward) -- no atomics, no workspace, the
// same bits on every run.  All arithmetic is f32 (-ffp-contract=off: the mean's divide and the dropout scale are separate
// roundings), the store rounds to nearest even, a NaN result is stored as the type's canonical quiet NaN.  The keep table travels
// by value in the kernel arguments (nothing to upload, so the launch can be captured in a graph); a view no path keeps is never
// read, and the backward writes zeros for it (the batched GEMM behind reads the whole buffer).
// Planes are addressed flat: vectors are used when E is a multiple of the vector width and every base pointer is 16-byte aligned
// (then every plane starts on a vector boundary), the scalar instantiation of the same body for the WHOLE launch otherwise: the
// planes start at multiples of E, so with E % vector != 0 they are misaligned against each other and a vector body + scalar tail
// has no element range that is aligned in all of them (an odd E at serving size pays several times the bandwidth; C = 2048 never
// does).  The grid is sized from the vector count (256 threads, at most 2048 workgroups, grid-stride beyond), offsets are 64-bit.
#include "common.h"

#define FJ_BLOCK 256
#define FJ_MAX_GRID 2048
#define FJ_MAX_PATHS 8
#define FJ_MAX_VIEWS 4

struct FjTable {
    unsigned char keep[FJ_MAX_PATHS][FJ_MAX_VIEWS];   // 0 / 1
    unsigned char used[FJ_MAX_PATHS][FJ_MAX_VIEWS];   // [s][v]: some path reading set s keeps view v
    float n[FJ_MAX_PATHS];                            // kept views of a path, as the divisor
};

template <int KIND> struct FjType;                    // 0 = f32, 1 = f16, 2 = bf16: storage word, vector of 16 bytes, conversions
template <> struct FjType<0> {
    typedef float word; enum { VEC = 4 };
    static __device__ __forceinline__ float load(word w) { return w; }
    static __device__ __forceinline__ word store(float x) { return x != x ? __builtin_bit_cast(float, 0x7FC00000u) : x; }
};
template <> struct FjType<1> {
    typedef unsigned short word; enum { VEC = 8 };
    static __device__ __forceinline__ float load(word w) { return (float)__builtin_bit_cast(_Float16, w); }
    static __device__ __forceinline__ word store(float x)
    {
        if (x != x) return (word)0x7E00u;
        const _Float16 h = (_Float16)x;                                   // round to nearest even
        return __builtin_bit_cast(unsigned short, h);
    }
};
template <> struct FjType<2> {
    typedef unsigned short word; enum { VEC = 8 };
    static __device__ __forceinline__ float load(word w) { return __builtin_bit_cast(float, (unsigned)w << 16); }
    static __device__ __forceinline__ word store(float x)
    {
        if (x != x) return (word)0x7FC0u;
        const unsigned u = __builtin_bit_cast(unsigned, x);
        return (word)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);            // round to nearest even (inf stays inf)
    }
};

template <typename W, int N> struct alignas(sizeof(W) * N) FjVec { W w[N]; };

template <int KIND, int N>
__global__ __launch_bounds__(FJ_BLOCK) void fusion_join_forward_kernel(const typename FjType<KIND>::word *__restrict__ h, const int sets_in, const int paths,
                                                                       const int views, const long long E, const FjTable tab,
                                                                       const unsigned char *__restrict__ drop, const float scale,
                                                                       typename FjType<KIND>::word *__restrict__ out)
{
    typedef FjType<KIND> T;
    typedef FjVec<typename T::word, N> V;
    typedef FjVec<unsigned char, N> D;
    const long long nvec = E / N;
    for (long long i = (long long)blockIdx.x * FJ_BLOCK + threadIdx.x; i < nvec; i += (long long)gridDim.x * FJ_BLOCK) {
        const long long e = i * N;
        float a[FJ_MAX_VIEWS][N];
        if (sets_in == 1) {
#pragma unroll
            for (int v = 0; v < FJ_MAX_VIEWS; ++v)
                if (v < views && tab.used[0][v]) {
                    const V x = *reinterpret_cast<const V *>(h + (long long)v * E + e);
#pragma unroll
                    for (int j = 0; j < N; ++j) { const float f = T::load(x.w[j]); a[v][j] = f < 0.0f ? 0.0f : f; }
                }
        }
        for (int p = 0; p < paths; ++p) {
            if (sets_in != 1) {
#pragma unroll
                for (int v = 0; v < FJ_MAX_VIEWS; ++v)
                    if (v < views && tab.keep[p][v]) {
                        const V x = *reinterpret_cast<const V *>(h + ((long long)p * views + v) * E + e);
#pragma unroll
                        for (int j = 0; j < N; ++j) { const float f = T::load(x.w[j]); a[v][j] = f < 0.0f ? 0.0f : f; }
                    }
            }
            float s[N];
#pragma unroll
            for (int j = 0; j < N; ++j) s[j] = 0.0f;
#pragma unroll
            for (int v = 0; v < FJ_MAX_VIEWS; ++v)
                if (v < views && tab.keep[p][v]) {
#pragma unroll
                    for (int j = 0; j < N; ++j) s[j] = s[j] + a[v][j];
                }
            const float n = tab.n[p];
            V o;
            if (drop) {
                const D d = *reinterpret_cast<const D *>(drop + (long long)p * E + e);
#pragma unroll
                for (int j = 0; j < N; ++j) { const float m = s[j] / n; o.w[j] = T::store(d.w[j] ? m * scale : 0.0f); }
            } else {
#pragma unroll
                for (int j = 0; j < N; ++j) o.w[j] = T::store(s[j] / n);
            }
            *reinterpret_cast<V *>(out + (long long)p * E + e) = o;
        }
    }
}

template <int KIND, int N>
__global__ __launch_bounds__(FJ_BLOCK) void fusion_join_backward_kernel(const typename FjType<KIND>::word *__restrict__ h,
                                                                        const typename FjType<KIND>::word *__restrict__ g_out, const int sets_in,
                                                                        const int paths, const int views, const long long E, const FjTable tab,
                                                                        const unsigned char *__restrict__ drop, const float scale,
                                                                        typename FjType<KIND>::word *__restrict__ g_h)
{
    typedef FjType<KIND> T;
    typedef FjVec<typename T::word, N> V;
    typedef FjVec<unsigned char, N> D;
    const long long nvec = E / N;
    for (long long i = (long long)blockIdx.x * FJ_BLOCK + threadIdx.x; i < nvec; i += (long long)gridDim.x * FJ_BLOCK) {
        const long long e = i * N;
        float x[FJ_MAX_VIEWS][N], acc[FJ_MAX_VIEWS][N];
        if (sets_in == 1) {
#pragma unroll
            for (int v = 0; v < FJ_MAX_VIEWS; ++v) {
#pragma unroll
                for (int j = 0; j < N; ++j) acc[v][j] = 0.0f;
                if (v < views && tab.used[0][v]) {
                    const V w = *reinterpret_cast<const V *>(h + (long long)v * E + e);
#pragma unroll
                    for (int j = 0; j < N; ++j) x[v][j] = T::load(w.w[j]);
                }
            }
        }
        for (int p = 0; p < paths; ++p) {
            const V g = *reinterpret_cast<const V *>(g_out + (long long)p * E + e);
            const float n = tab.n[p];
            float q[N];                                                  // t / n_p: the same for every kept view of the path
            if (drop) {
                const D d = *reinterpret_cast<const D *>(drop + (long long)p * E + e);
#pragma unroll
                for (int j = 0; j < N; ++j) q[j] = (T::load(g.w[j]) * (d.w[j] ? scale : 0.0f)) / n;
            } else {
#pragma unroll
                for (int j = 0; j < N; ++j) q[j] = T::load(g.w[j]) / n;
            }
            if (sets_in == 1) {
#pragma unroll
                for (int v = 0; v < FJ_MAX_VIEWS; ++v)
                    if (v < views && tab.keep[p][v]) {
#pragma unroll
                        for (int j = 0; j < N; ++j) acc[v][j] = acc[v][j] + (x[v][j] > 0.0f ? q[j] : 0.0f);
                    }
            } else {
#pragma unroll
                for (int v = 0; v < FJ_MAX_VIEWS; ++v)
                    if (v < views) {
                        const long long off = ((long long)p * views + v) * E + e;
                        V o;
                        if (tab.keep[p][v]) {
                            const V w = *reinterpret_cast<const V *>(h + off);
#pragma unroll
                            for (int j = 0; j < N; ++j) o.w[j] = T::store(T::load(w.w[j]) > 0.0f ? q[j] : 0.0f);
                        } else {
#pragma unroll
                            for (int j = 0; j < N; ++j) o.w[j] = T::store(0.0f);
                        }
                        *reinterpret_cast<V *>(g_h + off) = o;
                    }
            }
        }
        if (sets_in == 1) {
#pragma unroll
            for (int v = 0; v < FJ_MAX_VIEWS; ++v)
                if (v < views) {
                    V o;
#pragma unroll
                    for (int j = 0; j < N; ++j) o.w[j] = T::store(acc[v][j]);
                    *reinterpret_cast<V *>(g_h + (long long)v * E + e) = o;
                }
        }
    }
}

// the argument rules both entries share; fills the table the kernels take by value
static int fj_table(int dtype, int sets_in, int paths, int views, int rows, int channels, const unsigned char *keep, FjTable *tab, long long *E)
{
    if (dtype < 0 || dtype > 2) return MV3D_ERR_INVALID_ARG;
    if (views < 1 || views > FJ_MAX_VIEWS || paths < 1 || paths > FJ_MAX_PATHS) return MV3D_ERR_INVALID_ARG;
    if (sets_in != 1 && sets_in != paths) return MV3D_ERR_INVALID_ARG;
    if (rows < 0 || channels < 1 || !keep) return MV3D_ERR_INVALID_ARG;
    *E = (long long)rows * channels;
    if (*E > (1LL << 48)) return MV3D_ERR_INVALID_ARG;
    for (int p = 0; p < FJ_MAX_PATHS; ++p) {
        tab->n[p] = 1.0f;
        for (int v = 0; v < FJ_MAX_VIEWS; ++v) tab->keep[p][v] = tab->used[p][v] = 0;
    }
    for (int p = 0; p < paths; ++p) {
        int n = 0;
        for (int v = 0; v < views; ++v)
            if (keep[p * views + v]) {
                tab->keep[p][v] = 1;
                tab->used[sets_in == 1 ? 0 : p][v] = 1;
                ++n;
            }
        if (n == 0) return MV3D_ERR_INVALID_ARG;
        tab->n[p] = (float)n;
    }
    return MV3D_OK;
}

static inline bool fj_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
static inline unsigned fj_grid(long long nvec)
{
    const long long b = (nvec + FJ_BLOCK - 1) / FJ_BLOCK;
    return (unsigned)(b < FJ_MAX_GRID ? b : FJ_MAX_GRID);
}

template <int KIND>
static void fj_forward(const void *h, int sets_in, int paths, int views, long long E, const FjTable &tab, const unsigned char *drop, float scale,
                       void *out, hipStream_t st)
{
    typedef typename FjType<KIND>::word W;
    const int N = FjType<KIND>::VEC;
    const bool vec = E % N == 0 && fj_aligned16(h) && fj_aligned16(out) && (!drop || ((uintptr_t)drop & (N - 1)) == 0);
    if (vec)
        hipLaunchKernelGGL((fusion_join_forward_kernel<KIND, FjType<KIND>::VEC>), dim3(fj_grid(E / N)), dim3(FJ_BLOCK), 0, st, (const W *)h, sets_in, paths,
                           views, E, tab, drop, scale, (W *)out);
    else
        hipLaunchKernelGGL((fusion_join_forward_kernel<KIND, 1>), dim3(fj_grid(E)), dim3(FJ_BLOCK), 0, st, (const W *)h, sets_in, paths, views, E, tab,
                           drop, scale, (W *)out);
}

template <int KIND>
static void fj_backward(const void *h, const void *g_out, int sets_in, int paths, int views, long long E, const FjTable &tab,
                        const unsigned char *drop, float scale, void *g_h, hipStream_t st)
{
    typedef typename FjType<KIND>::word W;
    const int N = FjType<KIND>::VEC;
    const bool vec = E % N == 0 && fj_aligned16(h) && fj_aligned16(g_out) && fj_aligned16(g_h) && (!drop || ((uintptr_t)drop & (N - 1)) == 0);
    if (vec)
        hipLaunchKernelGGL((fusion_join_backward_kernel<KIND, FjType<KIND>::VEC>), dim3(fj_grid(E / N)), dim3(FJ_BLOCK), 0, st, (const W *)h,
                           (const W *)g_out, sets_in, paths, views, E, tab, drop, scale, (W *)g_h);
    else
        hipLaunchKernelGGL((fusion_join_backward_kernel<KIND, 1>), dim3(fj_grid(E)), dim3(FJ_BLOCK), 0, st, (const W *)h, (const W *)g_out, sets_in,
                           paths, views, E, tab, drop, scale, (W *)g_h);
}

extern "C" int mv3d_fusion_join_forward(const void *h_dev, int dtype, int sets_in, int paths, int views, int rows, int channels,
                                        const uint8_t *keep, const uint8_t *drop_dev, float scale, void *out_dev, void *stream)
{
    FjTable tab;
    long long E = 0;
    const int st = fj_table(dtype, sets_in, paths, views, rows, channels, keep, &tab, &E);
    if (st != MV3D_OK) return st;
    if (E == 0) return MV3D_OK;
    if (!h_dev || !out_dev) return MV3D_ERR_INVALID_ARG;
    if (dtype == 0) fj_forward<0>(h_dev, sets_in, paths, views, E, tab, drop_dev, scale, out_dev, (hipStream_t)stream);
    else if (dtype == 1) fj_forward<1>(h_dev, sets_in, paths, views, E, tab, drop_dev, scale, out_dev, (hipStream_t)stream);
    else fj_forward<2>(h_dev, sets_in, paths, views, E, tab, drop_dev, scale, out_dev, (hipStream_t)stream);
    return mv3d_launch_status();
}

extern "C" int mv3d_fusion_join_backward(const void *h_dev, const void *g_out_dev, int dtype, int sets_in, int paths, int views, int rows,
                                         int channels, const uint8_t *keep, const uint8_t *drop_dev, float scale, void *g_h_dev, void *stream)
{
    FjTable tab;
    long long E = 0;
    const int st = fj_table(dtype, sets_in, paths, views, rows, channels, keep, &tab, &E);
    if (st != MV3D_OK) return st;
    if (E == 0) return MV3D_OK;
    if (!h_dev || !g_out_dev || !g_h_dev) return MV3D_ERR_INVALID_ARG;
    if (dtype == 0) fj_backward<0>(h_dev, g_out_dev, sets_in, paths, views, E, tab, drop_dev, scale, g_h_dev, (hipStream_t)stream);
    else if (dtype == 1) fj_backward<1>(h_dev, g_out_dev, sets_in, paths, views, E, tab, drop_dev, scale, g_h_dev, (hipStream_t)stream);
    else fj_backward<2>(h_dev, g_out_dev, sets_in, paths, views, E, tab, drop_dev, scale, g_h_dev, (hipStream_t)stream);
    return mv3d_launch_status();
}
