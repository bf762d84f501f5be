// The training solver next to the Adam launch (adam.hip): the global gradient norm with its clip coefficient and non-finite guard, and a
// momentum-SGD step -- streaming passes over the same chunk tables (workgroup = chunk of ADAM_CHUNK elements, chunk -> tensor, first).
//
// mv3d_grad_norm reads 4 B per element (856 MB for the 214 M parameters of the 3-view graph) and leaves a 32-byte record on the device
// that the update launch reads: the host never waits for the norm.  Its sum is ORDER-STABLE: which thread adds an element, and where in
// that thread's chain, depends on the element's index in its chunk only -- thread t owns elements 1024 u + 4 t + j (u, j = 0 .. 3, added
// u-major): on a full 16-byte-aligned chunk these are its four 16-byte pieces, anywhere else the same sixteen elements through scalar
// loads.  Threads -> wave by a fixed butterfly (xor 32, 16, .. 1), the four waves as (w0 + w1) + (w2 + w3), the chunks' partials in a second
// launch of one workgroup: thread t adds partials t, t + 1024, ... in that order, then the same butterfly and a halving tree over the 16
// waves.  Squares are formed in f64 (exact: 24 + 24 bits) and everything is added in f64; no floating-point atomics, no workgroup waits on
// another.  So the 64 bits of the sum are a function of the tensors' sizes and values alone.
//
// mv3d_sgd_step is adam_step_kernel's shape with one state array: 12 B read + 8 B written per element (+ 2 B for a 16-bit copy).
#include "solver.h"

#define FINISH_THREADS MV3D_GRAD_NORM_FINISH_THREADS

// s + (double)g * (double)g.  The product of two f32 values is exact in f64, so the fused form returns the bits of the two-rounding form
__device__ __forceinline__ double sumsq_add(const double s, const float g)
{
    const double x = (double)g;
    return __builtin_fma(x, x, s);
}

// lane 0 of every wave ends with ((s0 + s32) + (s16 + s48)) + ...: a fixed tree whatever the values
__device__ __forceinline__ double wave_sum_f64(double s)
{
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) s = s + __shfl_xor(s, k);
    return s;
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const mv3d_solver_tensor *tensors, const int32_t *chunk_tensor,
                                                         const int32_t *chunk_first, double *partials)
{
    __shared__ double s_wave[4];
    const int c = blockIdx.x;
    const mv3d_solver_tensor t = tensors[chunk_tensor[c]];
    const long long first = (long long)chunk_first[c] * ADAM_CHUNK;
    const long long n = t.numel - first < ADAM_CHUNK ? t.numel - first : ADAM_CHUNK;
    const float *const g = t.grad + first;
    float4 G[4];
    if (n == ADAM_CHUNK && ((uintptr_t)g & 15) == 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) G[u] = reinterpret_cast<const float4 *>(g)[u * 256 + threadIdx.x];
    } else {                                                           // the same sixteen elements; one past the end adds +0 to a sum >= +0
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long i = 1024 * u + 4 * (int)threadIdx.x;
            G[u].x = i + 0 < n ? g[i + 0] : 0.0f; G[u].y = i + 1 < n ? g[i + 1] : 0.0f;
            G[u].z = i + 2 < n ? g[i + 2] : 0.0f; G[u].w = i + 3 < n ? g[i + 3] : 0.0f;
        }
    }
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        s = sumsq_add(s, G[u].x); s = sumsq_add(s, G[u].y); s = sumsq_add(s, G[u].z); s = sumsq_add(s, G[u].w);
    }
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[c] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

__global__ __launch_bounds__(FINISH_THREADS) void grad_norm_finish_kernel(const double *partials, int num_chunks, double max_norm, int guard,
                                                                          mv3d_step_control *control)
{
    __shared__ double s_wave[FINISH_THREADS / 64];
    double s = 0.0;
    int i = threadIdx.x;
    for (; i + 3 * FINISH_THREADS < num_chunks; i += 4 * FINISH_THREADS) {          // four loads in flight, added in index order
        const double a = partials[i], b = partials[i + FINISH_THREADS], c = partials[i + 2 * FINISH_THREADS], d = partials[i + 3 * FINISH_THREADS];
        s = s + a; s = s + b; s = s + c; s = s + d;
    }
    for (; i < num_chunks; i += FINISH_THREADS) s = s + partials[i];
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = FINISH_THREADS / 128; k >= 1; k >>= 1)
        for (int l = 0; l < k; ++l) s_wave[l] = s_wave[l] + s_wave[l + k];
    const double sumsq = s_wave[0], root = sqrt(sumsq);
    const int skip = (guard && !isfinite(sumsq)) ? 1 : 0;
    float coef = 1.0f;
    if (skip) coef = 0.0f;
    else if (max_norm != 0.0 && num_chunks > 0) {                      // torch.nn.utils.clip_grad_norm_: max_norm / (norm + 1e-6), clamped to 1
        const double q = max_norm / (root + 1e-6);
        coef = q >= 1.0 ? 1.0f : (float)q;
    }
    control->sumsq = sumsq;
    control->norm = (float)root;
    control->coef = coef;
    control->skip = skip;
    control->skipped_total += skip;
    control->calls_total += 1;
}

extern "C" int mv3d_grad_norm(const mv3d_solver_tensor *tensors_dev, const int32_t *chunk_tensor_dev, const int32_t *chunk_first_dev,
                              int num_chunks, double max_norm, int guard, double *partials_dev, mv3d_step_control *control_dev, void *stream)
{
    if (!tensors_dev || !chunk_tensor_dev || !chunk_first_dev || !partials_dev || !control_dev || num_chunks < 0) return MV3D_ERR_INVALID_ARG;
    if (!(max_norm >= 0.0) || !isfinite(max_norm)) return MV3D_ERR_INVALID_ARG;
    if (num_chunks > 0)
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)num_chunks), dim3(256), 0, (hipStream_t)stream, tensors_dev, chunk_tensor_dev,
                           chunk_first_dev, partials_dev);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(FINISH_THREADS), 0, (hipStream_t)stream, (const double *)partials_dev, num_chunks,
                       max_norm, guard ? 1 : 0, control_dev);
    return mv3d_launch_status();
}

// ------------------------------------------------------------------------------------------------ momentum SGD
struct SgdArgs {
    const mv3d_solver_tensor *tensors;
    const int32_t *chunk_tensor, *chunk_first;
    float lr, momentum;
    int lowp;                      // type of the optional 16-bit copies: 1 = f16, 2 = bf16
    const mv3d_step_control *control;
};

__device__ __forceinline__ void sgd_one(float &p, const float g, float &buf, const StepControl &sc, const float wd, const SgdArgs &a)
{
    buf = a.momentum * buf + step_gradient(g, p, sc, wd);
    p = p - a.lr * buf;
}

__global__ __launch_bounds__(256) void sgd_step_kernel(SgdArgs a)
{
    const int c = blockIdx.x;
    const StepControl sc = step_control(a.control);
    if (sc.skip) return;                                               // a non-finite norm under the guard: no store of this launch happens
    const mv3d_solver_tensor t = a.tensors[a.chunk_tensor[c]];
    const float wd = t.weight_decay;
    const long long first = (long long)a.chunk_first[c] * ADAM_CHUNK;
    const long long n = t.numel - first < ADAM_CHUNK ? t.numel - first : ADAM_CHUNK;
    float *const p = t.param + first;
    const float *const g = t.grad + first;
    float *const b = t.state0 + first;
    if (n == ADAM_CHUNK && (((uintptr_t)p | (uintptr_t)g | (uintptr_t)b) & 15) == 0) {
        float4 P[4], G[4], B[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = u * 256 + threadIdx.x;
            P[u] = reinterpret_cast<const float4 *>(p)[i]; G[u] = reinterpret_cast<const float4 *>(g)[i];
            B[u] = reinterpret_cast<const float4 *>(b)[i];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = u * 256 + threadIdx.x;
            sgd_one(P[u].x, G[u].x, B[u].x, sc, wd, a); sgd_one(P[u].y, G[u].y, B[u].y, sc, wd, a);
            sgd_one(P[u].z, G[u].z, B[u].z, sc, wd, a); sgd_one(P[u].w, G[u].w, B[u].w, sc, wd, a);
            reinterpret_cast<float4 *>(p)[i] = P[u]; reinterpret_cast<float4 *>(b)[i] = B[u];
            if (t.param_lowp) adam_lowp_store4((unsigned short *)t.param_lowp + first + 4 * (long long)i, P[u], a.lowp);
        }
        return;
    }
    for (long long i = threadIdx.x; i < n; i += 256) {                 // a tensor's last chunk, or a view at an odd offset
        float pp = p[i], bb = b[i];
        sgd_one(pp, g[i], bb, sc, wd, a);
        p[i] = pp; b[i] = bb;
        if (t.param_lowp) ((unsigned short *)t.param_lowp)[first + i] = adam_lowp(pp, a.lowp);
    }
}

extern "C" int mv3d_sgd_step(const mv3d_solver_tensor *tensors_dev, const int32_t *chunk_tensor_dev, const int32_t *chunk_first_dev,
                             int num_chunks, double lr, double momentum, const mv3d_step_control *control_dev, int lowp_dtype, void *stream)
{
    if (!tensors_dev || !chunk_tensor_dev || !chunk_first_dev || num_chunks < 0) return MV3D_ERR_INVALID_ARG;
    if (lowp_dtype < 0 || lowp_dtype > 2) return MV3D_ERR_INVALID_ARG;
    if (!(momentum >= 0.0 && momentum < 1.0) || !(lr >= 0.0) || !isfinite(lr)) return MV3D_ERR_INVALID_ARG;
    if (num_chunks == 0) return MV3D_OK;
    SgdArgs a;
    a.tensors = tensors_dev; a.chunk_tensor = chunk_tensor_dev; a.chunk_first = chunk_first_dev;
    a.lr = (float)lr; a.momentum = (float)momentum;
    a.lowp = lowp_dtype ? lowp_dtype : 2;
    a.control = control_dev;
    hipLaunchKernelGGL(sgd_step_kernel, dim3((unsigned)num_chunks), dim3(256), 0, (hipStream_t)stream, a);
    return mv3d_launch_status();
}
