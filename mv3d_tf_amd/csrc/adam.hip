// tf.train.AdamOptimizer's update (lib/fast_rcnn/train_mv.py:138-146: lr 1e-5, beta 0.9 / 0.999, eps 1e-8) for EVERY parameter tensor of the
// graph in ONE launch -- an HBM-bound elementwise pass: 16 B read (param, grad, both moments) + 12 B written per element, 214 M elements =
// 6.0 GB per step of the 3-view graph.  A tensor may name a 16-bit buffer that receives the updated parameter in the same pass (the dense
// head's weights: the next step's GEMMs read them in bf16, so the cast launch and its 4 B / element re-read disappear).
//
// The tensors are cut into chunks of ADAM_CHUNK elements by the host ONCE (chunk -> tensor, offset: two small device tables that only
// change when the parameter list does); workgroup = chunk, so a 100 M-element fc6 matrix and a 64-element bias go through the same grid
// without a tail problem.  Per thread four 16-byte pieces of each array in flight (64 loads per wave before the first use); the moments
// and the parameter are updated in place, f32 throughout, in the order torch's fused Adam evaluates the formula (lerp for the first
// moment), so a step taken here and a step taken by torch.optim.Adam agree to the last bits of the multiply-adds.
//
// mv3d_adam_step_ctl is the same body (the CTL instance of the one kernel template below) on mv3d_solver_tensor records: the gradient
// it feeds to adam_one is g' = coef * g + weight_decay * p (solver.h) with coef and the skip flag read from the device record that
// mv3d_grad_norm (solver.hip) wrote, and the whole step is dropped when skip is set.
#include "solver.h"

template <typename Tensor>
struct AdamArgs {
    const Tensor *tensors;
    const int32_t *chunk_tensor;   // chunk -> tensor index
    const int32_t *chunk_first;    // chunk -> first element / ADAM_CHUNK inside its tensor
    float lr_over_bc1;             // lr / (1 - beta1^t)
    float inv_sqrt_bc2;            // 1 / sqrt(1 - beta2^t)
    float beta1, beta2, eps;
    float omb1, omb2;              // 1 - beta, rounded from the DOUBLE difference as torch rounds them (1.0f - 0.999f is 1.3e-5 off)
    int lowp;                      // type of the optional 16-bit copies (param_lowp): 1 = f16, 2 = bf16
    const mv3d_step_control *control;   // (CTL only) NULL, or the record of mv3d_grad_norm
};

template <typename Tensor>
__device__ __forceinline__ void adam_one(float &p, const float g, float &m, float &v, const AdamArgs<Tensor> &a)
{
    m = m + (g - m) * a.omb1;                                          // lerp(exp_avg, grad, 1 - beta1)
    v = a.beta2 * v + a.omb2 * g * g;
    const float denom = sqrtf(v) * a.inv_sqrt_bc2 + a.eps;
    p = p - a.lr_over_bc1 * (m / denom);
}

__device__ __forceinline__ float *adam_m(const mv3d_adam_tensor &t) { return t.exp_avg; }
__device__ __forceinline__ float *adam_v(const mv3d_adam_tensor &t) { return t.exp_avg_sq; }
__device__ __forceinline__ float *adam_m(const mv3d_solver_tensor &t) { return t.state0; }
__device__ __forceinline__ float *adam_v(const mv3d_solver_tensor &t) { return t.state1; }
__device__ __forceinline__ float adam_decay(const mv3d_adam_tensor &) { return 0.0f; }
__device__ __forceinline__ float adam_decay(const mv3d_solver_tensor &t) { return t.weight_decay; }

// CTL false: mv3d_adam_step, the gradient as it stands.  CTL true: mv3d_adam_step_ctl, adam_one on g' (solver.h), nothing written under skip
template <typename Tensor, bool CTL>
__global__ __launch_bounds__(256) void adam_step_kernel(AdamArgs<Tensor> a)
{
    const int c = blockIdx.x;
    const Tensor t = a.tensors[a.chunk_tensor[c]];
    StepControl sc = {1.0f, false, false};
    if (CTL) {
        sc = step_control(a.control);
        if (sc.skip) return;
    }
    const float wd = adam_decay(t);
    const long long first = (long long)a.chunk_first[c] * ADAM_CHUNK;
    const long long n = t.numel - first < ADAM_CHUNK ? t.numel - first : ADAM_CHUNK;
    float *const p = t.param + first;
    const float *const g = t.grad + first;
    float *const m = adam_m(t) + first, *const v = adam_v(t) + first;
    if (n == ADAM_CHUNK && (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) {
        float4 P[4], G[4], M[4], V[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = u * 256 + threadIdx.x;
            P[u] = reinterpret_cast<const float4 *>(p)[i]; G[u] = reinterpret_cast<const float4 *>(g)[i];
            M[u] = reinterpret_cast<const float4 *>(m)[i]; V[u] = reinterpret_cast<const float4 *>(v)[i];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = u * 256 + threadIdx.x;
            if (CTL) {
                G[u].x = step_gradient(G[u].x, P[u].x, sc, wd); G[u].y = step_gradient(G[u].y, P[u].y, sc, wd);
                G[u].z = step_gradient(G[u].z, P[u].z, sc, wd); G[u].w = step_gradient(G[u].w, P[u].w, sc, wd);
            }
            adam_one(P[u].x, G[u].x, M[u].x, V[u].x, a); adam_one(P[u].y, G[u].y, M[u].y, V[u].y, a);
            adam_one(P[u].z, G[u].z, M[u].z, V[u].z, a); adam_one(P[u].w, G[u].w, M[u].w, V[u].w, a);
            reinterpret_cast<float4 *>(p)[i] = P[u]; reinterpret_cast<float4 *>(m)[i] = M[u]; reinterpret_cast<float4 *>(v)[i] = V[u];
            if (t.param_lowp) adam_lowp_store4((unsigned short *)t.param_lowp + first + 4 * (long long)i, P[u], a.lowp);
        }
        return;
    }
    for (long long i = threadIdx.x; i < n; i += 256) {                 // a tensor's last chunk, or a view at an odd offset
        float pp = p[i], mm = m[i], vv = v[i];
        adam_one(pp, CTL ? step_gradient(g[i], pp, sc, wd) : g[i], mm, vv, a);
        p[i] = pp; m[i] = mm; v[i] = vv;
        if (t.param_lowp) ((unsigned short *)t.param_lowp)[first + i] = adam_lowp(pp, a.lowp);
    }
}

extern "C" int mv3d_adam_chunk_elements(void) { return ADAM_CHUNK; }

template <typename Tensor, bool CTL>
static int adam_launch(const Tensor *tensors_dev, const int32_t *chunk_tensor_dev, const int32_t *chunk_first_dev, int num_chunks, double lr,
                       double beta1, double beta2, double eps, int step, const mv3d_step_control *control_dev, int lowp_dtype, void *stream)
{
    if (!tensors_dev || !chunk_tensor_dev || !chunk_first_dev || num_chunks < 0 || step < 1) return MV3D_ERR_INVALID_ARG;
    if (lowp_dtype < 0 || lowp_dtype > 2) return MV3D_ERR_INVALID_ARG;
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return MV3D_ERR_INVALID_ARG;
    if (num_chunks == 0) return MV3D_OK;
    AdamArgs<Tensor> a;
    a.tensors = tensors_dev; a.chunk_tensor = chunk_tensor_dev; a.chunk_first = chunk_first_dev;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    a.lr_over_bc1 = (float)(lr / bc1);
    a.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    a.beta1 = (float)beta1; a.beta2 = (float)beta2; a.eps = (float)eps;
    a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2);
    a.lowp = lowp_dtype ? lowp_dtype : 2;
    a.control = control_dev;
    hipLaunchKernelGGL((adam_step_kernel<Tensor, CTL>), dim3((unsigned)num_chunks), dim3(256), 0, (hipStream_t)stream, a);
    return mv3d_launch_status();
}

extern "C" int mv3d_adam_step(const mv3d_adam_tensor *tensors_dev, const int32_t *chunk_tensor_dev, const int32_t *chunk_first_dev,
                              int num_chunks, double lr, double beta1, double beta2, double eps, int step, int lowp_dtype, void *stream)
{
    return adam_launch<mv3d_adam_tensor, false>(tensors_dev, chunk_tensor_dev, chunk_first_dev, num_chunks, lr, beta1, beta2, eps, step,
                                                nullptr, lowp_dtype, stream);
}

extern "C" int mv3d_adam_step_ctl(const mv3d_solver_tensor *tensors_dev, const int32_t *chunk_tensor_dev, const int32_t *chunk_first_dev,
                                  int num_chunks, double lr, double beta1, double beta2, double eps, int step,
                                  const mv3d_step_control *control_dev, int lowp_dtype, void *stream)
{
    return adam_launch<mv3d_solver_tensor, true>(tensors_dev, chunk_tensor_dev, chunk_first_dev, num_chunks, lr, beta1, beta2, eps, step,
                                                 control_dev, lowp_dtype, stream);
}
