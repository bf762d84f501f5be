// What the optimizer launches share (adam.hip, solver.hip): the chunk size, the 16-bit copy of an updated parameter, and ONE statement of
// the controlled gradient g' = coef * g + weight_decay * p that the momentum-SGD body and the controlled Adam body both start from.
#pragma once
#include "common.h"

#define ADAM_CHUNK 4096            // elements per workgroup (256 threads x 4 pieces x 4 floats)

// the updated parameter in the 16-bit type the next step's GEMMs read it in (round to nearest even: what a cast launch would write)
__device__ __forceinline__ unsigned short adam_lowp(const float x, const int kind)
{
    if (kind == 1) { const _Float16 h = (_Float16)x; return __builtin_bit_cast(unsigned short, h); }
    const __bf16 h = (__bf16)x;
    return __builtin_bit_cast(unsigned short, h);
}

// four updated parameters -> their 16-bit copies at q: one 8-byte store where q allows it, four 2-byte stores elsewhere
__device__ __forceinline__ void adam_lowp_store4(unsigned short *const q, const float4 P, const int kind)
{
    const uint2 w = {(unsigned)adam_lowp(P.x, kind) | ((unsigned)adam_lowp(P.y, kind) << 16),
                     (unsigned)adam_lowp(P.z, kind) | ((unsigned)adam_lowp(P.w, kind) << 16)};
    if (((uintptr_t)q & 7) == 0) *reinterpret_cast<uint2 *>(q) = w;
    else { q[0] = (unsigned short)w.x; q[1] = (unsigned short)(w.x >> 16); q[2] = (unsigned short)w.y; q[3] = (unsigned short)(w.y >> 16); }
}

// what a controlled step reads of the control record, once per workgroup (mv3d_grad_norm wrote it earlier on the same stream; a NULL
// record is coef 1, no skip)
struct StepControl {
    float coef;
    bool scale;                    // coef != 1: the product is evaluated (1.0f * g is g anyway; the flag keeps the vector body free of it)
    bool skip;
};

__device__ __forceinline__ StepControl step_control(const mv3d_step_control *const c)
{
    StepControl s = {1.0f, false, false};
    if (c) { s.coef = c->coef; s.scale = s.coef != 1.0f; s.skip = c->skip != 0; }
    return s;
}

// g' = coef * g (+ weight_decay * p): each part only where it applies, so that a parameter or gradient holding inf never meets a zero factor
__device__ __forceinline__ float step_gradient(float g, const float p, const StepControl &s, const float weight_decay)
{
    if (s.scale) g = s.coef * g;
    if (weight_decay != 0.0f) g = g + weight_decay * p;
    return g;
}
