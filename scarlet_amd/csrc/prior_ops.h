// prior_ops.h -- the arithmetic of a component's Prior (component.py:39-67, 177-187), shared by the kernels that step
// with one: k_prior_step (prior.h, one observation) and k_obs_contract / k_obs_head (multiobs.h, several).
#pragma once
#include "common.h"

// The constant a factor steps with.  A fixed factor takes neither the step nor the prior's L (component.py:182-187);
// without a prior the scene's constant goes through unrounded, so that L_comp then equals `lipschitz`.
__device__ __forceinline__ double prior_L(double L, const float *given, const float *quad, size_t c, bool fixed)
{
    if (fixed) return L;
    const float Lp = (given ? given[c] : 0.f) + (quad ? quad[c] : 0.f);
    return Lp != 0.f ? (double)((float)L + Lp) : L;
}

// One element.  The prior's gradient is rounded operation by operation (no contraction), so that a caller who hands
// the same w (x - target) in as a given gradient gets the same bits; the step itself is k_step's expression.
template <bool GIVEN, bool QUAD>
__device__ __forceinline__ float prior_elem(float x, float g, float given, float target, float w, float step)
{
    if (GIVEN && QUAD) g = __fadd_rn(g, __fadd_rn(given, __fmul_rn(w, __fsub_rn(x, target))));
    else if (GIVEN) g = __fadd_rn(g, given);
    else if (QUAD) g = __fadd_rn(g, __fmul_rn(w, __fsub_rn(x, target)));
    return x - step * g;
}

// The prior's own gradient of one element, given + w (x - target), for the kernels that fold the prior into a pass
// of theirs (multiobs.h).  Every operation is rounded on its own: __fadd_rn / __fmul_rn are plain operators on this
// toolchain and may contract with their neighbours, the pragma keeps these apart.  The result then goes through the
// GIVEN form of prior_elem, so a caller who computes the same w (x - target) with separate float32 operations and
// hands it in as a given gradient gets the same bits by construction.
template <bool GIVEN, bool QUAD>
__device__ __forceinline__ float prior_term(float x, float given, float target, float w)
{
#pragma clang fp contract(off)
    if (GIVEN && QUAD) return given + w * (x - target);
    if (QUAD) return w * (x - target);
    return given;
}

// The same for element e of the SEDs of component c (k_prior_step's cases, prior.h); *has: the component has a term
__device__ __forceinline__ float prior_sed_term(const scarlet_prior &pr, float x, size_t c, size_t e, bool *has)
{
#pragma clang fp contract(off)
    *has = pr.grad_sed || pr.quad_sed_weight;
    const float q = pr.quad_sed_weight ? pr.quad_sed_weight[c] * (x - (pr.quad_sed_target ? pr.quad_sed_target[e] : 0.f)) : 0.f;
    if (pr.grad_sed && pr.quad_sed_weight) return pr.grad_sed[e] + q;
    return pr.grad_sed ? pr.grad_sed[e] : q;
}
