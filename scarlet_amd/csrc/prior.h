// prior.h -- the gradient step of components that carry a Prior (component.py:39-67, 177-187; blend.py:86-96).
//
// The gradient pass runs first with raw_gradient = 1: buffer 1-cur then holds d loss / d sed and d loss / d morph,
// `lipschitz` the scene's constants.  k_prior_step turns the gradients into the stepped factors IN PLACE:
//
//   g_prior = given gradient + w (x - target)            (either part may be missing)
//   L_k     = L + given L + w                            (float32, like the reference's frame dtype)
//   x'      = x - (1 / L_k) (g + g_prior)                (a fixed factor: x' = x, L_k = L)
//
// One workgroup per (component, run of SC_PRIOR_PIX pixels); the first workgroup of every scene also steps the K x B
// SEDs and writes L_comp.  The kernel streams: per pixel it reads x and g, the given gradient and the target where the
// component has them, and writes x' over g.  Nothing is reused, so there is no LDS and no atomic; what matters is bytes
// per instruction and loads in flight.  Where the planes allow 16-byte accesses (H W a multiple of 4, aligned bases)
// a lane issues the loads of four float4 groups of every stream before it uses any of them: 8 to 16 dwordx4 loads
// per lane, 32 - 64 KiB per workgroup, which is what a CU needs in flight to stream at the rate of HBM.  The scalars
// of the component (weights, constants, fix flags, buffer index) depend on blockIdx only and are read once per
// workgroup through the scalar cache.  Inactive scenes and absent components leave at once and cost no traffic; a
// component without a target, a weight of zero or a fixed morphology does not read the streams it does not need.
#pragma once
#include "common.h"
#include "prior_ops.h"

#define SC_PRIOR_GROUPS 4                                       // float4 groups per lane and stream
#define SC_PRIOR_PIX (SC_BLOCK * 4 * SC_PRIOR_GROUPS)           // pixels per workgroup (one 64 x 64 plane)

struct PriorArgs {
    int S, K, B, HW;
    float *sed[2], *morph[2];
    const int *cur;
    const int *active;
    const int *ncomp;             // [S] or NULL (scene_ncomp)
    const uint8_t *fix_sed, *fix_morph;
    const double *lipschitz;      // [S][2], written by the gradient pass
    scarlet_prior p;
};

// (prior_L, the constant a factor steps with, and prior_elem, one element's step: prior_ops.h)
template <bool GIVEN, bool QUAD>
__device__ __forceinline__ void prior_plane_vec(const float *x, float *g, const float *given, const float *target, float w,
                                                float step, int q0, int nq)
{
    // q: index of a float4 group of the plane; lane-contiguous within each of the SC_PRIOR_GROUPS passes
    const f32x4 *x4 = reinterpret_cast<const f32x4 *>(x), *gv4 = reinterpret_cast<const f32x4 *>(given),
                *t4 = reinterpret_cast<const f32x4 *>(target);
    f32x4 *g4 = reinterpret_cast<f32x4 *>(g);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 xv[SC_PRIOR_GROUPS], gv[SC_PRIOR_GROUPS], pv[SC_PRIOR_GROUPS], tv[SC_PRIOR_GROUPS];
#pragma unroll
    for (int j = 0; j < SC_PRIOR_GROUPS; ++j) {
        const int q = q0 + j * SC_BLOCK + (int)threadIdx.x;
        const bool in = q < nq;
        xv[j] = in ? x4[q] : zero;
        gv[j] = in ? g4[q] : zero;
        pv[j] = (GIVEN && in) ? gv4[q] : zero;
        tv[j] = (QUAD && target && in) ? t4[q] : zero;
    }
#pragma unroll
    for (int j = 0; j < SC_PRIOR_GROUPS; ++j) {
        const int q = q0 + j * SC_BLOCK + (int)threadIdx.x;
        if (q < nq) {
            f32x4 o;
            o.x = prior_elem<GIVEN, QUAD>(xv[j].x, gv[j].x, pv[j].x, tv[j].x, w, step);
            o.y = prior_elem<GIVEN, QUAD>(xv[j].y, gv[j].y, pv[j].y, tv[j].y, w, step);
            o.z = prior_elem<GIVEN, QUAD>(xv[j].z, gv[j].z, pv[j].z, tv[j].z, w, step);
            o.w = prior_elem<GIVEN, QUAD>(xv[j].w, gv[j].w, pv[j].w, tv[j].w, w, step);
            g4[q] = o;
        }
    }
}

template <bool GIVEN, bool QUAD>
__device__ __forceinline__ void prior_plane_scalar(const float *x, float *g, const float *given, const float *target, float w,
                                                   float step, int p0, int p_end)
{
#pragma unroll 4
    for (int p = p0 + (int)threadIdx.x; p < p_end; p += SC_BLOCK)
        g[p] = prior_elem<GIVEN, QUAD>(x[p], g[p], GIVEN ? given[p] : 0.f, (QUAD && target) ? target[p] : 0.f, w, step);
}

// grid (S K, ceil(H W / SC_PRIOR_PIX)).  VEC: 16-byte accesses (the host checks H W % 4 == 0 and the alignment).
template <bool VEC>
__global__ __launch_bounds__(SC_BLOCK) void k_prior_step(PriorArgs a)
{
    const int c = blockIdx.x, s = c / a.K, k = c - s * a.K, chunk = blockIdx.y;
    if (!a.active[s]) return;
    const int n = scene_ncomp(a.ncomp, s, a.K);
    if (k >= n) return;                                           // absent component: not read, not written
    const int K = a.K, B = a.B, HW = a.HW;
    const int c0 = a.cur[s];
    const scarlet_prior &pr = a.p;
    const double Ls = a.lipschitz[2 * s], Lm = a.lipschitz[2 * s + 1];

    if (k == 0 && chunk == 0) {
        // the scene's SEDs and the constants of its components
        const float *sx = a.sed[c0] + (size_t)s * K * B;
        float *sg = a.sed[1 - c0] + (size_t)s * K * B;
        for (int i = threadIdx.x; i < n * B; i += SC_BLOCK) {
            const int kk = i / B;
            const size_t cc = (size_t)s * K + kk, e = (size_t)s * K * B + i;
            const float x = sx[i];
            if (a.fix_sed && a.fix_sed[cc]) { sg[i] = x; continue; }
            const float step = 1.0f / (float)prior_L(Ls, pr.L_sed, pr.quad_sed_weight, cc, false);
            float g = sg[i];
            if (pr.grad_sed && pr.quad_sed_weight)
                g = __fadd_rn(g, __fadd_rn(pr.grad_sed[e], __fmul_rn(pr.quad_sed_weight[cc],
                                                                     __fsub_rn(x, pr.quad_sed_target ? pr.quad_sed_target[e] : 0.f))));
            else if (pr.grad_sed) g = __fadd_rn(g, pr.grad_sed[e]);
            else if (pr.quad_sed_weight)
                g = __fadd_rn(g, __fmul_rn(pr.quad_sed_weight[cc], __fsub_rn(x, pr.quad_sed_target ? pr.quad_sed_target[e] : 0.f)));
            sg[i] = x - step * g;
        }
        for (int kk = threadIdx.x; kk < n; kk += SC_BLOCK) {
            const size_t cc = (size_t)s * K + kk;
            pr.L_comp[2 * cc] = prior_L(Ls, pr.L_sed, pr.quad_sed_weight, cc, a.fix_sed && a.fix_sed[cc]);
            pr.L_comp[2 * cc + 1] = prior_L(Lm, pr.L_morph, pr.quad_morph_weight, cc, a.fix_morph && a.fix_morph[cc]);
        }
    }

    // the morphology plane of component c
    const bool fixed = a.fix_morph && a.fix_morph[c];
    const float w = (!fixed && pr.quad_morph_weight) ? pr.quad_morph_weight[c] : 0.f;
    const bool quad = w != 0.f, given = !fixed && pr.grad_morph;
    const float step = 1.0f / (float)prior_L(Lm, pr.L_morph, pr.quad_morph_weight, c, fixed);
    const float *x = a.morph[c0] + (size_t)c * HW;
    float *g = a.morph[1 - c0] + (size_t)c * HW;
    const float *gg = given ? pr.grad_morph + (size_t)c * HW : nullptr;
    const float *tt = (quad && pr.quad_morph_target) ? pr.quad_morph_target + (size_t)c * HW : nullptr;
    if (fixed) {
        // no step: the other buffer receives a copy, as in k_step
        if (VEC) {
            const int nq = HW >> 2;
#pragma unroll
            for (int j = 0; j < SC_PRIOR_GROUPS; ++j) {
                const int q = chunk * (SC_PRIOR_PIX / 4) + j * SC_BLOCK + (int)threadIdx.x;
                if (q < nq) reinterpret_cast<f32x4 *>(g)[q] = reinterpret_cast<const f32x4 *>(x)[q];
            }
        } else {
            const int p_end = min(HW, (chunk + 1) * SC_PRIOR_PIX);
            for (int p = chunk * SC_PRIOR_PIX + (int)threadIdx.x; p < p_end; p += SC_BLOCK) g[p] = x[p];
        }
        return;
    }
#define SC_PRIOR_PLANE(G_, Q_)                                                                                        \
    do {                                                                                                              \
        if (VEC) prior_plane_vec<G_, Q_>(x, g, gg, tt, w, step, chunk * (SC_PRIOR_PIX / 4), HW >> 2);                 \
        else prior_plane_scalar<G_, Q_>(x, g, gg, tt, w, step, chunk * SC_PRIOR_PIX, min(HW, (chunk + 1) * SC_PRIOR_PIX)); \
    } while (0)
    if (given && quad) SC_PRIOR_PLANE(true, true);
    else if (given) SC_PRIOR_PLANE(true, false);
    else if (quad) SC_PRIOR_PLANE(false, true);
    else SC_PRIOR_PLANE(false, false);
#undef SC_PRIOR_PLANE
}
