// multiobs.h -- Blend.fit with SEVERAL observations per blend (blend.py:24-43, 120-139, 219-220) for a whole batch.
//
// The factors live in a STATE batch over the model frame's C channels; observation o is a batch over the channels
// band0[o] .. band0[o] + B_o - 1 with its own images / weights / PSF kernel / workspace.  One iteration:
//
//   k_obs_slice      grid (S)     (observations with a PSF) the K x B_o band slice of the current SEDs
//   PSF chain        existing     (observations with a PSF) model planes from the STATE's morphologies and the slice,
//                                 render, residual, adjoint -> G planes + per-plane losses in the observation's
//                                 workspace (k_psf_conv / k_psf_conv_x128, or the hipFFT chain)
//   k_bigk_lmorph    grid (S)     lambda_max of the SED Gram over the C channels (exact), or sum |sed|^2 (approximate)
//   k_obs_contract   grid (T, S)  ONE pass over the morphologies for all observations: observations without a PSF get
//                                 their weighted residual inline, the others' G planes are read; the summed
//                                 d loss / d morph steps the morphology into buffer 1 - cur; loss and the summed
//                                 d loss / d sed go to the state's partials (engine.h layout, P = n_partials(K, C))
//   Gram / lambda_max existing    the state's morphology Gram (bigk.h for K <= 32, hugek.h above) -> L_sed; for K <= 8
//                                 k_obs_contract sums the Gram itself and k_obs_head finds its lambda_max
//   k_obs_head       grid (S)     L * n_obs, the loss record, the SED step
//
// No morphology is copied and no per-observation gradient plane is written for an observation without a PSF.
// With approximate constants L_morph depends on the loss of the iteration (blend.py:189-201): the contraction then
// runs twice, once for the partial sums and once for the step.
#pragma once
#include "common.h"
#include "engine.h"
#include "prior_ops.h"

#define SC_MAX_OBS 8
#define SC_OBS_J 4                // pixels per thread per sweep of the contraction (SC_BLOCK * SC_OBS_J per sweep)

enum { OBS_FULL = 0, OBS_PARTIALS = 1, OBS_STEP = 2 };

struct ObsView {
    const float *images, *weights;    // [S][B][H][W]; weights NULL -> weight_scalar
    float weight_scalar;
    const float *G;                   // observation with a PSF: G planes [S][B][Fy][Fx] (image at offset (oy, ox) mod F);
                                      // NULL: the residual is computed inline
    int Fy, Fx, oy, ox;
    const double *loss_part;          // with a PSF: per-plane loss sums [S][B]
    int B, band0;
};

struct ObsArgs {
    int S, K, C, H, W, HW, T, n_obs, mode;
    float *sed[2], *morph[2];         // state
    const int *cur, *active, *ncomp;
    const uint8_t *fix_sed, *fix_morph;
    double *partials;                 // state's [S][T][n_partials(K, C)]
    double *lipschitz, *mse;
    int mse_capacity;
    const int *it;
    int head_lsed;                    // 1: K <= 8 with exact constants: k_obs_head finds lambda_max of the Gram partials
    ObsView obs[SC_MAX_OBS];
    scarlet_prior p;                  // read by the PRIOR instances only (scarlet_fit_observations_prior)
};

// the band slice sed[cur][s][k][band0 .. band0 + B - 1] -> out[s][k][0 .. B - 1] (the SEDs an observation's PSF chain reads)
__global__ __launch_bounds__(SC_BLOCK) void k_obs_slice(ObsArgs a, int band0, int B, float *out)
{
    const int s = blockIdx.x;
    if (!a.active[s]) return;
    const float *in = a.sed[a.cur[s]] + (size_t)s * a.K * a.C;
    for (int i = threadIdx.x; i < a.K * B; i += SC_BLOCK) out[(size_t)s * a.K * B + i] = in[(i / B) * a.C + band0 + i % B];
}

// LDS bytes of k_obs_contract: per-wave d loss / d sed sums [SC_NWAVES][K][8] (float64) and the SEDs [K][8]
__host__ __device__ inline size_t obs_contract_lds(int K) { return (size_t)K * SC_BMAX * (SC_NWAVES * sizeof(double) + sizeof(float)); }

// One workgroup per (tile of SC_TILE_PIX pixels, scene).  Per pixel: model_c = sum_k sed[k][c] m_k for the C channels,
// then for every observation and band b (channel c = band0 + b) G_c += w^2 (model_c - image) (inline, loss
// += (w (model_c - image))^2 / 2) or the observation's G plane; then per component d loss / d m_k = sum_c sed[k][c] G_c
// (the step, mode != OBS_PARTIALS) and d loss / d sed[k][c] += m_k G_c (mode != OBS_STEP).  The morphologies are read
// twice by the same thread (the second time from cache).  KS = SC_KMAX: K <= 8, the morphologies of a pixel stay in
// registers and the pass also sums the morphology Gram (engine.h layout, slots 1 + K C ..) -- no Gram pass for small K;
// KS = 0: any K.
// PRIOR (a pass that writes the step; never OBS_PARTIALS): component k steps with 1 / prior_L(L_morph n_obs, ...) and
// its d loss / d m_k goes through prior_elem first -- the given gradient plane plus w (m - target) (prior_term: rounded
// operation by operation), read here, in the pass that holds m and the gradient, once each and only where the component
// has them (prior.h's rules).  The component's scalars are read at the top of its turn, under the loads of m.  The
// prior's planes are read beside m where the registers allow it (KS = 0: all loads of a component's sweep in flight
// together); the register-tiled instance, which holds the Gram sums as well, reads them after the sums of the sweep, all
// SC_OBS_J loads before the first store, and so stays within 128 VGPRs (4 waves per SIMD, as without a prior).
// m, dm, given, target: the SC_OBS_J pixels of this thread, in registers.
template <bool GIVEN, bool QUAD>
__device__ __forceinline__ void obs_prior_store(float *mout, const float *m, const float *dm, const float *given,
                                                const float *target, float w, float step, int p0, int p_end)
{
#pragma unroll
    for (int j = 0; j < SC_OBS_J; ++j) {
        const int p = p0 + j * SC_BLOCK + threadIdx.x;
        if (p >= p_end) continue;
        if (GIVEN || QUAD) {
            const float t = prior_term<GIVEN, QUAD>(m[j], given[j], target[j], w);
            mout[p] = prior_elem<true, false>(m[j], dm[j], t, 0.f, 0.f, step);
        } else
            mout[p] = prior_elem<false, false>(m[j], dm[j], 0.f, 0.f, 0.f, step);
    }
}

template <int KS, bool PRIOR>
__global__ __launch_bounds__(SC_BLOCK) void k_obs_contract(ObsArgs a)
{
    const int s = blockIdx.y, tile = blockIdx.x;
    if (!a.active[s]) return;
    extern __shared__ __align__(16) double obs_lds[];
    __shared__ double lred[SC_NWAVES];
    const int K = a.K, C = a.C, HW = a.HW, W = a.W, n = scene_ncomp(a.ncomp, s, K);
    double *red = obs_lds;                                         // [SC_NWAVES][K][SC_BMAX]
    float *sed_s = (float *)(obs_lds + (size_t)SC_NWAVES * K * SC_BMAX);   // [K][SC_BMAX]
    const int c0 = a.cur[s];
    for (int i = threadIdx.x; i < K * SC_BMAX; i += SC_BLOCK) {
        const int k = i / SC_BMAX, c = i % SC_BMAX;
        sed_s[i] = (k < n && c < C) ? a.sed[c0][((size_t)s * K + k) * C + c] : 0.f;
    }
    for (int i = threadIdx.x; i < SC_NWAVES * K * SC_BMAX; i += SC_BLOCK) red[i] = 0.0;
    __syncthreads();
    const int mode = a.mode;
    const float step_morph = mode == OBS_PARTIALS ? 0.f : 1.0f / (float)(a.lipschitz[2 * s + 1] * (double)a.n_obs);
    const double L_morph = PRIOR ? a.lipschitz[2 * s + 1] * (double)a.n_obs : 0.0;    // (the scene's, before the prior's)
    const float *mor = a.morph[c0] + (size_t)s * K * HW;
    float *mout = a.morph[1 - c0] + (size_t)s * K * HW;
    const int lane = threadIdx.x & (SC_WAVE - 1), wid = threadIdx.x / SC_WAVE;
    double loss = 0;
    constexpr int NG = KS * (KS + 1) / 2 > 0 ? KS * (KS + 1) / 2 : 1;
    constexpr bool EARLY = PRIOR && KS == 0;                         // the prior's planes are loaded beside m
    float gram[NG];
#pragma unroll
    for (int i = 0; i < NG; ++i) gram[i] = 0.f;
    const int p_end = min(HW, (tile + 1) * SC_TILE_PIX);
    for (int p0 = tile * SC_TILE_PIX; p0 < p_end; p0 += SC_BLOCK * SC_OBS_J) {
        float gs[SC_OBS_J][SC_BMAX];
#pragma unroll
        for (int j = 0; j < SC_OBS_J; ++j) {
            const int p = p0 + j * SC_BLOCK + threadIdx.x;
            float model[SC_BMAX];
#pragma unroll
            for (int c = 0; c < SC_BMAX; ++c) { model[c] = 0.f; gs[j][c] = 0.f; }
            if (p >= p_end) continue;
            if (KS > 0) {
                float mk[KS > 0 ? KS : 1];
#pragma unroll
                for (int k = 0; k < KS; ++k) mk[k] = k < n ? mor[(size_t)k * HW + p] : 0.f;
#pragma unroll
                for (int k = 0; k < KS; ++k)
#pragma unroll
                    for (int c = 0; c < SC_BMAX; ++c)
                        if (c < C && k < n) model[c] += sed_s[k * SC_BMAX + c] * mk[k];   // (sed_s has K rows)
                if (mode != OBS_STEP) {
                    int gi = 0;
#pragma unroll
                    for (int k = 0; k < KS; ++k)
#pragma unroll
                        for (int k2 = k; k2 < KS; ++k2) gram[gi++] += mk[k] * mk[k2];
                }
            } else
                for (int k = 0; k < n; ++k) {
                    const float m = mor[(size_t)k * HW + p];
#pragma unroll
                    for (int c = 0; c < SC_BMAX; ++c)
                        if (c < C) model[c] += sed_s[k * SC_BMAX + c] * m;
                }
            const int y = p / W, x = p - y * W;
            for (int o = 0; o < a.n_obs; ++o) {
                const ObsView &v = a.obs[o];
                const size_t base = (size_t)s * v.B;
#pragma unroll
                for (int c = 0; c < SC_BMAX; ++c) {
                    const int b = c - v.band0;
                    if (b < 0 || b >= v.B) continue;
                    if (v.G) {
                        gs[j][c] += v.G[((base + b) * v.Fy + pos_mod(y + v.oy, v.Fy)) * v.Fx + pos_mod(x + v.ox, v.Fx)];
                    } else {
                        const float w = v.weights ? v.weights[(base + b) * HW + p] : v.weight_scalar;
                        const float d = w * (model[c] - v.images[(base + b) * HW + p]);
                        loss += (double)d * (double)d;
                        gs[j][c] += w * d;
                    }
                }
            }
        }
        for (int k = 0; k < n; ++k) {
            const bool fixm = a.fix_morph && a.fix_morph[(size_t)s * K + k];
            float acc[SC_BMAX];
            float mj[PRIOR ? SC_OBS_J : 1], dmj[PRIOR ? SC_OBS_J : 1], gvj[PRIOR ? SC_OBS_J : 1], tgj[PRIOR ? SC_OBS_J : 1];
            // PRIOR: the component's own constant and the streams of its prior -- scalars of (scene, k), chosen outside
            // the pixel loop; a fixed morphology, a weight of 0 or a missing plane reads none of the streams
            float w = 0.f, step = step_morph;
            const float *gg = nullptr, *tt = nullptr;
            if (PRIOR) {
                const size_t cc = (size_t)s * K + k;
                w = (!fixm && a.p.quad_morph_weight) ? a.p.quad_morph_weight[cc] : 0.f;
                step = 1.0f / (float)prior_L(L_morph, a.p.L_morph, a.p.quad_morph_weight, cc, fixm);
                if (!fixm && a.p.grad_morph) gg = a.p.grad_morph + cc * HW;
                if (w != 0.f && a.p.quad_morph_target) tt = a.p.quad_morph_target + cc * HW;
            }
#pragma unroll
            for (int c = 0; c < SC_BMAX; ++c) acc[c] = 0.f;
#pragma unroll
            for (int j = 0; j < SC_OBS_J; ++j) {
                const int p = p0 + j * SC_BLOCK + threadIdx.x;
                if (p >= p_end) continue;
                const float m = mor[(size_t)k * HW + p];
                if (EARLY) { gvj[j] = gg ? gg[p] : 0.f; tgj[j] = tt ? tt[p] : 0.f; }
                float dm = 0.f;
#pragma unroll
                for (int c = 0; c < SC_BMAX; ++c)
                    if (c < C) { dm += sed_s[k * SC_BMAX + c] * gs[j][c]; acc[c] += m * gs[j][c]; }
                if (PRIOR) { mj[j] = m; dmj[j] = dm; }
                else if (mode != OBS_PARTIALS) mout[(size_t)k * HW + p] = fixm ? m : m - step_morph * dm;
            }
            if (PRIOR) {
                float *mo = mout + (size_t)k * HW;
                const bool quad = w != 0.f, given = gg != nullptr;
                if (!EARLY) {
#pragma unroll
                    for (int j = 0; j < SC_OBS_J; ++j) {
                        const int p = p0 + j * SC_BLOCK + threadIdx.x;
                        gvj[j] = (gg && p < p_end) ? gg[p] : 0.f;
                        tgj[j] = (tt && p < p_end) ? tt[p] : 0.f;
                    }
                }
                if (fixm) {
#pragma unroll
                    for (int j = 0; j < SC_OBS_J; ++j) {
                        const int p = p0 + j * SC_BLOCK + threadIdx.x;
                        if (p < p_end) mo[p] = mj[j];
                    }
                }
                else if (given && quad) obs_prior_store<true, true>(mo, mj, dmj, gvj, tgj, w, step, p0, p_end);
                else if (given) obs_prior_store<true, false>(mo, mj, dmj, gvj, tgj, w, step, p0, p_end);
                else if (quad) obs_prior_store<false, true>(mo, mj, dmj, gvj, tgj, w, step, p0, p_end);
                else obs_prior_store<false, false>(mo, mj, dmj, gvj, tgj, w, step, p0, p_end);
            }
            if (mode != OBS_STEP) {
#pragma unroll
                for (int c = 0; c < SC_BMAX; ++c)
                    if (c < C) {
                        const double r = wave_sum((double)acc[c]);
                        if (lane == 0) red[((size_t)wid * K + k) * SC_BMAX + c] += r;    // (each wave owns its slots)
                    }
            }
        }
    }
    if (mode == OBS_STEP) return;
    const int P = n_partials(K, C);
    double *out = a.partials + ((size_t)s * a.T + tile) * P;
    if (KS > 0) {
        // the Gram partials: packed upper triangle of the K x K block (k_bigk_gram's slots)
        __shared__ double gred[SC_NWAVES][NG];
        int gi = 0;
#pragma unroll
        for (int k = 0; k < KS; ++k)
#pragma unroll
            for (int k2 = k; k2 < KS; ++k2) {
                const double r = wave_sum((double)gram[gi]);
                if (lane == 0) gred[wid][gi] = r;
                ++gi;
            }
        __syncthreads();
        for (int k = 0, g2 = 0; k < K; ++k)
            for (int k2 = k; k2 < K; ++k2, ++g2)
                if (threadIdx.x == g2) {
                    const int gk = k * KS - (k * (k - 1)) / 2 + (k2 - k);
                    double r = 0;
#pragma unroll
                    for (int w = 0; w < SC_NWAVES; ++w) r += gred[w][gk];
                    out[1 + K * C + g2] = r;
                }
    }
    loss = block_sum(0.5 * loss, lred);                            // (its barriers also order the `red` updates)
    if (threadIdx.x == 0) {
        double l = loss;
        if (tile == 0)                                             // the losses of the observations with a PSF
            for (int o = 0; o < a.n_obs; ++o)
                if (a.obs[o].G)
                    for (int b = 0; b < a.obs[o].B; ++b) l += a.obs[o].loss_part[(size_t)s * a.obs[o].B + b];
        out[0] = l;
    }
    for (int i = threadIdx.x; i < n * C; i += SC_BLOCK) {
        const int k = i / C, c = i - k * C;
        double r = 0;
#pragma unroll
        for (int w = 0; w < SC_NWAVES; ++w) r += red[((size_t)w * K + k) * SC_BMAX + c];
        out[1 + i] = r;
    }
}

// per scene: the loss record, both Lipschitz constants times n_obs (blend.py:219-220), the SED step (blend.py:91-93)
// PRIOR: every component's SED steps with its own constant and the prior's SED terms (k_prior_step's order), and
// L_comp[s][k] = {L_sed,k, L_morph,k} is written for the present components; `lipschitz` and `mse` hold no prior.
template <bool PRIOR>
__global__ __launch_bounds__(SC_BLOCK) void k_obs_head(ObsArgs a)
{
    const int s = blockIdx.x;
    if (!a.active[s]) return;
    const int K = a.K, C = a.C, P = n_partials(K, C), n = scene_ncomp(a.ncomp, s, K);
    __shared__ float step_s;
    __shared__ double L_s[2];                                          // PRIOR: the scene's constants x n_obs
    __shared__ double Gm[SC_KMAX * SC_KMAX], eig[2][64], lsed;
    if (a.head_lsed) {
        // K <= 8, exact constants: lambda_max of the morphology Gram summed over the tiles (blend.py:205-218)
        for (int i = threadIdx.x; i < SC_KMAX * SC_KMAX; i += SC_BLOCK) {
            const int k = i / SC_KMAX, k2 = i - k * SC_KMAX;
            double r = 0;
            if (k < n && k2 < n) {
                const int lo = k < k2 ? k : k2, hi = k < k2 ? k2 : k;
                const int go = lo * K - (lo * (lo - 1)) / 2 + (hi - lo);
                for (int t = 0; t < a.T; ++t) r += a.partials[((size_t)s * a.T + t) * P + 1 + K * C + go];
            }
            Gm[i] = r;
        }
        __syncthreads();
        if (threadIdx.x < SC_WAVE) {
            double l = 0;
            if (n <= 4) { if (threadIdx.x == 0) l = lambda_max_charpoly4(Gm, n, SC_KMAX); }
            else l = wave_lambda_max8(Gm, n, SC_KMAX, eig);
            if (threadIdx.x == 0) lsed = l;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double loss = 0;
        for (int t = 0; t < a.T; ++t) loss += a.partials[((size_t)s * a.T + t) * P];
        const int it_new = a.it[s] + 1;
        if (it_new <= a.mse_capacity) a.mse[(size_t)s * a.mse_capacity + it_new - 1] = loss;
        const double Ls = (a.head_lsed ? lsed : a.lipschitz[2 * s]) * (double)a.n_obs;
        a.lipschitz[2 * s] = Ls;
        if (PRIOR) {
            const double Lm = a.lipschitz[2 * s + 1] * (double)a.n_obs;
            a.lipschitz[2 * s + 1] = Lm;
            L_s[0] = Ls; L_s[1] = Lm;
        } else
            a.lipschitz[2 * s + 1] *= (double)a.n_obs;
        step_s = 1.0f / (float)Ls;
    }
    __syncthreads();
    const float step_sed = step_s;
    const int c0 = a.cur[s];
    for (int i = threadIdx.x; i < n * C; i += SC_BLOCK) {
        double g = 0;
        for (int t = 0; t < a.T; ++t) g += a.partials[((size_t)s * a.T + t) * P + 1 + i];
        const float x = a.sed[c0][(size_t)s * K * C + i];
        const bool fixed = a.fix_sed && a.fix_sed[(size_t)s * K + i / C];
        if (PRIOR) {
            // a fixed factor takes neither the step nor the prior's constant
            const size_t cc = (size_t)s * K + i / C, e = (size_t)s * K * C + i;
            const float step = 1.0f / (float)prior_L(L_s[0], a.p.L_sed, a.p.quad_sed_weight, cc, false);
            bool has;
            const float t = prior_sed_term(a.p, x, cc, e, &has);
            const float gp = has ? (float)g + t : (float)g;
            a.sed[1 - c0][e] = fixed ? x : x - step * gp;
        } else
            a.sed[1 - c0][(size_t)s * K * C + i] = fixed ? x : x - step_sed * (float)g;
    }
    if (PRIOR)
        for (int k = threadIdx.x; k < n; k += SC_BLOCK) {
            const size_t cc = (size_t)s * K + k;
            a.p.L_comp[2 * cc] = prior_L(L_s[0], a.p.L_sed, a.p.quad_sed_weight, cc, a.fix_sed && a.fix_sed[cc]);
            a.p.L_comp[2 * cc + 1] = prior_L(L_s[1], a.p.L_morph, a.p.quad_morph_weight, cc, a.fix_morph && a.fix_morph[cc]);
        }
}

// CombinedExtendedSource's SED (source.py:183-240 via get_psf_sed, source.py:41-71) for one observation: the pixel
// values of its bands at every present component's centre, / the observation's PSF peak, x the model PSF's max,
// into channels band0 .. band0 + B - 1 of buffer cur.  One thread per component.
__global__ void k_combined_sed(int S, int K, int C, int H, int W, const int *ncomp, const int *status, const int *cur,
                               const int *centers, float *sed0, float *sed1, const float *images, int B, int band0,
                               const float *peak, int peak_stride, const float *model_max)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= S * K) return;
    const int s = c / K;
    if (c - s * K >= scene_ncomp(ncomp, s, K) || (status[s] & SCARLET_STATUS_BAD_INIT)) return;
    const int cy = centers[2 * c], cx = centers[2 * c + 1];
    float *sed = (cur[s] ? sed1 : sed0) + (size_t)c * C + band0;
    for (int b = 0; b < B; ++b) {
        float v = 0.f;
        if (cy >= 0 && cy < H && cx >= 0 && cx < W) {
            v = images[(((size_t)s * B + b) * H + cy) * W + cx];
            if (peak) v = v / peak[(size_t)s * peak_stride + b];
            if (model_max) v = v * *model_max;
        }
        sed[b] = v;
    }
}
