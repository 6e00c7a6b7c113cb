// multiobs_wide.h -- the joint fit of multiobs.h over a model frame of 8 < C <= 32 channels (SCARLET_MAX_CHANNELS).
//
// Every observation still has at most 8 bands: its PSF chain, k_lowres_planes, the streamed low-resolution chain and
// k_obs_slice work on its own slice and take C as a stride.  k_obs_head loops over n C.  What sees all C channels at
// once is the contraction over the observations and lambda_max of the SED Gram; this file holds their wide forms.
//
//   k_wide_lmorph        grid (S)     lambda_max of the n x n SED Gram, n = min(K, C) <= 32, float64, by repeated squaring
//                                     (the scheme of k_bigk_lipschitz); or sum |sed|^2 with approximate constants
//   k_obs_contract_wide  grid (T, S)  k_obs_contract for C <= CW channels, CW = 16 or 32, any K <= 256
//
// The morphology Gram (L_sed) of a wide state comes from the Gram passes of its K range for every K (bigk.h up to 32
// components, hugek.h above): the wide contraction sums no Gram of its own.
//
// k_obs_contract_wide, a vector formulation.  A thread owns J pixels of a sweep (J = 4 at CW = 16, 2 at CW = 32) and
// keeps their summed gradient G[J][CW] in registers, so the morphologies are read twice, as in k_obs_contract: once for
// the model (formed in the registers that then hold G) and once for the step and the SED sums.  The SEDs lie in LDS, rows padded
// with zeros to CW floats: all lanes read the same address (a broadcast, 16 bytes at a time) and no channel loop
// branches on C.  Which observations cover a channel is a small list in LDS built once per workgroup, so the residual
// loop runs sum_o B_o times per pixel and not n_obs x CW times.
// d loss / d sed: a wave holds acc[CW] per lane for component k.  Instead of CW all-lane sums it runs a reduce-scatter:
// a step over lane distance d sends the half of the values the partner keeps and adds what arrives, so 32 -> 16 -> .. 1
// values are live and CW - 1 float64 exchanges (the first CW / 2 move float32) replace 6 CW; the remaining steps sum the
// one value left.  Lane l ends with channel l CW / 64, summed over the wave in a fixed order, and adds it to the wave's
// float64 slot [wave][k][c] in LDS.  Those slots are what limits the workgroup: K C (8 NW + 4 CW / C) bytes for NW
// waves.  contract_plan (launch_plan.h) takes the most waves (4, 2 or 1) whose slots fit; four waves hold K C <= ~4400,
// which covers K = 256 at C = 17 with two and every (K, C) with one.
#pragma once
#include "bigk.h"
#include "psf_path.h"
#include "multiobs.h"

#define SC_CMAX 32                // SCARLET_MAX_CHANNELS

// LDS bytes of k_obs_contract_wide<CW, NW>: the SEDs [K][CW], the waves' d loss / d sed slots [NW][K][C] (float64)
__host__ __device__ inline size_t obs_contract_wide_lds(int K, int C, int CW, int NW)
{
    return (size_t)K * ((size_t)NW * C * sizeof(double) + (size_t)CW * sizeof(float));
}
// LDS bytes of k_wide_lmorph: the SEDs [K][C]
__host__ __device__ inline size_t wide_lmorph_lds(int K, int C) { return (size_t)K * C * sizeof(float); }

// ---- lambda_max(A^T A) of the K x C SED matrix through the smaller of its two Gram matrices (blend.py:205-218), one
// workgroup per scene.  M = G / tr G is squared SC_SQUARINGS times (bigk.h: the bound on what the Rayleigh quotient of
// the heaviest column misses, n / (e 2^31) relative, holds for any n <= 32); a thread owns a 2 x 2 block of the product.
// Rows of absent components are zero in the state's buffers and add zero rows and columns.
__global__ __launch_bounds__(SC_BLOCK) void k_wide_lmorph(GradArgs a)
{
    const int s = blockIdx.x;
    if (!a.active[s]) return;
    const int K = a.K, C = a.B, P = n_partials(K, C), tid = threadIdx.x, lane = tid & (SC_WAVE - 1);
    constexpr int N = SC_CMAX, LD = N + 1;
    extern __shared__ __align__(16) float wl_sed[];                    // [K][C]
    __shared__ double Gm[N][LD], M0[N][LD], M1[N][LD];
    __shared__ double red[SC_NWAVES];
    const float *sed = a.sed[a.cur[s]] + (size_t)s * K * C;
    for (int i = tid; i < K * C; i += SC_BLOCK) wl_sed[i] = sed[i];
    __syncthreads();
    double L_morph;
    if (a.approximate_L) {
        double LS = 0, loss = 0;
        for (int i = tid; i < K * C; i += SC_BLOCK) LS += (double)wl_sed[i] * wl_sed[i];
        LS = block_sum(LS, red);
        for (int t = 0; t < a.T; ++t) loss += a.partials[((size_t)s * a.T + t) * P];
        const int it_new = a.it[s] + 1;
        if (it_new > 1 && loss > a.mse[(size_t)s * a.mse_capacity + it_new - 2]) LS *= 2;
        L_morph = LS;
    } else {
        const int n = K < C ? K : C;
        for (int i = tid; i < N * N; i += SC_BLOCK) {
            const int x = i / N, y = i - x * N;
            double r = 0;
            if (x < n && y < n) {
                if (K < C) for (int c = 0; c < C; ++c) r += (double)wl_sed[x * C + c] * wl_sed[y * C + c];
                else       for (int k = 0; k < K; ++k) r += (double)wl_sed[k * C + x] * wl_sed[k * C + y];
            }
            Gm[x][y] = r;
        }
        __syncthreads();
        double trace = tid < N ? Gm[tid][tid] : 0.0;
        trace = block_sum(trace, red);
        L_morph = 0;
        if (trace != 0) {                                              // (uniform: every thread holds the block's sum)
            const double inv = 1.0 / trace;
            for (int i = tid; i < N * N; i += SC_BLOCK) M0[i / N][i % N] = Gm[i / N][i % N] * inv;
            __syncthreads();
            const int bi = (tid >> 4) << 1, bj = (tid & 15) << 1;
            double (*src)[LD] = M0, (*dst)[LD] = M1;
            for (int q = 0; q < SC_SQUARINGS; ++q) {
                double a00 = 0, a01 = 0, a10 = 0, a11 = 0;
#pragma unroll 2
                for (int k = 0; k < N; k += 4) {
                    double u0[4], u1[4], v0[4], v1[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) { u0[e] = src[bi][k + e]; u1[e] = src[bi + 1][k + e]; v0[e] = src[k + e][bj]; v1[e] = src[k + e][bj + 1]; }
#pragma unroll
                    for (int e = 0; e < 4; ++e) { a00 += u0[e] * v0[e]; a01 += u0[e] * v1[e]; a10 += u1[e] * v0[e]; a11 += u1[e] * v1[e]; }
                }
                // renormalised by the trace every fourth squaring (lambda_1 >= tr / 32: no underflow in between)
                double sc = 1.0;
                if ((q & 3) == 3 || q == SC_SQUARINGS - 1) {
                    double tr = (bi == bj) ? a00 + a11 : 0.0;
                    tr = block_sum(tr, red);
                    sc = 1.0 / tr;
                }
                dst[bi][bj] = a00 * sc; dst[bi][bj + 1] = a01 * sc; dst[bi + 1][bj] = a10 * sc; dst[bi + 1][bj + 1] = a11 * sc;
                __syncthreads();
                double (*tmp)[LD] = src; src = dst; dst = tmp;
            }
            if (tid < SC_WAVE) {
                // heaviest column of the (rank-one) power, lowest index on ties; Rayleigh quotient with G
                double best = lane < N ? src[lane][lane] : -1.0;
                int bidx = lane;
                for (int o = 32; o > 0; o >>= 1) {
                    const double b2 = __shfl_xor(best, o, SC_WAVE);
                    const int i2 = __shfl_xor(bidx, o, SC_WAVE);
                    if (b2 > best || (b2 == best && i2 < bidx)) { best = b2; bidx = i2; }
                }
                double v = lane < N ? src[lane][bidx] : 0.0, gv = 0;
                if (lane < N) dst[0][lane] = v;
                wave_sync();
                if (lane < N)
                    for (int j = 0; j < N; ++j) gv += Gm[lane][j] * dst[0][j];
                const double num = wave_sum(v * gv), den = wave_sum(v * v);
                L_morph = num / den;
            }
        }
    }
    if (tid == 0) a.lipschitz[2 * s + 1] = L_morph;
}

// ---- the d loss / d sed sums of one component over a wave: acc[c] of every lane -> the wave's sum of channel
// c = lane CW / 64 in every lane of that channel's group (float64, the same order in every launch)
template <int CW>
__device__ __forceinline__ double wave_reduce_scatter(const float (&acc)[CW], int lane)
{
    constexpr int H1 = CW / 2;
    double v[H1];
    const bool hi = (lane & 32) != 0;
    // distance 32: the values travel as float32 (widening commutes with the move)
#pragma unroll
    for (int i = 0; i < H1; ++i) {
        const float keep = hi ? acc[i + H1] : acc[i], send = hi ? acc[i] : acc[i + H1];
        v[i] = (double)keep + (double)__shfl_xor(send, 32, SC_WAVE);
    }
    int off = 16;
#pragma unroll
    for (int h = H1 / 2; h >= 1; h /= 2) {
        const bool up = (lane & off) != 0;
#pragma unroll
        for (int i = 0; i < h; ++i) {
            const double keep = up ? v[i + h] : v[i], send = up ? v[i] : v[i + h];
            v[i] = keep + __shfl_xor(send, off, SC_WAVE);
        }
        off >>= 1;
    }
    // one value left: the lanes of a channel's group sum it among themselves
#pragma unroll
    for (; off >= 1; off >>= 1) v[0] += __shfl_xor(v[0], off, SC_WAVE);
    return v[0];
}

// obs_prior_store of multiobs.h for J pixels per thread at a stride of NT threads
template <int J, int NT, bool GIVEN, bool QUAD>
__device__ __forceinline__ void obs_prior_store_wide(float *mout, const float *m, const float *dm, const float *given,
                                                     const float *target, float w, float step, int p0, int p_end)
{
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int p = p0 + j * NT + threadIdx.x;
        if (p >= p_end) continue;
        if (GIVEN || QUAD) {
            const float t = prior_term<GIVEN, QUAD>(m[j], given[j], target[j], w);
            mout[p] = prior_elem<true, false>(m[j], dm[j], t, 0.f, 0.f, step);
        } else
            mout[p] = prior_elem<false, false>(m[j], dm[j], 0.f, 0.f, 0.f, step);
    }
}

// One workgroup of NW waves per (tile of SC_TILE_PIX pixels, scene); the sums, the modes and the PRIOR rules are those
// of k_obs_contract (multiobs.h), the partials those of engine.h with P = n_partials(K, C) -- the Gram slots of K <= 32
// are left to the Gram pass.  Absent components are neither read nor written.
template <int CW, int NW, bool PRIOR>
__global__ __launch_bounds__(NW * SC_WAVE) void k_obs_contract_wide(ObsArgs a)
{
    constexpr int NT = NW * SC_WAVE, J = CW > 16 ? 2 : 4;
    const int s = blockIdx.y, tile = blockIdx.x;
    if (!a.active[s]) return;
    extern __shared__ __align__(16) double obsw_lds[];
    __shared__ double lred[NW];
    __shared__ int ch_n[CW];                                       // observations that cover channel c ...
    __shared__ unsigned char ch_o[CW][SC_MAX_OBS];                 // ... in ascending order
    const int K = a.K, C = a.C, HW = a.HW, W = a.W, n = scene_ncomp(a.ncomp, s, K);
    float *sed_s = (float *)obsw_lds;                              // [K][CW], zero beyond C and n (rows 16-byte aligned)
    double *red = (double *)(sed_s + (size_t)K * CW);              // [NW][K][C]
    const int c0 = a.cur[s];
    for (int i = threadIdx.x; i < K * CW; i += NT) {
        const int k = i / CW, c = i % CW;
        sed_s[i] = (k < n && c < C) ? a.sed[c0][((size_t)s * K + k) * C + c] : 0.f;
    }
    for (int i = threadIdx.x; i < NW * K * C; i += NT) red[i] = 0.0;
    if (threadIdx.x < CW) {
        const int c = threadIdx.x;
        int cnt = 0;
        for (int o = 0; o < a.n_obs; ++o) {
            const int b = c - a.obs[o].band0;
            if (c < C && b >= 0 && b < a.obs[o].B) ch_o[c][cnt++] = (unsigned char)o;
        }
        ch_n[c] = cnt;
    }
    __syncthreads();
    const int mode = a.mode;
    const float step_morph = mode == OBS_PARTIALS ? 0.f : 1.0f / (float)(a.lipschitz[2 * s + 1] * (double)a.n_obs);
    const double L_morph = PRIOR ? a.lipschitz[2 * s + 1] * (double)a.n_obs : 0.0;    // (the scene's, before the prior's)
    const float *mor = a.morph[c0] + (size_t)s * K * HW;
    float *mout = a.morph[1 - c0] + (size_t)s * K * HW;
    const int lane = threadIdx.x & (SC_WAVE - 1), wid = threadIdx.x / SC_WAVE;
    double loss = 0;
    const int p_end = min(HW, (tile + 1) * SC_TILE_PIX);
    for (int p0 = tile * SC_TILE_PIX; p0 < p_end; p0 += NT * J) {
        // gs first holds the model of the thread's J pixels (a SED row is read once for all of them), then their G
        float gs[J][CW];
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int c = 0; c < CW; ++c) gs[j][c] = 0.f;
        for (int k = 0; k < n; ++k) {
            float m[J];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int p = p0 + j * NT + threadIdx.x;
                m[j] = p < p_end ? mor[(size_t)k * HW + p] : 0.f;
            }
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                const float sk = sed_s[k * CW + c];
#pragma unroll
                for (int j = 0; j < J; ++j) gs[j][c] += sk * m[j];
            }
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int p = p0 + j * NT + threadIdx.x;
            const bool in = p < p_end;
            const int y = p / W, x = p - y * W;
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                const int nc = __builtin_amdgcn_readfirstlane(ch_n[c]);
                float g = 0.f;
                for (int i = 0; i < nc; ++i) {
                    const ObsView &v = a.obs[__builtin_amdgcn_readfirstlane((int)ch_o[c][i])];
                    const size_t plane = (size_t)s * v.B + (c - v.band0);
                    if (!in) continue;
                    if (v.G) {
                        g += v.G[(plane * v.Fy + pos_mod(y + v.oy, v.Fy)) * v.Fx + pos_mod(x + v.ox, v.Fx)];
                    } else {
                        const float w = v.weights ? v.weights[plane * HW + p] : v.weight_scalar;
                        const float d = w * (gs[j][c] - v.images[plane * HW + p]);
                        loss += (double)d * (double)d;
                        g += w * d;
                    }
                }
                gs[j][c] = g;
            }
        }
        for (int k = 0; k < n; ++k) {
            const bool fixm = a.fix_morph && a.fix_morph[(size_t)s * K + k];
            float acc[CW];
            float mj[PRIOR ? J : 1], dmj[PRIOR ? J : 1], gvj[PRIOR ? J : 1], tgj[PRIOR ? J : 1];
            // PRIOR: the component's own constant and the streams of its prior (k_obs_contract's rules: a fixed
            // morphology, a weight of 0 or a missing plane reads none of them)
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
            for (int c = 0; c < CW; ++c) acc[c] = 0.f;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int p = p0 + j * NT + threadIdx.x;
                if (p >= p_end) continue;
                const float m = mor[(size_t)k * HW + p];
                if (PRIOR) { gvj[j] = gg ? gg[p] : 0.f; tgj[j] = tt ? tt[p] : 0.f; }
                float dm = 0.f;
#pragma unroll
                for (int c = 0; c < CW; ++c) { dm += sed_s[k * CW + c] * gs[j][c]; acc[c] += m * gs[j][c]; }
                if (PRIOR) { mj[j] = m; dmj[j] = dm; }
                else if (mode != OBS_PARTIALS) mout[(size_t)k * HW + p] = fixm ? m : m - step_morph * dm;
            }
            if (PRIOR) {
                float *mo = mout + (size_t)k * HW;
                const bool quad = w != 0.f, given = gg != nullptr;
                if (fixm) {
#pragma unroll
                    for (int j = 0; j < J; ++j) {
                        const int p = p0 + j * NT + threadIdx.x;
                        if (p < p_end) mo[p] = mj[j];
                    }
                }
                else if (given && quad) obs_prior_store_wide<J, NT, true, true>(mo, mj, dmj, gvj, tgj, w, step, p0, p_end);
                else if (given) obs_prior_store_wide<J, NT, true, false>(mo, mj, dmj, gvj, tgj, w, step, p0, p_end);
                else if (quad) obs_prior_store_wide<J, NT, false, true>(mo, mj, dmj, gvj, tgj, w, step, p0, p_end);
                else obs_prior_store_wide<J, NT, false, false>(mo, mj, dmj, gvj, tgj, w, step, p0, p_end);
            }
            if (mode != OBS_STEP) {
                const double r = wave_reduce_scatter<CW>(acc, lane);
                const int c = lane / (SC_WAVE / CW);
                if (lane % (SC_WAVE / CW) == 0 && c < C) red[((size_t)wid * K + k) * C + c] += r;   // (each wave owns its slots)
            }
        }
    }
    if (mode == OBS_STEP) return;
    const int P = n_partials(K, C);
    double *out = a.partials + ((size_t)s * a.T + tile) * P;
    loss = wave_sum(0.5 * loss);
    if (lane == 0) lred[wid] = loss;
    __syncthreads();                                               // (also orders the `red` updates)
    if (threadIdx.x == 0) {
        double l = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) l += lred[w];
        if (tile == 0)                                             // the losses of the observations with a PSF
            for (int o = 0; o < a.n_obs; ++o)
                if (a.obs[o].G)
                    for (int b = 0; b < a.obs[o].B; ++b) l += a.obs[o].loss_part[(size_t)s * a.obs[o].B + b];
        out[0] = l;
    }
    for (int i = threadIdx.x; i < n * C; i += NT) {
        double r = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) r += red[(size_t)w * K * C + i];
        out[1 + i] = r;
    }
}
