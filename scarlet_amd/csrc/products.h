// products.h -- read-only evaluation of a batch's state (scarlet_batch_products): the model sum_k sed[k][b] morph[k],
// the model as the data sees it (Observation.render), the residual, the per-band loss and the component fluxes.
//
// Without a difference kernel ONE pass (k_products) does everything: a workgroup owns PR_TILE_PIX pixels of a scene, a
// thread four of them; it walks the scene's present morphology planes once with 16-byte loads, keeps one float4
// accumulator per band (ascending k, FMA, the SEDs as wave-uniform scalars), then reads image and weight once and
// writes model / rendered / residual once.  Losses (and, with FLUX, the plane sums) leave the workgroup as float64
// partials [S][T][.]; k_products_reduce adds the tiles in ascending order: no atomics, so loss and flux are
// bit-identical from run to run.  With a difference kernel the same pass writes only the unconvolved planes; the
// LDS-resident transform (k_products_conv: the passes of fftconv.h on the batch's prepared K-hat) or the hipFFT chain
// followed by k_products_finish renders them and takes residual and loss.
// Nothing here reads `active` or `status`, and nothing writes to the batch.
#pragma once
#include "common.h"
#include "engine.h"
#include "hugek.h"
#include "psf_path.h"
#include "fftconv.h"

#define PR_TILE_PIX 1024        // pixels per (scene, tile) workgroup: one float4 per thread

struct ProdArgs {
    int S, K, B, HW, T;              // B: bands of this evaluation; T: tiles per scene
    int C, band0;                    // the SEDs are [S][K][C]; the B bands start at channel band0
    const float *sed[2], *morph[2];
    const int *cur, *ncomp;
    const float *images, *weights;   // [S][B][HW]; images may be NULL when neither residual nor loss is wanted
    float weight_scalar;
    float *model;                    // [S - model_s0][model_C][HW] or NULL: the B planes go to model_b0 .. model_b0 + B - 1
    int model_C, model_b0;           // (B, 0 but for a state of more than 8 channels, evaluated in chunks of bands)
    float *rendered, *residual;      // [S][B][HW] or NULL
    int s0, model_s0;                // first scene of the launch; scene that `model` starts at (staged chunks)
    double *loss_part;               // [S][T][B] or NULL
    double *flux_part;               // [S][T][K] or NULL
};

// four consecutive pixels of a plane from pixel p0 on; pixels beyond the plane read as zero
template <bool VEC4>
__device__ __forceinline__ float4 pr_load4(const float *plane, int p0, int HW)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (VEC4) {
        if (p0 < HW) v = *reinterpret_cast<const float4 *>(plane + p0);
    } else {
        if (p0 < HW) v.x = plane[p0];
        if (p0 + 1 < HW) v.y = plane[p0 + 1];
        if (p0 + 2 < HW) v.z = plane[p0 + 2];
        if (p0 + 3 < HW) v.w = plane[p0 + 3];
    }
    return v;
}
template <bool VEC4>
__device__ __forceinline__ void pr_store4(float *plane, int p0, int HW, float4 v)
{
    if (VEC4) {
        if (p0 < HW) *reinterpret_cast<float4 *>(plane + p0) = v;
    } else {
        if (p0 < HW) plane[p0] = v.x;
        if (p0 + 1 < HW) plane[p0 + 1] = v.y;
        if (p0 + 2 < HW) plane[p0 + 2] = v.z;
        if (p0 + 3 < HW) plane[p0 + 3] = v.w;
    }
}
__device__ __forceinline__ float pr_uniform(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
// the squared weighted residual of pixel j of a group, zero for a pixel beyond the plane (its factors may be NaN)
__device__ __forceinline__ double pr_sq(float w, float r, float img, bool valid)
{
    const float d = w * (r - img);
    return valid ? (double)d * (double)d : 0.0;
}

// VEC4: 16-byte accesses (H W % 4 == 0 and every plane pointer 16-byte aligned); FLUX: also the plane sums of the
// morphologies, one wave reduction per component inside the pass.  grid (T, scenes of the launch).
template <bool VEC4, bool FLUX>
__global__ __launch_bounds__(SC_BLOCK) void k_products(ProdArgs a)
{
    const int s = a.s0 + blockIdx.y, tile = blockIdx.x;
    const int K = a.K, B = a.B, HW = a.HW;
    const int n = scene_ncomp(a.ncomp, s, K), c0 = a.cur[s] & 1;
    __shared__ __align__(16) float sed_s[SC_KHUGE * SC_BMAX];
    __shared__ double red_l[SC_NWAVES][SC_BMAX];
    __shared__ double red_f[SC_NWAVES][FLUX ? SC_KHUGE : 1];
    for (int i = threadIdx.x; i < n * B; i += SC_BLOCK) {
        const int k = i / B, b = i - k * B;
        sed_s[k * SC_BMAX + b] = a.sed[c0][((size_t)s * K + k) * a.C + a.band0 + b];
    }
    __syncthreads();
    const int lane = threadIdx.x & (SC_WAVE - 1), wid = threadIdx.x / SC_WAVE;
    const int p0 = tile * PR_TILE_PIX + threadIdx.x * 4;
    float4 acc[SC_BMAX];
#pragma unroll
    for (int b = 0; b < SC_BMAX; ++b) acc[b] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float *mor = a.morph[c0] + (size_t)s * K * HW;
#pragma unroll 4
    for (int k = 0; k < n; ++k) {
        const float4 m = pr_load4<VEC4>(mor + (size_t)k * HW, p0, HW);
        // (the row of SEDs in two 16-byte LDS reads; entries b >= B were never written and are not used)
        const float4 slo = *reinterpret_cast<const float4 *>(&sed_s[k * SC_BMAX]), shi = *reinterpret_cast<const float4 *>(&sed_s[k * SC_BMAX + 4]);
        const float srow[SC_BMAX] = {slo.x, slo.y, slo.z, slo.w, shi.x, shi.y, shi.z, shi.w};
#pragma unroll
        for (int b = 0; b < SC_BMAX; ++b)
            if (b < B) {
                const float sk = pr_uniform(srow[b]);
                acc[b].x = fmaf(sk, m.x, acc[b].x); acc[b].y = fmaf(sk, m.y, acc[b].y);
                acc[b].z = fmaf(sk, m.z, acc[b].z); acc[b].w = fmaf(sk, m.w, acc[b].w);
            }
        if (FLUX) {
            const double f = wave_sum(((double)m.x + (double)m.y) + ((double)m.z + (double)m.w));
            if (lane == 0) red_f[wid][k] = f;
        }
    }
    const bool observed = a.residual || a.loss_part;
#pragma unroll
    for (int b = 0; b < SC_BMAX; ++b)
        if (b < B) {
            const size_t plane = ((size_t)s * B + b) * HW;
            if (a.model) pr_store4<VEC4>(a.model + ((size_t)(s - a.model_s0) * a.model_C + a.model_b0 + b) * HW, p0, HW, acc[b]);
            if (a.rendered) pr_store4<VEC4>(a.rendered + plane, p0, HW, acc[b]);
            if (observed) {
                const float4 img = pr_load4<VEC4>(a.images + plane, p0, HW);
                const float ws = a.weight_scalar;
                const float4 w = a.weights ? pr_load4<VEC4>(a.weights + plane, p0, HW) : make_float4(ws, ws, ws, ws);
                if (a.residual)
                    pr_store4<VEC4>(a.residual + plane, p0, HW,
                                    make_float4(img.x - acc[b].x, img.y - acc[b].y, img.z - acc[b].z, img.w - acc[b].w));
                if (a.loss_part) {
                    double l = (pr_sq(w.x, acc[b].x, img.x, p0 < HW) + pr_sq(w.y, acc[b].y, img.y, p0 + 1 < HW)) +
                               (pr_sq(w.z, acc[b].z, img.z, p0 + 2 < HW) + pr_sq(w.w, acc[b].w, img.w, p0 + 3 < HW));
                    l = wave_sum(l);
                    if (lane == 0) red_l[wid][b] = l;
                }
            }
        }
    __syncthreads();
    const size_t st = (size_t)s * a.T + tile;
    if (a.loss_part && threadIdx.x < B) {
        double r = 0;
#pragma unroll
        for (int w = 0; w < SC_NWAVES; ++w) r += red_l[w][threadIdx.x];
        a.loss_part[st * B + threadIdx.x] = r;
    }
    if (FLUX)
        for (int k = threadIdx.x; k < K; k += SC_BLOCK) {
            double r = 0;
            if (k < n) {
#pragma unroll
                for (int w = 0; w < SC_NWAVES; ++w) r += red_f[w][k];
            }
            a.flux_part[st * K + k] = r;
        }
}

// one workgroup per scene: the tiles' partials in ascending order -> loss [S][B] and flux [S][K][B] (either may be NULL)
__global__ __launch_bounds__(SC_BLOCK) void k_products_reduce(ProdArgs a, double *loss, double *flux)
{
    const int s = blockIdx.x, K = a.K, B = a.B, T = a.T;
    __shared__ double tot[SC_KHUGE];
    if (loss && threadIdx.x < B) {
        double r = 0;
        for (int t = 0; t < T; ++t) r += a.loss_part[((size_t)s * T + t) * B + threadIdx.x];
        loss[(size_t)s * B + threadIdx.x] = 0.5 * r;
    }
    if (!flux) return;
    for (int k = threadIdx.x; k < K; k += SC_BLOCK) {
        double r = 0;
        for (int t = 0; t < T; ++t) r += a.flux_part[((size_t)s * T + t) * K + k];
        tot[k] = r;
    }
    __syncthreads();
    const int n = scene_ncomp(a.ncomp, s, K), c0 = a.cur[s] & 1;
    for (int i = threadIdx.x; i < K * B; i += SC_BLOCK) {
        const int k = i / B, b = i - k * B;
        flux[(size_t)s * K * B + i] = k < n ? tot[k] * (double)a.sed[c0][((size_t)s * K + k) * a.C + a.band0 + b] : 0.0;
    }
}

// Component.get_model of the selected components: out [S][n][B][HW] = sed[k][b] morph[k]; absent components: zeros.
// grid (T * sel.n, S)
struct ProdSelection { int n; int k[SC_KHUGE]; };
template <bool VEC4>
__global__ __launch_bounds__(SC_BLOCK) void k_products_components(ProdArgs a, ProdSelection sel, float *out)
{
    const int s = blockIdx.y, j = blockIdx.x / a.T, tile = blockIdx.x - j * a.T;
    const int K = a.K, B = a.B, HW = a.HW, k = sel.k[j];
    const int n = scene_ncomp(a.ncomp, s, K), c0 = a.cur[s] & 1;
    const int p0 = tile * PR_TILE_PIX + threadIdx.x * 4;
    const bool present = k < n;
    const float4 m = present ? pr_load4<VEC4>(a.morph[c0] + ((size_t)s * K + k) * HW, p0, HW) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float *sed = a.sed[c0] + ((size_t)s * K + k) * a.C + a.band0;
    for (int b = 0; b < B; ++b) {
        const float sk = present ? sed[b] : 0.f;
        pr_store4<VEC4>(out + (((size_t)s * sel.n + j) * B + b) * HW, p0, HW, make_float4(sk * m.x, sk * m.y, sk * m.z, sk * m.w));
    }
}

// ---- with a difference kernel
struct ProdObsArgs {
    int B, HW, T;
    int plane0;                      // first (scene, band) plane of the launch
    const float *images, *weights;   // [S][B][HW]
    float weight_scalar;
    float *rendered, *residual;      // [S][B][HW] or NULL
    double *loss;                    // k_products_conv: [S][B] or NULL
    double *loss_part;               // k_products_finish: [S][T][B] or NULL
    const int *frame_hw;             // scarlet_batch::frame_hw; read by the RAGGED instantiations only
};
// Ragged frames: pixel (y, x) of plane `plane` lies outside its scene's own frame, where the convolution spills: rendered
// and residual are written as zero there and the pixel adds nothing to the loss.  (The entries are only compared with.)
__device__ __forceinline__ bool pr_outside(const ProdObsArgs &a, size_t plane, int pix, int y, int x)
{
    const size_t s = plane / a.B;
    if (y < a.frame_hw[2 * s] && x < a.frame_hw[2 * s + 1]) return false;
    const size_t i = plane * a.HW + pix;
    if (a.rendered) a.rendered[i] = 0.f;
    if (a.residual) a.residual[i] = 0.f;
    return true;
}
// rendered value r of pixel `pix` of plane `plane`: the outputs it feeds; returns its squared weighted residual
__device__ __forceinline__ double pr_observe(const ProdObsArgs &a, size_t plane, int pix, float r)
{
    const size_t i = plane * a.HW + pix;
    if (a.rendered) a.rendered[i] = r;
    if (!a.images) return 0.0;
    const float img = a.images[i];
    if (a.residual) a.residual[i] = img - r;
    return pr_sq(a.weights ? a.weights[i] : a.weight_scalar, r, img, true);
}

// The LDS-resident transform (fftconv.h) on compact planes in [n][H][W]: one workgroup per plane renders it with the
// batch's prepared K-hat (khat [B] or [S * B] planes of Fy x (M + 1)) and feeds rendered / residual / loss from LDS.
template <bool RAGGED = false>
__global__ __launch_bounds__(SC_FFT_NT) void k_products_conv(ProdObsArgs a, const float *in, FftPlan p, const float2 *khat,
                                                             int khat_per_scene)
{
    extern __shared__ __align__(16) float2 fft_lds[];
    __shared__ double red[SC_FFT_NT / SC_WAVE];
    const FftLds l = fft_lds_setup(fft_lds, p);
    const int H = p.H, W = p.W, M = p.M, Wh = (W + 1) / 2;
    const size_t plane = (size_t)a.plane0 + blockIdx.x;
    const float *ip = in + (size_t)blockIdx.x * H * W;
    for (int u = threadIdx.x; u < p.Fy * p.RS; u += SC_FFT_NT) {
        const int y = u / p.RS, n = u - y * p.RS;
        cf v = cf_zero();
        if (y < H && n < Wh) {
            v.x = ip[y * W + 2 * n];
            if (2 * n + 1 < W) v.y = ip[y * W + 2 * n + 1];
        }
        l.A[u] = v;
    }
    __syncthreads();
    fft2d_fwd(l, p, H);
    fft_spec_mul<false>(l, p, khat + (khat_per_scene ? plane : plane % a.B) * p.Fy * (M + 1));
    fft2d_inv(l, p, H);
    double loss = 0;
    for (int u = threadIdx.x; u < H * W; u += SC_FFT_NT) {
        const int y = u / W, x = u - y * W;
        const cf v = l.A[y * p.RS + (x >> 1)];
        if (RAGGED && pr_outside(a, plane, u, y, x)) continue;
        loss += pr_observe(a, plane, u, (x & 1) ? v.y : v.x);
    }
    if (!a.loss) return;
    loss = wave_sum(loss);
    if ((threadIdx.x & (SC_WAVE - 1)) == 0) red[threadIdx.x / SC_WAVE] = loss;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = 0;
        for (int w = 0; w < SC_FFT_NT / SC_WAVE; ++w) r += red[w];
        a.loss[plane] = 0.5 * r;
    }
}

// After the hipFFT chain: the rendered planes lie padded in real [n][g.Fy][g.Fx].  grid (planes of the launch, T)
template <bool RAGGED = false>
__global__ __launch_bounds__(SC_BLOCK) void k_products_finish(ProdObsArgs a, const float *real, PsfGeom g)
{
    __shared__ double red[SC_NWAVES];
    const size_t plane = (size_t)a.plane0 + blockIdx.x;
    const int tile = blockIdx.y;
    const float *rp = real + (size_t)blockIdx.x * g.Fy * g.Fx;
    const int p_end = min(a.HW, (tile + 1) * PR_TILE_PIX);
    double loss = 0;
    for (int pix = tile * PR_TILE_PIX + threadIdx.x; pix < p_end; pix += SC_BLOCK) {
        const int y = pix / g.W, x = pix - y * g.W;
        if (RAGGED && pr_outside(a, plane, pix, y, x)) continue;
        loss += pr_observe(a, plane, pix, rp[(size_t)pos_mod(y + g.oy, g.Fy) * g.Fx + pos_mod(x + g.ox, g.Fx)]);
    }
    if (!a.loss_part) return;
    loss = block_sum(loss, red);
    if (threadIdx.x == 0) a.loss_part[((plane / a.B) * a.T + tile) * a.B + plane % a.B] = loss;
}
