// lowres_stream.h -- the STREAMED form of the low-resolution operator of lowres.h, for model frames whose factor
// matrices do not fit LDS (up to SCARLET_MAX_SIDE a side).  The operator is the same sandwich,
//
//     out_c = Re( Vy . ( Dhat_c o (Uy . model_c . Ux^T) ) . Vx^T )      G_c = Re( Uy^T . ( Dhat_c o (Vy^T . (w d) . Vx) ) . Ux )
//
// on the same stacked real operands ((Re | Im) factors; [[Re, -Im], [-Im, -Re]] for what an elementwise pass produces)
// with the same k-ordered float32 sums, but nothing stays resident: every product is ONE launch of a batched GEMM over
// all planes of a chunk (k_lrs_gemm, grid = (output tiles, planes)), the intermediates lie in a scratch area in HBM and
// small elementwise kernels run between the GEMMs:
//
//   fit     model_c = sum_k sed[k][band0 + c] m_k  (k_lrs_model: the B band models, not the K components)
//   render  T = m Ux^T | C = Uy T | Z = expand(C o Dhat_c) (k_lrs_expand) | R = Z Vx^T | out = Vy R
//   fit     d = w (out - image), E = w d, loss partial sums (k_lrs_resid), loss_c = 1/2 sum d^2 (k_lrs_loss)
//   adjoint A1 = Vy^T E | C2 = A1 Vx | Z2 = expand(C2 o Dhat_c) | G1 = Z2 Ux | G = Uy^T G1
//   products (read-only): model_c (or the caller's `model` output) | render | rendered, residual = image - out, loss
//           partial sums (k_lrs_products_finish, which leaves `out` as it is) | k_lrs_loss
//
// The factor matrices are read where the caller put them, as (re, im) pairs: an operand that is a stacked factor names
// the index along which it is stacked (LrsOperand::stack) and the loader turns an index >= n into the imaginary part of
// index - n.  The plane -> (band, scene) map selects dhat and, with v_per_scene, vy / vx; planes of inactive scenes
// return at once in every kernel, so nothing of theirs is written (the products pass no `active`: every scene runs).
#pragma once
#include "lowres.h"

#define LRS_BM 32                    // output tile of one workgroup: 32 x 64, each of the 4 waves two 16 x 16 MFMA tiles
#define LRS_BN 64
#define LRS_BK 16                    // K-step staged through LDS
#define LRS_LDA (LRS_BM + 16)        // rows of the k-major LDS tiles: 16 (mod 32) floats, so that the lanes (l & 15, l >> 4)
#define LRS_LDB (LRS_BN + 16)        //   of one ds_read_b32 lane group fall on 32 different banks
#define LRS_LOSS_BLOCKS 64           // partial sums per plane of the loss (fixed: the sum's order does not depend on the launch)

// which plane of the caller a plane of the chunk is, and its band and scene.  B > 0 (a fit): plane p is band p % B of
// scene p / B; B == 0 (the plane operators): band[p] and scene[p], NULL = 0.  active: NULL, or the state's flags.
struct LrsPlanes {
    const int *band, *scene, *active;
    int B, p0;
};
__device__ __forceinline__ bool lrs_plane(const LrsPlanes &pl, int local, int &band, int &scene)
{
    const int p = pl.p0 + local;
    if (pl.B > 0) { scene = p / pl.B; band = p - scene * pl.B; }
    else { band = pl.band ? pl.band[p] : 0; scene = pl.scene ? pl.scene[p] : 0; }
    return !pl.active || pl.active[scene] != 0;
}

// a GEMM operand: element (i, j) = p[i * rs + j * cs] (+ plane / scene offsets).  stack = 1 / 2: p holds (re, im) pairs
// (rs, cs count floats) and the operand is (Re | Im) stacked along its first / second index, 2 n long there.
struct LrsOperand {
    const float *p;
    int rs, cs, stack, n;
    size_t plane, scene;             // floats added per plane of the chunk / per scene of the plane
};
__device__ __forceinline__ float lrs_load(const float *p, const LrsOperand &o, int i, int j)
{
    int im = 0;
    if (o.stack == 1 && i >= o.n) { i -= o.n; im = 1; }
    if (o.stack == 2 && j >= o.n) { j -= o.n; im = 1; }
    return p[(size_t)i * o.rs + (size_t)j * o.cs + im];
}

// C[plane] [M][N] (row-major, leading dimension ldc) = A [M][K] . B [K][N]
struct LrsGemm {
    LrsOperand a, b;
    float *c;
    int ldc;
    size_t c_plane;
    int M, N, K;
    LrsPlanes pl;
};

// Operands outside the matrices are staged as zeros (ragged edges need no second path; K is summed to the next multiple
// of LRS_BK in both forms).  MFMA: v_mfma_f32_16x16x4_f32, an exact f32 FMA chain in k order, two independent
// accumulators per wave (the instruction's dependent latency is 40 cycles against a 32-cycle issue).  !MFMA (the
// NO_LOWRES_MFMA switch): the same sums from the same LDS tiles as plain fmaf chains, bit-identical.
template <bool MFMA>
__global__ __launch_bounds__(SC_BLOCK) void k_lrs_gemm(LrsGemm g)
{
    int band, scene;
    if (!lrs_plane(g.pl, blockIdx.y, band, scene)) return;
    __shared__ float As[LRS_BK * LRS_LDA], Bs[LRS_BK * LRS_LDB];
    const int tn = (g.N + LRS_BN - 1) / LRS_BN;
    const int i0 = (blockIdx.x / tn) * LRS_BM, j0 = (blockIdx.x % tn) * LRS_BN;
    const float *A = g.a.p + (size_t)blockIdx.y * g.a.plane + (size_t)scene * g.a.scene;
    const float *B = g.b.p + (size_t)blockIdx.y * g.b.plane + (size_t)scene * g.b.scene;
    float *C = g.c + (size_t)blockIdx.y * g.c_plane;
    const int t = threadIdx.x, M = g.M, N = g.N, K = g.K;
    // staging: the index with the smaller stride runs fastest across the threads
    const bool a_kfast = g.a.cs <= g.a.rs, b_kfast = g.b.rs <= g.b.cs;
    const int lane = t & (SC_WAVE - 1), wid = t / SC_WAVE, lr = lane & 15, lq = lane >> 4;
    const int wi = (wid & 1) * 16, wj = (wid >> 1) * 32;           // the wave's 16 x 32 part of the tile (MFMA)
    const int fi = t >> 3, fj = t & 7;                             // row and first column of the thread's 8 outputs (FMA)
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    float facc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += LRS_BK) {
        for (int e = t; e < LRS_BM * LRS_BK; e += SC_BLOCK) {
            const int i = a_kfast ? e / LRS_BK : e % LRS_BM, k = a_kfast ? e % LRS_BK : e / LRS_BM;
            As[k * LRS_LDA + i] = (i0 + i < M && k0 + k < K) ? lrs_load(A, g.a, i0 + i, k0 + k) : 0.f;
        }
        for (int e = t; e < LRS_BK * LRS_BN; e += SC_BLOCK) {
            const int j = b_kfast ? e / LRS_BK : e % LRS_BN, k = b_kfast ? e % LRS_BK : e / LRS_BN;
            Bs[k * LRS_LDB + j] = (j0 + j < N && k0 + k < K) ? lrs_load(B, g.b, k0 + k, j0 + j) : 0.f;
        }
        __syncthreads();
        if (MFMA) {
#pragma unroll
            for (int kk = 0; kk < LRS_BK; kk += 4) {
                const float a = As[(kk + lq) * LRS_LDA + wi + lr];
                const float b0 = Bs[(kk + lq) * LRS_LDB + wj + lr], b1 = Bs[(kk + lq) * LRS_LDB + wj + 16 + lr];
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc1, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int k = 0; k < LRS_BK; ++k) {
                const float a = As[k * LRS_LDA + fi];
#pragma unroll
                for (int c = 0; c < 8; ++c) facc[c] = fmaf(a, Bs[k * LRS_LDB + fj + 8 * c], facc[c]);
            }
        }
        __syncthreads();
    }
    if (MFMA) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + wi + lq * 4 + r, j = j0 + wj + lr;
            if (i < M && j < N) C[(size_t)i * g.ldc + j] = acc0[r];
            if (i < M && j + 16 < N) C[(size_t)i * g.ldc + j + 16] = acc1[r];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int i = i0 + fi, j = j0 + fj + 8 * c;
            if (i < M && j < N) C[(size_t)i * g.ldc + j] = facc[c];
        }
    }
}

// the band models of a fit: out[plane] [H W] = sum_k sed[k][band0 + band] morph[k] over the scene's present components,
// a float32 FMA chain in k order; absent components are not read
struct LrsModel {
    const float *sed[2], *morph[2];
    const int *cur, *ncomp;
    int K, C, band0, HW;
    float *out;
    size_t plane;
    LrsPlanes pl;
};
__global__ __launch_bounds__(SC_BLOCK) void k_lrs_model(LrsModel a)
{
    int band, s;
    if (!lrs_plane(a.pl, blockIdx.y, band, s)) return;
    const int n = scene_ncomp(a.ncomp, s, a.K), c0 = a.cur[s];
    const float *sed = a.sed[c0] + (size_t)s * a.K * a.C + a.band0 + band;
    const float *morph = a.morph[c0] + (size_t)s * a.K * a.HW;
    float *out = a.out + (size_t)blockIdx.y * a.plane;
    for (int e = blockIdx.x * SC_BLOCK + threadIdx.x; e < a.HW; e += gridDim.x * SC_BLOCK) {
        float acc = 0.f;
        for (int k = 0; k < n; ++k) acc = fmaf(sed[(size_t)k * a.C], morph[(size_t)k * a.HW + e], acc);
        out[e] = acc;
    }
}

// z[plane] = the four real blocks c[plane] [2 nfy][2 nfx] of a projection read as a complex spectrum, times Dhat of the
// plane's band, written as [[Re, -Im], [-Im, -Re]] (lr_projected, lr_expand of lowres.h)
struct LrsExpand {
    const float *c;
    float *z;
    size_t plane;
    int nfy, nfx, B;
    LowresFactors f;
    LrsPlanes pl;
};
__global__ __launch_bounds__(SC_BLOCK) void k_lrs_expand(LrsExpand a)
{
    int band, s;
    if (!lrs_plane(a.pl, blockIdx.y, band, s)) return;
    const int nf = a.nfy * a.nfx, ld = 2 * a.nfx, e = blockIdx.x * SC_BLOCK + threadIdx.x;
    if (e >= nf) return;
    const int f = e / a.nfx, g = e - f * a.nfx;
    const float *C = a.c + (size_t)blockIdx.y * a.plane;
    float *Z = a.z + (size_t)blockIdx.y * a.plane;
    const float2 x = lr_projected(C, ld, a.nfy, a.nfx, f, g);
    const float2 b = a.f.dhat[((size_t)(a.f.dhat_per_scene ? s * a.B : 0) + band) * nf + e];
    const float re = x.x * b.x - x.y * b.y, im = x.x * b.y + x.y * b.x;
    Z[f * ld + g] = re; Z[f * ld + a.nfx + g] = -im;
    Z[(a.nfy + f) * ld + g] = -im; Z[(a.nfy + f) * ld + a.nfx + g] = -re;
}

// the residual of a fit, in place: out[plane] [h w] -> w^2 (out - image), and LRS_LOSS_BLOCKS float64 partial sums of
// d^2 = (w (out - image))^2 per plane.  Block b sums the elements b * 256 + t + i * 64 * 256 whatever the launch, and
// k_lrs_loss adds the blocks' sums in order: no atomics, the same bits every time.
struct LrsResid {
    float *out;
    size_t plane;
    const float *images, *weights;          // [planes of the caller][h w]; weights NULL -> weight_scalar
    float weight_scalar;
    int hw;
    double *partials;                       // [planes of the chunk][LRS_LOSS_BLOCKS]
    double *loss_part;                      // [planes of the caller]
    LrsPlanes pl;
};
__global__ __launch_bounds__(SC_BLOCK) void k_lrs_resid(LrsResid a)
{
    int band, s;
    if (!lrs_plane(a.pl, blockIdx.y, band, s)) return;
    __shared__ double lred[SC_NWAVES];
    const size_t p = (size_t)(a.pl.p0 + blockIdx.y);
    float *out = a.out + (size_t)blockIdx.y * a.plane;
    const float *img = a.images + p * a.hw, *wgt = a.weights ? a.weights + p * a.hw : nullptr;
    double loss = 0;
    for (int e = blockIdx.x * SC_BLOCK + threadIdx.x; e < a.hw; e += LRS_LOSS_BLOCKS * SC_BLOCK) {
        const float w = wgt ? wgt[e] : a.weight_scalar;
        const float r = w * (out[e] - img[e]);
        loss += (double)r * (double)r;
        out[e] = w * r;
    }
    loss = block_sum(loss, lred);
    if (threadIdx.x == 0) a.partials[(size_t)blockIdx.y * LRS_LOSS_BLOCKS + blockIdx.x] = loss;
}
__global__ __launch_bounds__(SC_BLOCK) void k_lrs_loss(LrsResid a, int planes)
{
    const int local = blockIdx.x * SC_BLOCK + threadIdx.x;
    int band, s;
    if (local >= planes || !lrs_plane(a.pl, local, band, s)) return;
    const double *part = a.partials + (size_t)local * LRS_LOSS_BLOCKS;
    double loss = 0;
    for (int b = 0; b < LRS_LOSS_BLOCKS; ++b) loss += part[b];
    a.loss_part[a.pl.p0 + local] = 0.5 * loss;
}

// the finish of the read-only products (scarlet_observations_products_lowres): out[plane] [h w], the rendered image of
// the chain, is only read -- rendered, residual = image - out (each where given) and, with `partials`, the sums of
// k_lrs_resid in its order (block b: the elements b * 256 + t + i * 64 * 256), which k_lrs_loss adds.  Every plane is
// evaluated: pl.active is NULL.
struct LrsFinish {
    const float *out;
    size_t plane;
    const float *images, *weights;          // [planes of the caller][h w]; images NULL: rendered alone
    float weight_scalar;
    int hw;
    float *rendered, *residual;             // [planes of the caller][h w] or NULL
    double *partials;                       // [planes of the chunk][LRS_LOSS_BLOCKS] or NULL
    int p0;
};
__global__ __launch_bounds__(SC_BLOCK) void k_lrs_products_finish(LrsFinish a)
{
    __shared__ double lred[SC_NWAVES];
    const size_t p = (size_t)(a.p0 + blockIdx.y) * a.hw;
    const float *out = a.out + (size_t)blockIdx.y * a.plane;
    const float *img = a.images ? a.images + p : nullptr, *wgt = a.weights ? a.weights + p : nullptr;
    double loss = 0;
    for (int e = blockIdx.x * SC_BLOCK + threadIdx.x; e < a.hw; e += LRS_LOSS_BLOCKS * SC_BLOCK) {
        const float r = out[e];
        if (a.rendered) a.rendered[p + e] = r;
        if (!img) continue;
        const float v = img[e];
        if (a.residual) a.residual[p + e] = v - r;
        const float dw = (wgt ? wgt[e] : a.weight_scalar) * (r - v);
        loss += (double)dw * (double)dw;
    }
    if (!a.partials) return;
    loss = block_sum(loss, lred);
    if (threadIdx.x == 0) a.partials[(size_t)blockIdx.y * LRS_LOSS_BLOCKS + blockIdx.x] = loss;
}

// ---- the scratch of one chunk, floats per plane (host): M (the band model of a fit), A (T, R, A1, G1), B and Z (the
// projections and their expansions), D (the rendered image and its residual of a fit), and the loss partials after them
struct LrsScratch {
    size_t m, a, b, d;               // floats per plane of each buffer (m, d = 0 for the plane operators)
    size_t per_plane;                // bytes per plane, partial sums included
};
inline LrsScratch lrs_scratch(const LowresDims &d, bool fit)
{
    LrsScratch s;
    const size_t ny2 = 2 * (size_t)d.nfy, nx2 = 2 * (size_t)d.nfx;
    s.a = (size_t)d.H * nx2;
    if (ny2 * d.W > s.a) s.a = ny2 * d.W;
    if (ny2 * d.w > s.a) s.a = ny2 * d.w;
    s.b = ny2 * nx2;
    s.m = fit ? (size_t)d.H * d.W : 0;
    s.d = fit ? (size_t)d.h * d.w : 0;
    s.per_plane = (s.m + s.a + 2 * s.b + s.d) * sizeof(float) + (fit ? LRS_LOSS_BLOCKS * sizeof(double) : 0);
    s.per_plane = (s.per_plane + 15) & ~(size_t)15;
    return s;
}
// ... of the read-only products: the buffers of a fit (M for the band models, D for the rendered image that the finish
// reads, the loss partials).  One layout whatever the call wants, so that its size is a function of the shape alone; a
// call that finds the band models in the caller's `model` output leaves M unused.
inline LrsScratch lrs_products_scratch(const LowresDims &d) { return lrs_scratch(d, true); }
// Planes per chunk: as many as LRS_SCRATCH_CAP bytes of scratch hold, at least one, at most all
#define LRS_SCRATCH_CAP ((size_t)256 << 20)
inline int lrs_chunk(const LrsScratch &s, int planes)
{
    size_t c = LRS_SCRATCH_CAP / s.per_plane;
    if (c < 1) c = 1;
    return c < (size_t)planes ? (int)c : planes;
}
