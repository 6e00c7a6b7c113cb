// lowres.h -- a LOW-RESOLUTION observation of the model frame (reference LowResObservation, observation.py:242-599) as
// one more producer of the per-observation gradient planes that multiobs.h contracts (ObsView::G, loss_part).
//
// For frames that are not rotated against each other the reference's resample-and-convolve operator, restricted to the
// frequencies its sinc cut keeps, is a sandwich of five small complex matrices (scarlet_amd/resampling.py builds them):
//
//     out_c = Re( Vy . ( Dhat_c o (Uy . model_c . Ux^T) ) . Vx^T )            Uy [nfy][H]   Ux [nfx][W]
//     G_c   = Re( Uy^T . ( Dhat_c o (Vy^T . (w d) . Vx) ) . Ux )              Vy [h][nfy]   Vx [w][nfx]   Dhat [B][nfy][nfx]
//
// k_lowres_planes, one workgroup per scene:
//   1. every present component's morphology is read once and projected, P_k = Uy m_k Ux^T (linear in m), and added to
//      the spectra of the B bands with the component's SEDs: spec_c += sed[k][band0 + c] P_k  (LDS, [B][2][nfy][nfx]);
//   2. per band: spectrum x Dhat_c, out_c through Vx and Vy, the low-resolution image and weights streamed once,
//      d = w (out - image), loss_c = 1/2 sum d^2 (float64 sum), the adjoint of w d back through Vy, Vx, Dhat_c, Ux, Uy,
//      written as G[s][c][H][W] -- an ObsView with Fy = H, Fx = W, oy = ox = 0.
//
// Complex products run as REAL GEMMs on stacked operands: a complex matrix Z that an elementwise pass produces is
// written as the block matrix [[Re Z, -Im Z], [-Im Z, -Re Z]], so that one real GEMM with a stacked factor (Re | Im)
// yields [Re; -Im] of the product, which is what the next real GEMM with a stacked factor consumes.  Every GEMM is
// lr_gemm: v_mfma_f32_16x16x4_f32 (an exact f32 FMA chain in k order) on 16 x 16 output tiles, the waves taking tiles
// in turn; operands outside the matrices are read as zero, so ragged edges need no second code path.  The
// NO_LOWRES_MFMA switch runs the same sums as plain FMA chains (bit-identical; diagnostics).
// All factor matrices and intermediates stay in LDS; leading dimensions are odd so that the 16 lanes that walk a column
// fall on different banks.  This is the LDS-RESIDENT form, up to 64 x 64 model frames at 8 bands (84 x 84 at 2); beyond,
// the *_large entry points run the STREAMED form of lowres_stream.h: the same sums as batched GEMMs through HBM scratch.
#pragma once
#include "common.h"
#include <type_traits>

struct LowresDims {
    int H, W, h, w, nfy, nfx, B;
};

__host__ __device__ inline int lr_odd(int n) { return n | 1; }

// LDS layout (floats), shared by host (size check) and device
struct LowresLds {
    int ldH, ldW, ldw, ldVy, ldVx, ld2x;       // leading dimensions
    int uy, ux, vy, vx, spec, x, p, total;     // offsets; `p` holds tile + tp while projecting and buffer Y afterwards
    int tp;                                    // offset of tp inside the p region
    int sz;                                    // floats of one scratch buffer (X, Y)
};

__host__ __device__ inline LowresLds lowres_lds(const LowresDims &d)
{
    LowresLds l;
    const int ny2 = 2 * d.nfy, nx2 = 2 * d.nfx;
    l.ldH = lr_odd(d.H); l.ldW = lr_odd(d.W); l.ldw = lr_odd(d.w); l.ldVy = lr_odd(ny2); l.ldVx = lr_odd(nx2); l.ld2x = lr_odd(nx2);
    int sz = ny2 * l.ld2x;
    if (ny2 * l.ldw > sz) sz = ny2 * l.ldw;
    if (d.h * l.ldw > sz) sz = d.h * l.ldw;
    if (ny2 * l.ldW > sz) sz = ny2 * l.ldW;
    l.sz = sz;
    int o = 0;
    l.uy = o; o += ny2 * l.ldH;
    l.ux = o; o += nx2 * l.ldW;
    l.vy = o; o += d.h * l.ldVy;
    l.vx = o; o += d.w * l.ldVx;
    l.spec = o; o += d.B * 2 * d.nfy * d.nfx;
    l.x = o; o += sz;
    l.p = o;
    l.tp = d.H * l.ldW;
    const int proj = d.H * l.ldW + d.H * l.ld2x;
    o += proj > sz ? proj : sz;
    l.total = o;
    return l;
}
__host__ __device__ inline size_t lowres_lds_bytes(const LowresDims &d) { return (size_t)lowres_lds(d).total * sizeof(float); }

struct LowresFactors {
    const float2 *uy, *ux, *vy, *vx, *dhat;
    int v_per_scene, dhat_per_scene;
};

// C[M][N] = A[M][K] . B[K][N]; A(i, k) = A[i * a_rs + k * a_cs], B(k, j) = B[k * b_rs + j * b_cs]; store(i, j, value) once
// per element.  The caller synchronises the workgroup before (operands complete) and after (result complete).
template <typename Store>
__device__ __forceinline__ void lr_gemm(const float *A, int a_rs, int a_cs, const float *B, int b_rs, int b_cs, int M, int N,
                                        int K, bool mfma, Store store)
{
    if (mfma) {
        const int lane = threadIdx.x & (SC_WAVE - 1), wid = threadIdx.x / SC_WAVE;
        const int lr = lane & 15, lq = lane >> 4;
        const int tn = (N + 15) >> 4, tiles = ((M + 15) >> 4) * tn;
        for (int t = wid; t < tiles; t += SC_NWAVES) {
            const int i0 = (t / tn) << 4, j0 = (t % tn) << 4;
            const int ai = i0 + lr, bj = j0 + lr;
            const bool a_ok = ai < M, b_ok = bj < N;
            const float *ap = A + ai * a_rs, *bp = B + bj * b_cs;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < K; k0 += 4) {
                const int k = k0 + lq;
                const float a = (a_ok && k < K) ? ap[k * a_cs] : 0.f;
                const float b = (b_ok && k < K) ? bp[k * b_rs] : 0.f;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + lq * 4 + r;
                if (i < M && bj < N) store(i, bj, acc[r]);
            }
        }
    } else
        for (int e = threadIdx.x; e < M * N; e += SC_BLOCK) {
            const int i = e / N, j = e - i * N;
            float acc = 0.f;
            for (int k = 0; k < K; ++k) acc = fmaf(A[i * a_rs + k * a_cs], B[k * b_rs + j * b_cs], acc);
            store(i, j, acc);
        }
}

// the four factor matrices into LDS as stacked real matrices: uy [2 nfy][ldH] and ux [2 nfx][ldW] (rows: Re, then Im),
// vy [h][ldVy] and vx [w][ldVx] (columns: Re, then Im).  `p` holds the shape of the global tables: d itself, or (RAGGED,
// below) the maxima that every scene's own tables are zero-padded to, with uy and ux per scene like vy and vx.
template <bool RAGGED = false>
__device__ inline void lr_load_factors(float *lds, const LowresLds &l, const LowresDims &d, const LowresDims &p,
                                       const LowresFactors &f, int scene)
{
    const float2 *uy = RAGGED ? f.uy + (size_t)scene * p.nfy * p.H : f.uy;
    const float2 *ux = RAGGED ? f.ux + (size_t)scene * p.nfx * p.W : f.ux;
    const float2 *vy = f.vy + (f.v_per_scene ? (size_t)scene * p.h * p.nfy : 0);
    const float2 *vx = f.vx + (f.v_per_scene ? (size_t)scene * p.w * p.nfx : 0);
    for (int e = threadIdx.x; e < d.nfy * d.H; e += SC_BLOCK) {
        const int r = e / d.H, c = e - r * d.H;
        const float2 v = uy[RAGGED ? r * p.H + c : e];
        lds[l.uy + r * l.ldH + c] = v.x; lds[l.uy + (d.nfy + r) * l.ldH + c] = v.y;
    }
    for (int e = threadIdx.x; e < d.nfx * d.W; e += SC_BLOCK) {
        const int r = e / d.W, c = e - r * d.W;
        const float2 v = ux[RAGGED ? r * p.W + c : e];
        lds[l.ux + r * l.ldW + c] = v.x; lds[l.ux + (d.nfx + r) * l.ldW + c] = v.y;
    }
    for (int e = threadIdx.x; e < d.h * d.nfy; e += SC_BLOCK) {
        const int r = e / d.nfy, c = e - r * d.nfy;
        const float2 v = vy[RAGGED ? r * p.nfy + c : e];
        lds[l.vy + r * l.ldVy + c] = v.x; lds[l.vy + r * l.ldVy + d.nfy + c] = v.y;
    }
    for (int e = threadIdx.x; e < d.w * d.nfx; e += SC_BLOCK) {
        const int r = e / d.nfx, c = e - r * d.nfx;
        const float2 v = vx[RAGGED ? r * p.nfx + c : e];
        lds[l.vx + r * l.ldVx + c] = v.x; lds[l.vx + r * l.ldVx + d.nfx + c] = v.y;
    }
}

// one H x W plane (global, row stride W) -> the tile of the p region, then its projection Uy m Ux^T as the four real
// blocks C = [[Re Uy . Re T, Re Uy . Im T], [Im Uy . Re T, Im Uy . Im T]] (T = m Ux^T) in buffer X, [2 nfy][ld2x].
// Ends with the workgroup synchronised.
// (RAGGED changes nothing in the helpers that only take it along: the ragged-frames kernels get instances of their own,
// so that the compiler's inlining of the uniform kernels' instances does not depend on them)
template <bool RAGGED = false>
__device__ inline void lr_project_tile(float *lds, const LowresLds &l, const LowresDims &d, bool mfma);
template <bool RAGGED = false>
__device__ inline void lr_project(float *lds, const LowresLds &l, const LowresDims &d, const float *plane, bool mfma, int stride = 0)
{
    float *tile = lds + l.p;
    for (int e = threadIdx.x; e < d.H * d.W; e += SC_BLOCK) {
        const int y = e / d.W, x = e - y * d.W;
        tile[y * l.ldW + x] = plane[RAGGED ? y * stride + x : e];      // (RAGGED: the plane's rows are `stride` apart)
    }
    lr_project_tile<RAGGED>(lds, l, d, mfma);
}
// ... of the plane that the workgroup has written into the tile [H][ldW] of the p region itself (no barrier needed before)
template <bool RAGGED>
__device__ inline void lr_project_tile(float *lds, const LowresLds &l, const LowresDims &d, bool mfma)
{
    float *tile = lds + l.p, *tp = lds + l.p + l.tp, *C = lds + l.x;
    __syncthreads();
    const int ld2x = l.ld2x;
    // T [H][2 nfx] = m [H][W] . (Re Ux | Im Ux)^T
    lr_gemm(tile, l.ldW, 1, lds + l.ux, 1, l.ldW, d.H, 2 * d.nfx, d.W, mfma, [=](int i, int j, float v) { tp[i * ld2x + j] = v; });
    __syncthreads();
    // C [2 nfy][2 nfx] = (Re Uy; Im Uy) [2 nfy][H] . T
    lr_gemm(lds + l.uy, l.ldH, 1, tp, ld2x, 1, 2 * d.nfy, 2 * d.nfx, d.H, mfma, [=](int i, int j, float v) { C[i * ld2x + j] = v; });
    __syncthreads();
}

// complex (re, im) of the projection in buffer X at frequency (f, g)
__device__ __forceinline__ float2 lr_projected(const float *C, int ld2x, int nfy, int nfx, int f, int g)
{
    return make_float2(C[f * ld2x + g] - C[(nfy + f) * ld2x + nfx + g], C[f * ld2x + nfx + g] + C[(nfy + f) * ld2x + g]);
}

// A complex spectrum z(f, g) times Dhat, written into `dst` [2 nfy][ld2x] as [[Re, -Im], [-Im, -Re]]
// (RAGGED: the rows of dhat are `dld` apart, the nfx of the padded table)
template <bool RAGGED = false, typename Z>
__device__ __forceinline__ void lr_expand(float *dst, int ld2x, int nfy, int nfx, const float2 *dhat, Z z, int dld = 0)
{
    for (int e = threadIdx.x; e < nfy * nfx; e += SC_BLOCK) {
        const int f = e / nfx, g = e - f * nfx;
        const float2 a = z(f, g), b = dhat[RAGGED ? f * dld + g : e];
        const float re = a.x * b.x - a.y * b.y, im = a.x * b.y + a.y * b.x;
        dst[f * ld2x + g] = re; dst[f * ld2x + nfx + g] = -im;
        dst[(nfy + f) * ld2x + g] = -im; dst[(nfy + f) * ld2x + nfx + g] = -re;
    }
}

// forward of one band: the expanded spectrum in buffer X -> out [h][ldw] in buffer X (through buffer Y).  Ends synchronised.
template <bool RAGGED = false>
__device__ inline void lr_forward(float *lds, const LowresLds &l, const LowresDims &d, bool mfma)
{
    float *X = lds + l.x, *Y = lds + l.p;
    const int ldw = l.ldw;
    // R [2 nfy][w] = A [2 nfy][2 nfx] . (Re Vx | Im Vx)^T  = [Re R; -Im R]
    lr_gemm(X, l.ld2x, 1, lds + l.vx, 1, l.ldVx, 2 * d.nfy, d.w, 2 * d.nfx, mfma, [=](int i, int j, float v) { Y[i * ldw + j] = v; });
    __syncthreads();
    // out [h][w] = (Re Vy | Im Vy) [h][2 nfy] . R
    lr_gemm(lds + l.vy, l.ldVy, 1, Y, ldw, 1, d.h, d.w, 2 * d.nfy, mfma, [=](int i, int j, float v) { X[i * ldw + j] = v; });
    __syncthreads();
}

// adjoint of one band: E [h][ldw] in buffer X -> store(y, x, value) for the H x W plane.  Starts and ends synchronised.
template <bool RAGGED = false, typename Store>
__device__ inline void lr_adjoint(float *lds, const LowresLds &l, const LowresDims &d, const float2 *dhat, bool mfma, Store store,
                                  int dld = 0)
{
    float *X = lds + l.x, *Y = lds + l.p;
    const int ldw = l.ldw, ld2x = l.ld2x, ldW = l.ldW, nfy = d.nfy, nfx = d.nfx;
    // A1 [2 nfy][w] = (Re Vy | Im Vy)^T . E
    lr_gemm(lds + l.vy, 1, l.ldVy, X, ldw, 1, 2 * nfy, d.w, d.h, mfma, [=](int i, int j, float v) { Y[i * ldw + j] = v; });
    __syncthreads();
    // C2 [2 nfy][2 nfx] = A1 . (Re Vx | Im Vx): the four real blocks of A1 Vx
    lr_gemm(Y, ldw, 1, lds + l.vx, l.ldVx, 1, 2 * nfy, 2 * nfx, d.w, mfma, [=](int i, int j, float v) { X[i * ld2x + j] = v; });
    __syncthreads();
    lr_expand<RAGGED>(Y, ld2x, nfy, nfx, dhat, [=](int f, int g) { return lr_projected(X, ld2x, nfy, nfx, f, g); }, dld);
    __syncthreads();
    // G1 [2 nfy][W] = Z [2 nfy][2 nfx] . (Re Ux; Im Ux) = [Re G1; -Im G1]
    lr_gemm(Y, ld2x, 1, lds + l.ux, l.ldW, 1, 2 * nfy, d.W, 2 * nfx, mfma, [=](int i, int j, float v) { X[i * ldW + j] = v; });
    __syncthreads();
    // G [H][W] = (Re Uy; Im Uy)^T . G1
    lr_gemm(lds + l.uy, 1, l.ldH, X, ldW, 1, d.H, d.W, 2 * nfy, mfma, store);
    __syncthreads();
}

struct LowresArgs {
    LowresDims d;
    LowresFactors f;
    int S, K, C, band0;
    const float *sed[2], *morph[2];           // the STATE's factors: sed [S][K][C], morph [S][K][H][W]
    const int *cur, *active, *ncomp;
    const float *images, *weights;            // [S][B][h][w]; weights NULL -> weight_scalar
    float weight_scalar;
    float *G;                                 // [S][B][H][W]
    double *loss_part;                        // [S][B]
    int mfma;
};

// RAGGED FRAMES (scarlet_lowres_frames): every scene has its own H_s, W_s, h_s, w_s, nfy_s, nfx_s in its row of `dims`
// and its own five factor matrices, each zero-padded to the shape `d` of the arguments, which holds the per-dimension
// maxima over the scenes: the strides of every global array and the LDS layout are those of the maxima, the loops and
// the GEMM extents the scene's own.  frame_hw: the frames the constraint side runs on (scarlet_frames).
struct LowresFrames {
    const int *dims;                          // [S][6]
    const int *frame_hw;                      // [S][2]
};
// the scene's own shape inside the padded shape p.  False -- the caller touches nothing -- for a row outside 1..max in
// any column or one that disagrees with frame_hw (k_check_lowres_frames has marked that scene; the products run without
// `active`): no entry becomes a loop bound before this test.
__device__ __forceinline__ bool lr_scene_dims(const LowresFrames &r, int s, const LowresDims &p, LowresDims &d)
{
    const int *q = r.dims + 6 * (size_t)s;
    d.H = q[0]; d.W = q[1]; d.h = q[2]; d.w = q[3]; d.nfy = q[4]; d.nfx = q[5]; d.B = p.B;
    return d.H >= 1 && d.H <= p.H && d.W >= 1 && d.W <= p.W && d.h >= 1 && d.h <= p.h && d.w >= 1 && d.w <= p.w &&
           d.nfy >= 1 && d.nfy <= p.nfy && d.nfx >= 1 && d.nfx <= p.nfx &&
           r.frame_hw[2 * (size_t)s] == d.H && r.frame_hw[2 * (size_t)s + 1] == d.W;
}

// the arguments of the ragged-frames instance: a.d holds the maxima, a.f.uy / ux one table per scene, v and dhat are per scene
struct LowresFramesArgs : LowresArgs {
    LowresFrames fr;
};
// Args = LowresArgs: every scene has the shape a.d (k_lowres_planes); LowresFramesArgs: RAGGED (k_lowres_planes_frames)
template <typename Args>
__global__ __launch_bounds__(SC_BLOCK) void k_lowres_planes_t(Args a)
{
    constexpr bool RAGGED = std::is_same<Args, LowresFramesArgs>::value;
    const int s = blockIdx.x;
    if (!a.active[s]) return;
    extern __shared__ __align__(16) float lr_lds[];
    __shared__ double lred[SC_NWAVES];
    const LowresDims p = a.d;                  // the shape of the global arrays and of the LDS layout
    LowresDims d = a.d;                        // the shape the scene runs on
    if constexpr (RAGGED)
        if (!lr_scene_dims(a.fr, s, p, d)) return;
    const LowresLds l = lowres_lds(p);
    const bool mfma = a.mfma != 0;
    const int n = scene_ncomp(a.ncomp, s, a.K), c0 = a.cur[s], nf = d.nfy * d.nfx, HW = p.H * p.W, hw = p.h * p.w;
    const int nfp = p.nfy * p.nfx;
    float *spec = lr_lds + l.spec, *X = lr_lds + l.x;
    lr_load_factors<RAGGED>(lr_lds, l, d, p, a.f, s);
    for (int e = threadIdx.x; e < d.B * 2 * nf; e += SC_BLOCK) spec[e] = 0.f;
    const float *sed = a.sed[c0] + (size_t)s * a.K * a.C + a.band0;
    for (int k = 0; k < n; ++k) {
        lr_project<RAGGED>(lr_lds, l, d, a.morph[c0] + ((size_t)s * a.K + k) * HW, mfma, p.W);   // (its first barrier also covers the loads above)
        for (int e = threadIdx.x; e < nf; e += SC_BLOCK) {
            const float2 z = lr_projected(X, l.ld2x, d.nfy, d.nfx, e / d.nfx, e % d.nfx);
            for (int c = 0; c < d.B; ++c) {
                const float sc = sed[(size_t)k * a.C + c];
                spec[(c * 2) * nf + e] += sc * z.x;
                spec[(c * 2 + 1) * nf + e] += sc * z.y;
            }
        }
        __syncthreads();
    }
    if (n == 0) __syncthreads();
    for (int c = 0; c < d.B; ++c) {
        const float2 *dhat = a.f.dhat + ((size_t)(a.f.dhat_per_scene ? s * d.B : 0) + c) * nfp;
        const float *sre = spec + (c * 2) * nf, *sim = sre + nf;
        const int nfx = d.nfx;
        lr_expand<RAGGED>(X, l.ld2x, d.nfy, d.nfx, dhat, [=](int f, int g) { return make_float2(sre[f * nfx + g], sim[f * nfx + g]); },
                          p.nfx);
        __syncthreads();
        lr_forward<RAGGED>(lr_lds, l, d, mfma);
        const float *img = a.images + ((size_t)s * d.B + c) * hw;
        const float *wgt = a.weights ? a.weights + ((size_t)s * d.B + c) * hw : nullptr;
        double loss = 0;
        for (int e = threadIdx.x; e < d.h * d.w; e += SC_BLOCK) {
            const int i = e / d.w, j = e - i * d.w, ge = RAGGED ? i * p.w + j : e;
            const float w = wgt ? wgt[ge] : a.weight_scalar;
            const float r = w * (X[i * l.ldw + j] - img[ge]);
            loss += (double)r * (double)r;
            X[i * l.ldw + j] = w * r;
        }
        loss = block_sum(0.5 * loss, lred);                      // (its barriers also complete E)
        if (threadIdx.x == 0) a.loss_part[(size_t)s * d.B + c] = loss;
        float *G = a.G + ((size_t)s * d.B + c) * HW;
        const int W = p.W;
        if (RAGGED)        // the contraction reads the whole padded plane and the workspace is not zeroed: 0 outside the frame
            for (int e = threadIdx.x; e < HW; e += SC_BLOCK)
                if (e / W >= d.H || e % W >= d.W) G[e] = 0.f;
        lr_adjoint<RAGGED>(lr_lds, l, d, dhat, mfma, [=](int y, int x, float v) { G[y * W + x] = v; }, p.nfx);
    }
}
static constexpr auto k_lowres_planes = &k_lowres_planes_t<LowresArgs>;
static constexpr auto k_lowres_planes_frames = &k_lowres_planes_t<LowresFramesArgs>;

// The read-only products of a low-resolution observation (scarlet_observations_products_lowres): what the observation
// sees of the state, forward only.  One workgroup per scene -- every scene, whatever `active` and `status` say, from its
// own buffer cur[s] -- loads the factors once and, band by band, forms the band model sum_k sed[k][band0 + c] m_k (the
// float32 FMA chain in k order of k_products and k_lrs_model, absent components not read) straight in the tile of
// lr_project, projects it, multiplies by Dhat_c as k_lowres_render does (so the rendered planes are, bit for bit, that
// kernel's on the model planes), runs lr_forward, and reads the h x w result once for rendered, residual = image -
// rendered and loss_c = 1/2 sum (w (rendered - image))^2 (float64, block_sum: a fixed order).  Outputs that are NULL
// are not written; nothing of the state or of a workspace is.
struct LowresProductsArgs {
    LowresDims d;
    LowresFactors f;
    int K, C, band0;
    const float *sed[2], *morph[2];           // the STATE's factors: sed [S][K][C], morph [S][K][H][W]
    const int *cur, *ncomp;
    const float *images, *weights;            // [S][B][h][w]; images NULL: rendered alone; weights NULL -> weight_scalar
    float weight_scalar;
    float *rendered, *residual;               // [S][B][h][w] or NULL
    double *loss;                             // [S][B] or NULL
    int mfma;
};

// RAGGED (scarlet_observations_products_frames_lowres; LowresFrames above): the scene's own sizes bound every loop,
// rendered and residual are written over the whole padded h x w plane, 0 outside the scene's own pixels, and a scene
// whose `dims` row lr_scene_dims refuses gets zeros in all three.
struct LowresProductsFramesArgs : LowresProductsArgs {
    LowresFrames fr;
};
template <typename Args>
__global__ __launch_bounds__(SC_BLOCK) void k_lowres_products_t(Args a)
{
    constexpr bool RAGGED = std::is_same<Args, LowresProductsFramesArgs>::value;
    extern __shared__ __align__(16) float lr_lds[];
    __shared__ double lred[SC_NWAVES];
    const int s = blockIdx.x;
    const LowresDims p = a.d;                  // the shape of the global arrays and of the LDS layout
    LowresDims d = a.d;                        // the shape the scene runs on
    const int HW = p.H * p.W, hw = p.h * p.w;
    if constexpr (RAGGED) if (!lr_scene_dims(a.fr, s, p, d)) {
        for (int e = threadIdx.x; e < d.B * hw; e += SC_BLOCK) {
            if (a.rendered) a.rendered[(size_t)s * d.B * hw + e] = 0.f;
            if (a.residual) a.residual[(size_t)s * d.B * hw + e] = 0.f;
        }
        if (a.loss && threadIdx.x < d.B) a.loss[(size_t)s * d.B + threadIdx.x] = 0;
        return;
    }
    const LowresLds l = lowres_lds(p);
    const bool mfma = a.mfma != 0;
    const int n = scene_ncomp(a.ncomp, s, a.K), c0 = a.cur[s] & 1, nf = p.nfy * p.nfx;
    const int ld2x = l.ld2x, nfy = d.nfy, nfx = d.nfx;
    float *X = lr_lds + l.x, *Y = lr_lds + l.p, *tile = lr_lds + l.p;
    lr_load_factors<RAGGED>(lr_lds, l, d, p, a.f, s);
    const float *sed = a.sed[c0] + (size_t)s * a.K * a.C + a.band0;
    const float *morph = a.morph[c0] + (size_t)s * a.K * HW;
    for (int c = 0; c < d.B; ++c) {
        // (the band before no longer reads the p region: lr_forward ended synchronised; its epilogue reads X, which is
        // written again only behind lr_project_tile's barriers)
        for (int e = threadIdx.x; e < d.H * d.W; e += SC_BLOCK) {
            const int y = e / d.W, x = e % d.W, ge = RAGGED ? y * p.W + x : e;
            float acc = 0.f;
            for (int k = 0; k < n; ++k) acc = fmaf(sed[(size_t)k * a.C + c], morph[(size_t)k * HW + ge], acc);
            tile[y * l.ldW + x] = acc;
        }
        lr_project_tile<RAGGED>(lr_lds, l, d, mfma);               // (its first barrier also covers the factors)
        const float2 *dhat = a.f.dhat + ((size_t)(a.f.dhat_per_scene ? s * d.B : 0) + c) * nf;
        // (the projection sits in X, which lr_forward reads expanded: expand through Y)
        lr_expand<RAGGED>(Y, ld2x, nfy, nfx, dhat, [=](int f, int g) { return lr_projected(X, ld2x, nfy, nfx, f, g); }, p.nfx);
        __syncthreads();
        for (int e = threadIdx.x; e < 2 * nfy * ld2x; e += SC_BLOCK) X[e] = Y[e];
        __syncthreads();
        lr_forward<RAGGED>(lr_lds, l, d, mfma);
        const size_t plane = ((size_t)s * d.B + c) * hw;
        const float *img = a.images ? a.images + plane : nullptr;
        const float *wgt = a.weights ? a.weights + plane : nullptr;
        double loss = 0;
        for (int e = threadIdx.x; e < d.h * d.w; e += SC_BLOCK) {
            const int i = e / d.w, j = e % d.w, ge = RAGGED ? i * p.w + j : e;
            const float r = X[i * l.ldw + j];
            if (a.rendered) a.rendered[plane + ge] = r;
            if (!img) continue;
            const float v = img[ge];
            if (a.residual) a.residual[plane + ge] = v - r;
            const float dw = (wgt ? wgt[ge] : a.weight_scalar) * (r - v);
            loss += (double)dw * (double)dw;
        }
        if (RAGGED)
            for (int e = threadIdx.x; e < hw; e += SC_BLOCK) {
                if (e / p.w < d.h && e % p.w < d.w) continue;
                if (a.rendered) a.rendered[plane + e] = 0.f;
                if (a.residual && img) a.residual[plane + e] = 0.f;
            }
        if (a.loss) {
            loss = block_sum(loss, lred);
            if (threadIdx.x == 0) a.loss[(size_t)s * d.B + c] = 0.5 * loss;
        }
    }
}
static constexpr auto k_lowres_products = &k_lowres_products_t<LowresProductsArgs>;
static constexpr auto k_lowres_products_frames = &k_lowres_products_t<LowresProductsFramesArgs>;

// LowResObservation.render / its adjoint for n planes: plane p uses band[p] (NULL: 0) and the factors of scene[p] (NULL: 0)
struct LowresOpArgs {
    LowresDims d;
    LowresFactors f;
    const float *in;
    float *out;
    const int *band, *scene;
    int mfma;
};

__global__ __launch_bounds__(SC_BLOCK) void k_lowres_render(LowresOpArgs a)
{
    extern __shared__ __align__(16) float lr_lds[];
    const LowresDims d = a.d;
    const LowresLds l = lowres_lds(d);
    const int p = blockIdx.x, c = a.band ? a.band[p] : 0, s = a.scene ? a.scene[p] : 0, nf = d.nfy * d.nfx;
    float *X = lr_lds + l.x, *Y = lr_lds + l.p;
    lr_load_factors(lr_lds, l, d, d, a.f, s);
    lr_project(lr_lds, l, d, a.in + (size_t)p * d.H * d.W, a.mfma != 0);
    const float2 *dhat = a.f.dhat + ((size_t)(a.f.dhat_per_scene ? s * d.B : 0) + c) * nf;
    // (the projection sits in X, which lr_forward reads expanded: expand through Y)
    const int ld2x = l.ld2x, nfy = d.nfy, nfx = d.nfx;
    lr_expand(Y, ld2x, nfy, nfx, dhat, [=](int f, int g) { return lr_projected(X, ld2x, nfy, nfx, f, g); });
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * nfy * ld2x; e += SC_BLOCK) X[e] = Y[e];
    __syncthreads();
    lr_forward(lr_lds, l, d, a.mfma != 0);
    float *out = a.out + (size_t)p * d.h * d.w;
    for (int e = threadIdx.x; e < d.h * d.w; e += SC_BLOCK) out[e] = X[(e / d.w) * l.ldw + e % d.w];
}

__global__ __launch_bounds__(SC_BLOCK) void k_lowres_adjoint(LowresOpArgs a)
{
    extern __shared__ __align__(16) float lr_lds[];
    const LowresDims d = a.d;
    const LowresLds l = lowres_lds(d);
    const int p = blockIdx.x, c = a.band ? a.band[p] : 0, s = a.scene ? a.scene[p] : 0, nf = d.nfy * d.nfx;
    float *X = lr_lds + l.x;
    lr_load_factors(lr_lds, l, d, d, a.f, s);
    const float *in = a.in + (size_t)p * d.h * d.w;
    for (int e = threadIdx.x; e < d.h * d.w; e += SC_BLOCK) X[(e / d.w) * l.ldw + e % d.w] = in[e];
    __syncthreads();
    const float2 *dhat = a.f.dhat + ((size_t)(a.f.dhat_per_scene ? s * d.B : 0) + c) * nf;
    float *out = a.out + (size_t)p * d.H * d.W;
    const int W = d.W;
    lr_adjoint(lr_lds, l, d, dhat, a.mfma != 0, [=](int y, int x, float v) { out[y * W + x] = v; });
}
