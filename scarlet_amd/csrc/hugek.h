// hugek.h -- the gradient step of Blend.fit for CROWDED scenes (SC_KBIG < K <= SC_KHUGE components per scene).
//
// bigk.h keeps the packed K x K Gram matrix in the per-tile partial sums and finds its largest eigenvalue in LDS, both
// sized for K <= 32: at K = 256 on a 1024 x 1024 frame the partials alone would be 33 k doubles per tile.  Above 32 the
// partials hold the loss and d loss / d sed only (engine.h n_partials), and the Gram matrix has its own area:
//
//   k_bigk_resid<SC_KHUGE> grid (T, S)              model, residual, loss -> G planes              (bigk.h)  [a1-a5]
//   k_huge_gram            grid (C, pairs, S)       S S^T on the matrix cores in float64: one 32 x 32 block of
//                                                   component pairs over one of C <= 16 pixel chunks        [a6]
//   k_huge_gram_reduce     grid (pairs, S)          sum over the chunks -> the full Gram G [S][Kp][Kp]       [a6]
//   k_huge_square x 32     grid (nb, nb, S)         M <- (M / tr M)^2, one 32 x 32 output block each         [a6]
//   k_huge_lipschitz       grid (S)                 Rayleigh quotient of the heaviest column of M with G,
//                                                   loss record (or trace of G with approximate_L)          [a6]
//   k_bigk_lmorph<SC_KHUGE> grid (S)                lambda_max(A^T A)                               (bigk.h)  [a6]
//   k_bigk_step<BM>        grid (T, K / 8, S)       d loss / d sed partials and the morphology step (bigk.h)  [a5, a7]
//   k_bigk_sed             grid (S)                 SED step                                        (bigk.h)  [a7]
//
// Kp = 32 nb, nb = ceil(K / 32): rows and columns K .. Kp - 1 of G are zero, which adds zero eigenvalues only.
// The Gram products m_i m_j of two float32 values are exact in float64 and v_mfma_f64_16x16x4_f64 accumulates them in
// float64, so G is the float64 Gram of the float32 morphologies up to float64 rounding.
#pragma once
#include "common.h"
#include "engine.h"

#define SC_KHUGE 256              // SCARLET_MAX_COMPONENTS
#define SC_GBLK 32                // component block of the Gram matrix
#define SC_GCHUNK_PIX 16384       // pixels per Gram workgroup (before the cap on the number of chunks)
#define SC_GCHUNK_MAX 16
#define SC_HUGE_SQUARINGS 32      // lambda_max within K / (e 2^33) relative (< 1.2e-8 at K = 256), whatever the gaps

__host__ __device__ inline int huge_nblk(int K) { return (K + SC_GBLK - 1) / SC_GBLK; }
__host__ __device__ inline int huge_npairs(int K) { const int n = huge_nblk(K); return n * (n + 1) / 2; }
__host__ __device__ inline int huge_nchunks(int HW)
{
    const int c = (HW + SC_GCHUNK_PIX - 1) / SC_GCHUNK_PIX;
    return c < SC_GCHUNK_MAX ? c : SC_GCHUNK_MAX;
}
// pixels per chunk: a multiple of 4 waves x 32 pixels
__host__ __device__ inline int huge_chunk_pix(int HW)
{
    const int c = huge_nchunks(HW), per = (HW + c - 1) / c;
    return (per + 127) & ~127;
}

struct HugeArgs {
    double *gpart;                // [S][pairs][C][32][32]  per-chunk Gram blocks
    double *gram;                 // [S][Kp][Kp]            G
    double *msq[2];               // [S][Kp][Kp]            the squared matrices (ping-pong)
    int C;
};

// pair index -> (bi, bj), bi <= bj, in the order (0,0) (0,1) .. (0,nb-1) (1,1) ..
__device__ inline void huge_pair(int pair, int nb, int &bi, int &bj)
{
    bi = 0;
    while (pair >= nb - bi) { pair -= nb - bi; ++bi; }
    bj = bi + pair;
}

// ---- the Gram blocks on the matrix cores.  A wave takes 32 consecutive pixels per trip; lane l (row r = l & 15, slot
// q = l >> 4) holds pixels 8 q .. 8 q + 7 of components 32 bi + r, 32 bi + 16 + r (A operands) and 32 bj + r,
// 32 bj + 16 + r (B operands).  In the e-th MFMA of a trip slot q supplies pixel 8 q + e, the same pixel in A and B, so
// the four 16 x 16 x 4 products sum m_i m_j over the trip's pixels.  C layout (f64): column lane & 15, row
// (lane >> 4) + 4 reg.  VEC: HW % 4 == 0 (16-byte loads).
typedef double huge_f64x4 __attribute__((ext_vector_type(4)));
template <bool VEC>
__global__ __launch_bounds__(SC_BLOCK) void k_huge_gram(GradArgs a, HugeArgs h)
{
    const int s = blockIdx.z, pair = blockIdx.y, chunk = blockIdx.x;
    if (!a.active[s]) return;
    const int K = a.K, HW = a.HW, nb = huge_nblk(K);
    int bi, bj;
    huge_pair(pair, nb, bi, bj);
    // ragged batch: a pair with an absent block (bj >= bi) is not formed; its readers stop at the present blocks
    if (bj * SC_GBLK >= scene_ncomp(a.ncomp, s, K)) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const float *mor = a.morph[a.cur[s]] + (size_t)s * K * HW;
    const int k0 = bi * SC_GBLK + r, k1 = k0 + 16, k2 = bj * SC_GBLK + r, k3 = k2 + 16;
    const float *m0 = mor + (size_t)(k0 < K ? k0 : 0) * HW, *m1 = mor + (size_t)(k1 < K ? k1 : 0) * HW;
    const float *m2 = mor + (size_t)(k2 < K ? k2 : 0) * HW, *m3 = mor + (size_t)(k3 < K ? k3 : 0) * HW;
    const bool v0 = k0 < K, v1 = k1 < K, v2 = k2 < K, v3 = k3 < K;
    const int per = huge_chunk_pix(HW), p_begin = chunk * per, p_end = min(HW, p_begin + per);
    huge_f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = huge_f64x4{0.0, 0.0, 0.0, 0.0};
    auto load8 = [&](const float *m, bool valid, int p, float (&x)[8]) {
        if (VEC) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float4 f = (valid && p + 4 * u < p_end) ? *reinterpret_cast<const float4 *>(m + p + 4 * u)
                                                              : make_float4(0.f, 0.f, 0.f, 0.f);
                x[4 * u] = f.x; x[4 * u + 1] = f.y; x[4 * u + 2] = f.z; x[4 * u + 3] = f.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = (valid && p + e < p_end) ? m[p + e] : 0.f;
        }
    };
#pragma unroll 1
    for (int p0 = p_begin + wid * 32; p0 < p_end; p0 += SC_NWAVES * 32) {
        const int p = p0 + 8 * q;
        float x0[8], x1[8], x2[8], x3[8];
        load8(m0, v0, p, x0); load8(m1, v1, p, x1);
        if (bi != bj) { load8(m2, v2, p, x2); load8(m3, v3, p, x3); }
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) { x2[e] = x0[e]; x3[e] = x1[e]; }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const double a0 = x0[e], a1 = x1[e], b0 = x2[e], b1 = x3[e];
            acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[3], 0, 0, 0);
        }
    }
    // four waves -> one 32 x 32 block; sub-tile t = 2 ii + jj holds rows 16 ii + .., columns 16 jj + ..
    __shared__ double red[SC_NWAVES][SC_GBLK * SC_GBLK];               // 32 KB
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int row = 16 * (t >> 1) + q + 4 * g, col = 16 * (t & 1) + r;
            red[wid][row * SC_GBLK + col] = acc[t][g];
        }
    __syncthreads();
    double *out = h.gpart + (((size_t)s * huge_npairs(K) + pair) * h.C + chunk) * (SC_GBLK * SC_GBLK);
    for (int e = threadIdx.x; e < SC_GBLK * SC_GBLK; e += SC_BLOCK) {
        double v = 0;
#pragma unroll
        for (int w = 0; w < SC_NWAVES; ++w) v += red[w][e];
        out[e] = v;
    }
}

// ---- sum over the pixel chunks; both triangles of G (a diagonal block is mirrored from its upper triangle, so G is
// exactly symmetric)
__global__ __launch_bounds__(SC_BLOCK) void k_huge_gram_reduce(GradArgs a, HugeArgs h)
{
    const int s = blockIdx.y, pair = blockIdx.x;
    if (!a.active[s]) return;
    const int nb = huge_nblk(a.K), Kp = nb * SC_GBLK;
    int bi, bj;
    huge_pair(pair, nb, bi, bj);
    if (bj * SC_GBLK >= scene_ncomp(a.ncomp, s, a.K)) return;           // (not formed by k_huge_gram: not read)
    const double *in = h.gpart + ((size_t)s * huge_npairs(a.K) + pair) * h.C * (SC_GBLK * SC_GBLK);
    double *G = h.gram + (size_t)s * Kp * Kp;
    for (int e = threadIdx.x; e < SC_GBLK * SC_GBLK; e += SC_BLOCK) {
        const int il = e / SC_GBLK, jl = e % SC_GBLK;
        if (bi == bj && il > jl) continue;
        double v = 0;
        for (int c = 0; c < h.C; ++c) v += in[(size_t)c * SC_GBLK * SC_GBLK + e];
        const int i = bi * SC_GBLK + il, j = bj * SC_GBLK + jl;
        G[(size_t)i * Kp + j] = v;
        G[(size_t)j * Kp + i] = v;
    }
}

// ---- one squaring: dst = (src / tr src)^2 for the 32 x 32 output block (blockIdx.y, blockIdx.x).  src is symmetric,
// so the B operand is read by rows as well.  Every workgroup sums the trace in the same order.  The scaled matrix has
// its eigenvalues in [0, 1] and the largest >= 1 / K: no overflow, no underflow.
__global__ __launch_bounds__(SC_BLOCK) void k_huge_square(GradArgs a, const double *src_all, double *dst_all)
{
    const int s = blockIdx.z, bi = blockIdx.y, bj = blockIdx.x;
    if (!a.active[s]) return;
    const int Kp = huge_nblk(a.K) * SC_GBLK;
    // ragged batch: only the blocks of present components (Kn = 32 ceil(n / 32)) are squared and read; the rest of G and
    // of the squares is neither written nor read in this call (absent components add zero rows and columns only)
    const int n = scene_ncomp(a.ncomp, s, a.K), Kn = huge_nblk(n) * SC_GBLK;
    if (bi * SC_GBLK >= n || bj * SC_GBLK >= n) return;
    const double *src = src_all + (size_t)s * Kp * Kp;
    double *dst = dst_all + (size_t)s * Kp * Kp;
    __shared__ double As[SC_GBLK][SC_GBLK + 1], Bs[SC_GBLK][SC_GBLK + 1];
    __shared__ double red[SC_NWAVES];
    const int tid = threadIdx.x;
    double tr = 0;
    for (int i = tid; i < Kn; i += SC_BLOCK) tr += src[(size_t)i * Kp + i];
    tr = block_sum(tr, red);
    const double sc = 1.0 / (tr * tr);
    const int ti = (tid >> 4) * 2, tj = (tid & 15) * 2;
    double c00 = 0, c01 = 0, c10 = 0, c11 = 0;
    for (int k0 = 0; k0 < Kn; k0 += SC_GBLK) {
        for (int e = tid; e < SC_GBLK * SC_GBLK; e += SC_BLOCK) {
            const int x = e / SC_GBLK, y = e % SC_GBLK;
            As[x][y] = src[(size_t)(bi * SC_GBLK + x) * Kp + k0 + y];            // A[row][k]
            Bs[x][y] = src[(size_t)(k0 + x) * Kp + bj * SC_GBLK + y];            // B[k][col]
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < SC_GBLK; ++k) {
            const double u0 = As[ti][k], u1 = As[ti + 1][k], w0 = Bs[k][tj], w1 = Bs[k][tj + 1];
            c00 += u0 * w0; c01 += u0 * w1; c10 += u1 * w0; c11 += u1 * w1;
        }
        __syncthreads();
    }
    double *o = dst + (size_t)(bi * SC_GBLK + ti) * Kp + bj * SC_GBLK + tj;
    o[0] = c00 * sc; o[1] = c01 * sc; o[Kp] = c10 * sc; o[Kp + 1] = c11 * sc;
}

// ---- L_sed: Rayleigh quotient with G of the heaviest column of the last power (as k_bigk_lipschitz), or the trace of G
// with approximate_L (doubled when the loss rose, blend.py:186-203); the loss record of the iteration.
// lambda_max(A^T A) comes from k_bigk_lmorph.
__global__ __launch_bounds__(SC_BLOCK) void k_huge_lipschitz(GradArgs a, HugeArgs h, const double *msq_all)
{
    const int s = blockIdx.x;
    if (!a.active[s]) return;
    const int B = a.B, P = n_partials(a.K, B), Kp = huge_nblk(a.K) * SC_GBLK, tid = threadIdx.x;
    const int K = scene_ncomp(a.ncomp, s, a.K);        // ragged batch: the present components' rows of G and M only
    const double *G = h.gram + (size_t)s * Kp * Kp;
    __shared__ double red[SC_NWAVES];
    __shared__ double vcol[SC_KHUGE];
    __shared__ double bestv[SC_NWAVES];
    __shared__ int besti[SC_NWAVES];
    double loss = 0;
    if (tid == 0) for (int t = 0; t < a.T; ++t) loss += a.partials[((size_t)s * a.T + t) * P];
    double trace = 0;
    for (int i = tid; i < K; i += SC_BLOCK) trace += G[(size_t)i * Kp + i];
    trace = block_sum(trace, red);
    const int it_new = a.it[s] + 1;
    double L_sed;
    if (a.approximate_L) {
        __shared__ double loss_s;
        if (tid == 0) loss_s = loss;
        __syncthreads();
        L_sed = (it_new > 1 && loss_s > a.mse[(size_t)s * a.mse_capacity + it_new - 2]) ? 2 * trace : trace;
    } else {
        const double *M = msq_all + (size_t)s * Kp * Kp;
        // heaviest column: largest diagonal entry, lowest index on ties
        double best = -1.0;
        int bidx = 0;
        for (int i = tid; i < K; i += SC_BLOCK) {
            const double d = M[(size_t)i * Kp + i];
            if (d > best) { best = d; bidx = i; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double b2 = __shfl_xor(best, o, SC_WAVE);
            const int i2 = __shfl_xor(bidx, o, SC_WAVE);
            if (b2 > best || (b2 == best && i2 < bidx)) { best = b2; bidx = i2; }
        }
        if ((tid & 63) == 0) { bestv[tid >> 6] = best; besti[tid >> 6] = bidx; }
        __syncthreads();
        best = bestv[0]; bidx = besti[0];
        for (int w = 1; w < SC_NWAVES; ++w)
            if (bestv[w] > best || (bestv[w] == best && besti[w] < bidx)) { best = bestv[w]; bidx = besti[w]; }
        for (int i = tid; i < K; i += SC_BLOCK) vcol[i] = M[(size_t)i * Kp + bidx];
        __syncthreads();
        double num = 0, den = 0;
        for (int i = tid; i < K; i += SC_BLOCK) {
            double gv = 0;
            for (int j = 0; j < K; ++j) gv += G[(size_t)j * Kp + i] * vcol[j];     // (G symmetric: column reads)
            num += vcol[i] * gv; den += vcol[i] * vcol[i];
        }
        num = block_sum(num, red);
        den = block_sum(den, red);
        L_sed = num / den;
    }
    if (tid == 0) {
        if (it_new <= a.mse_capacity) a.mse[(size_t)s * a.mse_capacity + it_new - 1] = loss;
        a.lipschitz[2 * s] = L_sed;
    }
}
