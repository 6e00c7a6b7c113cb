// Source initialisation on the device: the detection tile shared by every extended start (source.py:139-180), and the
// kernels of scarlet_init_sources -- extended sources with per-scene noise and PSF peaks, point sources
// (source.py:340-400) and the layered components of a multi-component source (source.py:242-295).
#pragma once

// ---- the detection tile of one source at (cy, cx): SED-weighted coadd of the bands with a positive SED
// (build_detection_coadd, source.py:101-136), sdss symmetry (source.py:162), the thresh=.1 weighted monotone sweep
// (source.py:165-167).  The tile holds the float64 coadd afterwards; returns the sweep level past which nothing is
// kept (the sweep may stop once three levels hold nothing above the cutoff: the levels beyond cannot exceed it
// either) and the noise cutoff in `cutoff`.
// RAGGED: the tile is a scene's own frame in the top-left corner of image planes of PHW pixels with row stride PW.
template <bool GT, bool RAGGED = false>
__device__ __forceinline__ int init_detect_tile(TileT<double> &t, const float *img, int B, int cy, int cx,
                                                const float *sed_s, const double (&bg)[SC_BMAX], double thresh,
                                                int do_symmetric, int do_monotonic, int no_hybrid, double &cutoff,
                                                int PW = 0, int PHW = 0)
{
    const int H = t.H, W = t.W, HW = H * W;
    double wb[SC_BMAX], jac = 0, var = 0;
#pragma unroll
    for (int b = 0; b < SC_BMAX; ++b) {
        wb[b] = 0;
        if (b < B && sed_s[b] > 0.f) {
            const double sd = (double)sed_s[b], bgb = bg[b];
            wb[b] = sd / (bgb * bgb);
            jac += sd * sd / (bgb * bgb);
            var += wb[b] * wb[b] * bgb * bgb;
        }
    }
    cutoff = thresh * sqrt(var) / jac;
    for (int i = threadIdx.x; i < HW; i += SC_BLOCK) {
        double acc = 0;
#pragma unroll
        for (int b = 0; b < SC_BMAX; ++b)
            if (b < B && wb[b] != 0) acc += wb[b] * (double)img[RAGGED ? (size_t)b * PHW + (i / W) * PW + (i % W) : (size_t)b * HW + i];
        t.m[(i / W) * t.LW + (i % W)] = acc / jac;
    }
    __syncthreads();
    const SymWindow sw = sym_window(H, W, cy, cx);
    if (do_symmetric) flip_symmetry_tile<double>(t, sw, true, 1.0);
    __shared__ int lastpos_s;
    int lstop = 1 << 30;
    if (do_monotonic) {
        if (!GT && cutoff >= 0 && !no_hybrid) {
            // levels 1 .. 46 on one wave without barriers (wave_ops.h), the rest on the workgroup if needed
            __shared__ int hyb[2];
            if (threadIdx.x < SC_WAVE) {
                int done, quiet;
                wave_monotonic<double>(t, cy, cx, 0.1, &done, &quiet, cutoff);
                if (threadIdx.x == 0) { hyb[0] = done; hyb[1] = quiet; }
            }
            __syncthreads();
            lstop = hyb[0];
            if (lstop == (1 << 30))
                lstop = monotonic_tile<false, double>(t, cy, cx, 0.1, &lastpos_s, cutoff, SC_COMPACT_LAST + 1,
                                                      SC_COMPACT_LAST - hyb[1]);
        } else
            lstop = monotonic_tile<false, double>(t, cy, cx, 0.1, cutoff >= 0 ? &lastpos_s : nullptr, cutoff);
    }
    return lstop;
}

// pixel i survives the cut (source.py:170-175)
__device__ __forceinline__ bool init_kept(const TileT<double> &t, int i, int cy, int cx, double cutoff, int lstop)
{
    return t.m[(i / t.W) * t.LW + (i % t.W)] > cutoff && sweep_level(i / t.W, i % t.W, cy, cx) <= lstop;
}

// a component whose centre lies outside the frame (IndexError in the reference, ValueError in BlendBatch): empty
__device__ __forceinline__ void init_empty_outside(float *gm, float *gs, int HW, int B, int *flag, int *status)
{
    for (int i = threadIdx.x; i < HW; i += SC_BLOCK) gm[i] = 0.f;
    if (threadIdx.x < B) gs[threadIdx.x] = 0.f;
    if (threadIdx.x == 0) {
        *flag = SCARLET_FLAG_SED_NOT_CONVERGED | SCARLET_FLAG_MORPH_NOT_CONVERGED | SCARLET_FLAG_NO_VALID_PIXELS;
        atomicOr(status, SCARLET_STATUS_CENTER_AT_EDGE);
    }
}

// =====================================================================================
// scarlet_init_sources
struct InitSrcArgs {
    int S, K, B, H, W;
    const float *images;
    float *sed[2], *morph[2];
    const int *cur, *centers;
    int *flags, *status, *active;
    const int *ncomp_in;              // scarlet_batch::n_components (NULL: K)
    int *ncomp;                       // [S] what this call initialises: 0 for a scene with bad input
    const int *group, *kind;          // [S][K] or NULL
    const float *bg_rms;              // [B] (bg_stride 0) or [S][B] (bg_stride B)
    int bg_stride;
    const float *obs_peak;            // [B] / [S][B] or NULL
    int peak_stride;
    const float *model_psf;           // [P][P] or NULL
    int P;
    const float *perc;                // [S][K] or NULL (25)
    double thresh;
    int do_symmetric, do_monotonic, group_symmetric, no_hybrid;
    const int *frame_hw;              // scarlet_batch::frame_hw (NULL: every scene is H x W); read by the RAGGED instantiation
};

__device__ __forceinline__ int init_kind(const InitSrcArgs &a, int c)
{
    if (a.group && a.group[c] >= 0) return -1;
    return a.kind ? a.kind[c] : SCARLET_INIT_EXTENDED;
}

// One thread per scene: the checks of the input that need the device arrays.  A scene with bad input gets
// SCARLET_STATUS_BAD_INIT, active = 0 and a count of 0 (nothing of it is initialised or updated); the others lose
// the bit of an earlier call.
__global__ void k_init_check(InitSrcArgs a)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.S) return;
    const int K = a.K, n = scene_ncomp(a.ncomp_in, s, K);
    bool bad = false;
    for (int b = 0; b < a.B; ++b)
        if (!(a.bg_rms[(size_t)s * a.bg_stride + b] > 0.f)) bad = true;
    for (int k = 0; k < n; ++k) {
        const int c = s * K + k;
        const int g = a.group ? a.group[c] : -1;
        if (g < 0) {
            if (a.kind && a.kind[c] != SCARLET_INIT_EXTENDED && a.kind[c] != SCARLET_INIT_POINT) bad = true;
            continue;
        }
        if (k > 0 && a.group[c - 1] == g) continue;                 // not the first member
        int m = 1;
        while (k + m < n && a.group[c + m] == g) ++m;
        if (m > SCARLET_MAX_LAYERS) bad = true;
        float last = 0.f;
        for (int j = 1; j < m && j < SCARLET_MAX_LAYERS; ++j) {
            const float p = a.perc ? a.perc[c + j] : 25.f;
            if (!(p > 0.f && p < 100.f && p > last)) bad = true;
            last = p;
        }
    }
    if (bad) {
        a.status[s] |= SCARLET_STATUS_BAD_INIT;
        a.active[s] = 0;
    } else
        a.status[s] &= ~SCARLET_STATUS_BAD_INIT;
    a.ncomp[s] = bad ? 0 : n;
}

// max of the model PSF (get_psf_sed's frame.psfs[0].max()), 1 without one
__device__ __forceinline__ float init_model_psf_max(const InitSrcArgs &a, float *redf)
{
    if (!a.model_psf) return 1.f;
    float v = -__builtin_huge_valf();
    bool nan = false;
    for (int i = threadIdx.x; i < a.P * a.P; i += SC_BLOCK) {
        const float p = a.model_psf[i];
        nan |= p != p;
        v = fmaxf(v, p);
    }
    return block_max_nan(v, nan, redf);
}

// pixel SED of component c at (cy, cx) into sed_s: / obs peak, then x max(model PSF) when `psf_max` is not NULL
__device__ __forceinline__ void init_pixel_sed(const InitSrcArgs &a, int s, int cy, int cx, const float *psf_max,
                                               float *sed_s)
{
    const int HW = a.H * a.W;
    if (threadIdx.x < a.B) {
        float v = a.images[((size_t)s * a.B + threadIdx.x) * HW + cy * a.W + cx];
        if (a.obs_peak) v = v / a.obs_peak[(size_t)s * a.peak_stride + threadIdx.x];
        if (psf_max) v = v * *psf_max;
        sed_s[threadIdx.x] = v;
    }
    __syncthreads();
}

__device__ __forceinline__ void init_scene_bg(const InitSrcArgs &a, int s, double (&bg)[SC_BMAX])
{
#pragma unroll
    for (int b = 0; b < SC_BMAX; ++b) bg[b] = b < a.B ? (double)a.bg_rms[(size_t)s * a.bg_stride + b] : 1.0;
}

// the float64 tile of one component (row stride W + 1), in dynamic LDS or, for GT, in a temporary HBM buffer:
// k_init_extended, k_init_extended_rows, k_init_layers
__host__ __device__ inline size_t init_tile_bytes(int H, int W) { return sizeof(double) * (size_t)H * (W + 1); }

// ---- ExtendedSource with the scene's own noise and PSF peaks: what k_init_extended does for one row of bg_rms
// RAGGED: the scene's own frame (frame_hw) bounds the coadd, the symmetry window, the sweep and the centre test; the
// rest of the H x W plane is written as zero
template <bool GT, bool RAGGED = false>
__global__ __launch_bounds__(SC_BLOCK) void k_init_extended_rows(InitSrcArgs a, double *gtile)
{
    extern __shared__ __align__(16) double ldsd[];
    const int c = blockIdx.x, s = c / a.K, PH = a.H, PW = a.W, PHW = PH * PW, B = a.B;
    __shared__ double red[SC_NWAVES];
    __shared__ float redf[SC_NWAVES], sed_s[SC_BMAX], mmax_s;
    if (c - s * a.K >= a.ncomp[s] || init_kind(a, c) != SCARLET_INIT_EXTENDED) return;
    int fh = PH, fw = PW;
    if (RAGGED && !frame_ok(a.frame_hw, s, PH, PW, fh, fw)) return;
    const int H = fh, W = fw, HW = H * W;
    const int wbuf = a.cur[s];
    float *gm = a.morph[wbuf] + (size_t)c * PHW, *gs = a.sed[wbuf] + (size_t)c * B;
    const int cy = a.centers[2 * c], cx = a.centers[2 * c + 1];
    if (cy < 0 || cy >= H || cx < 0 || cx >= W) { init_empty_outside(gm, gs, PHW, B, &a.flags[c], &a.status[s]); return; }
    const float mmax = init_model_psf_max(a, redf);
    if (threadIdx.x == 0) mmax_s = mmax;
    __syncthreads();
    init_pixel_sed(a, s, cy, cx, a.model_psf ? &mmax_s : nullptr, sed_s);
    TileT<double> t; t.H = H; t.W = W; t.LW = PW + 1;
    t.m = GT ? gtile + (size_t)c * PH * (PW + 1) : ldsd;
    double bg[SC_BMAX], cutoff;
    init_scene_bg(a, s, bg);
    const int lstop = init_detect_tile<GT, RAGGED>(t, a.images + (size_t)s * B * PHW, B, cy, cx, sed_s, bg, a.thresh,
                                                   a.do_symmetric, a.do_monotonic, a.no_hybrid, cutoff, PW, PHW);
    double cnt = 0;
    for (int i = threadIdx.x; i < HW; i += SC_BLOCK)
        if (init_kept(t, i, cy, cx, cutoff, lstop)) cnt += 1;
    cnt = block_sum(cnt, red);
    const double centre = t.m[cy * t.LW + cx] > cutoff ? t.m[cy * t.LW + cx] : 0.0;
    for (int i = threadIdx.x; i < HW; i += SC_BLOCK)
        gm[RAGGED ? (i / W) * PW + (i % W) : i] = (float)(init_kept(t, i, cy, cx, cutoff, lstop) ? t.m[(i / W) * t.LW + (i % W)] / centre : 0.0);
    if (RAGGED) zero_outside_frame(gm, PH, PW, H, W, threadIdx.x, SC_BLOCK);
    if (threadIdx.x < B) gs[threadIdx.x] = sed_s[threadIdx.x];
    if (threadIdx.x == 0)
        a.flags[c] = SCARLET_FLAG_SED_NOT_CONVERGED | SCARLET_FLAG_MORPH_NOT_CONVERGED |
                     (cnt == 0 ? SCARLET_FLAG_NO_VALID_PIXELS : 0);
}

// ---- PointSource (source.py:360-380): the model PSF pasted with its centre on the pixel and clipped to the frame
// (a single 1 without one); SED = pixel / obs peak
// RAGGED: the centre test and the clipping of the paste are the scene's own frame's (frame_hw); the walk covers the whole
// H x W plane with its own strides, so every pixel outside the frame is written as zero
template <bool RAGGED = false>
__global__ __launch_bounds__(SC_BLOCK) void k_init_point(InitSrcArgs a)
{
    const int c = blockIdx.x, s = c / a.K, H = a.H, W = a.W, HW = H * W, B = a.B;
    __shared__ float sed_s[SC_BMAX];
    if (c - s * a.K >= a.ncomp[s] || init_kind(a, c) != SCARLET_INIT_POINT) return;
    int fh = H, fw = W;
    if (RAGGED && !frame_ok(a.frame_hw, s, H, W, fh, fw)) return;
    const int wbuf = a.cur[s];
    float *gm = a.morph[wbuf] + (size_t)c * HW, *gs = a.sed[wbuf] + (size_t)c * B;
    const int cy = a.centers[2 * c], cx = a.centers[2 * c + 1];
    if (cy < 0 || cy >= fh || cx < 0 || cx >= fw) { init_empty_outside(gm, gs, HW, B, &a.flags[c], &a.status[s]); return; }
    init_pixel_sed(a, s, cy, cx, nullptr, sed_s);
    const int R = (a.P - 1) / 2;
    for (int i = threadIdx.x; i < HW; i += SC_BLOCK) {
        const int dy = i / W - cy + R, dx = i % W - cx + R;
        float v;
        if (a.model_psf) v = (dy >= 0 && dy < a.P && dx >= 0 && dx < a.P) ? a.model_psf[dy * a.P + dx] : 0.f;
        else v = (i / W == cy && i % W == cx) ? 1.f : 0.f;
        if (RAGGED && (i / W >= fh || i % W >= fw)) v = 0.f;
        gm[i] = v;
    }
    if (threadIdx.x < B) gs[threadIdx.x] = sed_s[threadIdx.x];
    if (threadIdx.x == 0) a.flags[c] = SCARLET_FLAG_SED_NOT_CONVERGED | SCARLET_FLAG_MORPH_NOT_CONVERGED;
}

// ---- MultiComponentSource (init_multicomponent_source, source.py:242-295): one workgroup per group, on the
// workgroup of its first member.  Base morphology = the extended start at the group's centre (symmetric =
// b->symmetric), layers cut at perc * max / 100, each divided by its own max (float32), SEDs = the least-squares
// fit (M M^T)^-1 M D^T to the scene's images, sums and solve in float64.
__device__ __forceinline__ double layer_value(double m, int j, int n, const double *tcut)
{
    // tcut[0] = 0, tcut[j] = cut j (1 <= j < n): member j holds the flux between cut j and cut j + 1
    if (j + 1 < n && m > tcut[j + 1]) return tcut[j + 1] - tcut[j];
    if (j == 0) return m;
    return m > tcut[j] ? m - tcut[j] : 0.0;
}

// RAGGED: the scene's own frame (frame_hw) in the top-left corner of planes of PH x PW pixels.  The detection tile, the
// layer cuts, the layers' maxima and the normal equations run over the scene's h_s x w_s pixels only; images and
// morphologies are addressed with the planes' strides, the float64 tile has row stride PW + 1, and every layer's plane is
// written as zero outside the frame.
template <bool GT, bool RAGGED = false>
__global__ __launch_bounds__(SC_BLOCK) void k_init_layers(InitSrcArgs a, double *gtile)
{
    extern __shared__ __align__(16) double ldsd[];
    const int c = blockIdx.x, s = c / a.K, k = c - s * a.K, PH = a.H, PW = a.W, PHW = PH * PW, B = a.B;
    __shared__ double red[SC_NWAVES], tcut[SCARLET_MAX_LAYERS + 1], gram[SCARLET_MAX_LAYERS][SCARLET_MAX_LAYERS],
        rhs[SCARLET_MAX_LAYERS][SC_BMAX];
    __shared__ float redf[SC_NWAVES], sed_s[SC_BMAX], mmax_s, lmax[SCARLET_MAX_LAYERS];
    __shared__ int singular_s;
    const int ns = a.ncomp[s];
    if (k >= ns || !a.group || a.group[c] < 0 || (k > 0 && a.group[c - 1] == a.group[c])) return;
    int fh = PH, fw = PW;
    if (RAGGED && !frame_ok(a.frame_hw, s, PH, PW, fh, fw)) return;
    const int H = fh, W = fw, HW = H * W;
    int n = 1;
    while (k + n < ns && a.group[c + n] == a.group[c]) ++n;
    n = uniform(n);                                   // k_init_check left at most SCARLET_MAX_LAYERS
    const int wbuf = a.cur[s];
    float *gm0 = a.morph[wbuf] + (size_t)c * PHW, *gs0 = a.sed[wbuf] + (size_t)c * B;
    const int cy = a.centers[2 * c], cx = a.centers[2 * c + 1];
    if (cy < 0 || cy >= H || cx < 0 || cx >= W) {
        for (int j = 0; j < n; ++j)
            init_empty_outside(gm0 + (size_t)j * PHW, gs0 + (size_t)j * B, PHW, B, &a.flags[c + j], &a.status[s]);
        return;
    }
    const float mmax = init_model_psf_max(a, redf);
    if (threadIdx.x == 0) mmax_s = mmax;
    __syncthreads();
    init_pixel_sed(a, s, cy, cx, a.model_psf ? &mmax_s : nullptr, sed_s);
    TileT<double> t; t.H = H; t.W = W; t.LW = PW + 1;
    t.m = GT ? gtile + (size_t)c * PH * (PW + 1) : ldsd;
    const float *img = a.images + (size_t)s * B * PHW;
    double bg[SC_BMAX], cutoff;
    init_scene_bg(a, s, bg);
    const int lstop = init_detect_tile<GT, RAGGED>(t, img, B, cy, cx, sed_s, bg, a.thresh, a.group_symmetric,
                                                   a.do_monotonic, a.no_hybrid, cutoff, PW, PHW);
    double cnt = 0;
    for (int i = threadIdx.x; i < HW; i += SC_BLOCK)
        if (init_kept(t, i, cy, cx, cutoff, lstop)) cnt += 1;
    cnt = block_sum(cnt, red);                        // (its barriers also order the tile reads below)
    if (cnt == 0) {                                   // SourceInitError: every member gets NO_VALID_PIXELS
        for (int j = 0; j < n; ++j) {
            for (int i = threadIdx.x; i < PHW; i += SC_BLOCK) gm0[(size_t)j * PHW + i] = 0.f;
            if (threadIdx.x < B) gs0[(size_t)j * B + threadIdx.x] = 0.f;
        }
        if (threadIdx.x < n)
            a.flags[c + threadIdx.x] = SCARLET_FLAG_SED_NOT_CONVERGED | SCARLET_FLAG_MORPH_NOT_CONVERGED |
                                       SCARLET_FLAG_NO_VALID_PIXELS;
        return;
    }
    const double centre = t.m[cy * t.LW + cx] > cutoff ? t.m[cy * t.LW + cx] : 0.0;
    // the tile becomes the base morphology (float64, like the reference's coadd) and its max
    double vmax = -__builtin_huge_val();
    __syncthreads();                                  // every thread has read the centre
    for (int i = threadIdx.x; i < HW; i += SC_BLOCK) {
        double *p = &t.m[(i / W) * t.LW + (i % W)];
        const double m = init_kept(t, i, cy, cx, cutoff, lstop) ? *p / centre : 0.0;
        vmax = fmax(vmax, m);
        *p = m;
    }
    for (int o = SC_WAVE / 2; o > 0; o >>= 1) vmax = fmax(vmax, __shfl_xor(vmax, o));
    if ((threadIdx.x & (SC_WAVE - 1)) == 0) red[threadIdx.x / SC_WAVE] = vmax;
    __syncthreads();
    vmax = red[0];
#pragma unroll
    for (int w = 1; w < SC_NWAVES; ++w) vmax = fmax(vmax, red[w]);
    if (threadIdx.x <= SCARLET_MAX_LAYERS) {
        const int j = threadIdx.x;
        const double p = (j >= 1 && j < n) ? (double)(a.perc ? a.perc[c + j] : 25.f) : 0.0;
        tcut[j] = p * vmax / 100;
    }
    __syncthreads();
    // each layer's max in float32
    for (int j = 0; j < n; ++j) {
        float v = -__builtin_huge_valf();
        for (int i = threadIdx.x; i < HW; i += SC_BLOCK)
            v = fmaxf(v, (float)layer_value(t.m[(i / W) * t.LW + (i % W)], j, n, tcut));
        v = block_max_nan(v, false, redf);
        if (threadIdx.x == 0) lmax[j] = v;
    }
    __syncthreads();
    bool empty = false;
    for (int j = 0; j < n; ++j) empty |= !(lmax[j] > 0.f);
    if (empty) {
        // the reference divides by zero here: the scene is left inactive and the update does not run on it
        if (threadIdx.x == 0) {
            atomicOr(&a.status[s], SCARLET_STATUS_BAD_INIT);
            a.active[s] = 0;
            a.ncomp[s] = 0;
        }
        return;
    }
    for (int j = 0; j < n; ++j) {
        for (int i = threadIdx.x; i < HW; i += SC_BLOCK)
            gm0[(size_t)j * PHW + (RAGGED ? (i / W) * PW + (i % W) : i)] =
                (float)layer_value(t.m[(i / W) * t.LW + (i % W)], j, n, tcut) / lmax[j];
        if (RAGGED) zero_outside_frame(gm0 + (size_t)j * PHW, PH, PW, H, W, threadIdx.x, SC_BLOCK);
    }
    // the normal equations: gram[j][q] = sum_i M_j M_q, rhs[j][b] = sum_i M_j D_b, one column q (or band) per pass
    for (int q = 0; q < n + B; ++q) {
        double acc[SCARLET_MAX_LAYERS];
#pragma unroll
        for (int j = 0; j < SCARLET_MAX_LAYERS; ++j) acc[j] = 0;
        for (int i = threadIdx.x; i < HW; i += SC_BLOCK) {
            const double m = t.m[(i / W) * t.LW + (i % W)];
            const double o = q < n ? (double)((float)layer_value(m, q, n, tcut) / lmax[q])
                                   : (double)img[(size_t)(q - n) * PHW + (RAGGED ? (i / W) * PW + (i % W) : i)];
#pragma unroll
            for (int j = 0; j < SCARLET_MAX_LAYERS; ++j)
                if (j < n) acc[j] += (double)((float)layer_value(m, j, n, tcut) / lmax[j]) * o;
        }
#pragma unroll
        for (int j = 0; j < SCARLET_MAX_LAYERS; ++j) {
            if (j < n) {
                const double v = block_sum(acc[j], red);
                if (threadIdx.x == 0) {
                    if (q < n) gram[j][q] = v;
                    else rhs[j][q - n] = v;
                }
            }
        }
    }
    __syncthreads();
    // Gauss-Jordan elimination with partial pivoting on lane 0 (n <= 8, B <= 8)
    if (threadIdx.x == 0) {
        int singular = 0;
        for (int col = 0; col < n; ++col) {
            int piv = col;
            for (int r = col + 1; r < n; ++r)
                if (fabs(gram[r][col]) > fabs(gram[piv][col])) piv = r;
            if (!(fabs(gram[piv][col]) > 0)) { singular = 1; break; }
            if (piv != col) {
                for (int q = 0; q < n; ++q) { const double x = gram[col][q]; gram[col][q] = gram[piv][q]; gram[piv][q] = x; }
                for (int b = 0; b < B; ++b) { const double x = rhs[col][b]; rhs[col][b] = rhs[piv][b]; rhs[piv][b] = x; }
            }
            const double inv = 1.0 / gram[col][col];
            for (int r = 0; r < n; ++r) {
                if (r == col) continue;
                const double f = gram[r][col] * inv;
                if (f == 0) continue;
                for (int q = col; q < n; ++q) gram[r][q] -= f * gram[col][q];
                for (int b = 0; b < B; ++b) rhs[r][b] -= f * rhs[col][b];
            }
        }
        if (!singular)
            for (int r = 0; r < n; ++r)
                for (int b = 0; b < B; ++b) rhs[r][b] /= gram[r][r];
        singular_s = singular;
    }
    __syncthreads();
    if (singular_s) {                                 // np.linalg.inv raises: bad input of this scene
        if (threadIdx.x == 0) {
            atomicOr(&a.status[s], SCARLET_STATUS_BAD_INIT);
            a.active[s] = 0;
            a.ncomp[s] = 0;
        }
        return;
    }
    if (threadIdx.x < n * B) {
        const int j = threadIdx.x / B, b = threadIdx.x - j * B;
        gs0[(size_t)j * B + b] = (float)rhs[j][b];
    }
    if (threadIdx.x < n) a.flags[c + threadIdx.x] = SCARLET_FLAG_SED_NOT_CONVERGED | SCARLET_FLAG_MORPH_NOT_CONVERGED;
}
