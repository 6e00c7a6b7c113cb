// scarlet_hip.hip -- C ABI (include/scarlet_hip.h) of the gfx950 deblending engine.
//
// Build: hipcc --offload-arch=gfx950 -O3 -fPIC -shared scarlet_hip.hip -o libscarlet_hip.so
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <atomic>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>
#include <algorithm>
#include <hipfft/hipfft.h>

#include "common.h"
#include "prox_ops.h"
#include "engine.h"
#include "fused.h"
#include "fused2.h"
#include "bigk.h"
#include "hugek.h"
#include "boxupdate.h"
#include "psf_path.h"
#include "fftconv.h"
#include "extras.h"
#include "initsrc.h"
#include "multiobs.h"
#include "multiobs_wide.h"
#include "lowres.h"
#include "lowres_stream.h"
#include "prior.h"
#include "launch_plan.h"

__constant__ unsigned short sc_nfl_table[SC_NFL_MAX];

static thread_local char g_err[512] = "";
static int set_err(int code, const char *msg)
{
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}
#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            snprintf(g_err, sizeof(g_err), "%s failed: %s (%s:%d)", #expr,               \
                     hipGetErrorString(e_), __FILE__, __LINE__);                         \
            return SCARLET_E_HIP;                                                        \
        }                                                                                \
    } while (0)

extern "C" const char *scarlet_version(void) { return "scarlet_amd-hip 0.2 (gfx950)"; }

// ---- diagnostic switches: process-wide integers, initialised ONCE from the
// environment (SCARLET_<NAME>) at first use and changed afterwards only through scarlet_set_option.
// None of them changes results beyond float32 rounding.
enum { OPT_NO_EXACT = 0, OPT_NO_KSCACHE, OPT_FUSED_V1, OPT_NO_FUSED, OPT_FORCE_BLOCK_UPDATE, OPT_NO_HYBRID_SWEEP,
       OPT_PAD_LDS, OPT_STAMPS, OPT_PSF_HIPFFT, OPT_NO_BOX, OPT_NO_BOX2, OPT_NO_PSF3PASS, OPT_NO_SIDE_STREAM, OPT_NO_GRAM_MFMA, OPT_NO_BIGK_FUSED, OPT_NO_PIPELINE, OPT_NO_PERSIST, OPT_PERSIST_DBG, OPT_FORCE_HUGEK, OPT_NO_PLACE, OPT_NO_LOWRES_MFMA, OPT_LOWRES_STREAMED, OPT_LOWRES_CHUNK, OPT_COUNT };
static const char *const g_opt_names[OPT_COUNT] = {"NO_EXACT", "NO_KSCACHE", "FUSED_V1", "NO_FUSED", "FORCE_BLOCK_UPDATE",
                                                   "NO_HYBRID_SWEEP", "PAD_LDS", "STAMPS", "PSF_HIPFFT", "NO_BOX", "NO_BOX2",
                                                   "NO_PSF3PASS", "NO_SIDE_STREAM", "NO_GRAM_MFMA", "NO_BIGK_FUSED", "NO_PIPELINE", "NO_PERSIST", "PERSIST_DBG", "FORCE_HUGEK", "NO_PLACE", "NO_LOWRES_MFMA", "LOWRES_STREAMED", "LOWRES_CHUNK"};
static std::atomic<int> g_opt[OPT_COUNT];
static std::once_flag g_opt_once;
static void options_init(void)
{
    std::call_once(g_opt_once, [] {
        for (int i = 0; i < OPT_COUNT; ++i) {
            char name[64];
            snprintf(name, sizeof(name), "SCARLET_%s", g_opt_names[i]);
            const char *v = getenv(name);
            int val = 0;
            if (v) { val = atoi(v); if (val == 0 && v[0] != '0') val = 1; }    // "yes", "" ... count as on
            if (v && !v[0]) val = 1;
            g_opt[i].store(val, std::memory_order_relaxed);
        }
    });
}
static inline int opt(int which) { options_init(); return g_opt[which].load(std::memory_order_relaxed); }
// PSF_HIPFFT and STAMPS decide the LAYOUT of a PSF batch's workspace (ws_layout): they are read when a workspace is
// sized and again by every later call on that batch, so a change in between would move regions under a live batch
// (K-hat and tables read from the wrong offsets, writes past the allocation).  The first PSF layout computed for a live
// batch (ws_layout, WS_FIX) therefore FREEZES the two switches: scarlet_set_option then refuses a different value.
static std::atomic<bool> g_layout_frozen{false};
// FORCE_HUGEK (diagnostics: the K > 32 gradient path of hugek.h for 8 < K <= 32 as well) adds the Gram area of that
// path to the workspace of such batches: it freezes, likewise, once a workspace with 8 < K <= 32 has been sized.
static std::atomic<bool> g_hugek_frozen{false};
extern "C" int scarlet_set_option(const char *name, int value)
{
    options_init();
    if (!name) return set_err(SCARLET_E_ARG, "null option name");
    for (int i = 0; i < OPT_COUNT; ++i)
        if (!strcmp(name, g_opt_names[i])) {
            if (i == OPT_FORCE_HUGEK && g_hugek_frozen.load() && (g_opt[i].load() != 0) != (value != 0))
                return set_err(SCARLET_E_ARG, "FORCE_HUGEK fixes the workspace layout of batches with 8 < K <= 32: it cannot "
                                              "change after the first such workspace of the process was sized");
            if ((i == OPT_PSF_HIPFFT || i == OPT_STAMPS) && g_layout_frozen.load() && (g_opt[i].load() != 0) != (value != 0))
                return set_err(SCARLET_E_ARG, "PSF_HIPFFT / STAMPS fix the workspace layout of PSF batches: they cannot change "
                                              "after the first PSF workspace of the process was sized");
            if (i == OPT_LOWRES_CHUNK) {            // (the one switch that is a count: planes per chunk, 0 = automatic)
                if (value < 0) return set_err(SCARLET_E_ARG, "LOWRES_CHUNK: planes per chunk, 0 = automatic");
                return g_opt[i].exchange(value);
            }
            return g_opt[i].exchange(value) != 0 ? 1 : 0;
        }
    return set_err(SCARLET_E_ARG, "unknown option");
}

// device allocation released on every exit path of the set-up / host-pointer entry points
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    template <typename T> T *as() const { return (T *)p; }
};
#define DEV_ALLOC(buf, bytes) HIP_TRY(hipMalloc(&(buf).p, (bytes)))
extern "C" const char *scarlet_last_error(void) { return g_err; }

// scipy.fftpack.next_fast_len: smallest 2^a 3^b 5^c >= n
extern "C" int scarlet_next_fast_len(int n)
{
    if (n <= 1) return 1;
    long best = -1;
    for (long p5 = 1; p5 < 2L * n; p5 *= 5)
        for (long p35 = p5; p35 < 2L * n; p35 *= 3) {
            long v = p35;
            while (v < n) v *= 2;
            if (best < 0 || v < best) best = v;
        }
    return (int)best;
}

static int ensure_tables(void)
{
    static bool done[64] = {false};
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return set_err(SCARLET_E_HIP, "device index out of range");
    if (done[dev]) return SCARLET_OK;
    std::vector<unsigned short> t(SC_NFL_MAX);
    for (int i = 0; i < SC_NFL_MAX; ++i) t[i] = (unsigned short)scarlet_next_fast_len(i);
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(sc_nfl_table), t.data(), SC_NFL_MAX * sizeof(unsigned short)));
    done[dev] = true;
    return SCARLET_OK;
}

// diagnostics (STAMPS switch): a device buffer of shader-clock stamps owned by the library, read back with
// scarlet_debug_stamps; NULL when the switch is off
static long long *g_dbg_stamps = nullptr;
static size_t g_dbg_count = 0;
static std::mutex g_dbg_mu;
static long long *debug_stamps(size_t count)
{
    if (!opt(OPT_STAMPS)) return nullptr;
    std::lock_guard<std::mutex> lock(g_dbg_mu);
    if (count > g_dbg_count) {
        if (g_dbg_stamps) (void)hipFree(g_dbg_stamps);
        g_dbg_stamps = nullptr; g_dbg_count = 0;
        if (hipMalloc((void **)&g_dbg_stamps, count * sizeof(long long)) != hipSuccess) return nullptr;
        g_dbg_count = count;
    }
    (void)hipMemset(g_dbg_stamps, 0, g_dbg_count * sizeof(long long));
    return g_dbg_stamps;
}
extern "C" int64_t scarlet_debug_stamps(int64_t *out, int64_t capacity)
{
    std::lock_guard<std::mutex> lock(g_dbg_mu);
    if (!g_dbg_stamps || !out || capacity <= 0) return 0;
    const int64_t n = capacity < (int64_t)g_dbg_count ? capacity : (int64_t)g_dbg_count;
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(out, g_dbg_stamps, n * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return n;
}

// compute units of the current device (cached per device index)
static int device_cu_count(void)
{
    static std::atomic<int> cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int n = cus[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        hipDeviceProp_t prop;
        n = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

template <typename Kern>
static int allow_lds(Kern k, size_t bytes)
{
    if (bytes > LDS_LIMIT) return set_err(SCARLET_E_TOO_LARGE, "image tile does not fit in LDS");
    if (bytes > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return SCARLET_OK;
}
// allow the dynamic LDS, launch
template <typename Kern, typename... Args>
static int launch_lds(Kern k, dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &... args)
{
    if (int rc = allow_lds(k, lds)) return rc;
    hipLaunchKernelGGL(k, grid, block, lds, st, args...);
    return SCARLET_OK;
}

// =====================================================================================
// 2. batched device operators
// =====================================================================================
enum { OP_MONO_WEIGHTED = 0, OP_MONO_NEAREST = 1, OP_SYMMETRY = 2, OP_MAX_PIXEL = 3, OP_CENTROID = 4 };

struct OpArgs {
    float *x; int n, H, W;
    int *centers; double *shifts; int *status;
    int op, algorithm, use_fill;
    float thresh, strength, fill;
    const double *psf; int P;
};

// GT: arrays whose tile does not fit LDS (up to SCARLET_MAX_SIDE a side) are processed in place in HBM, the GEMM
// scratch of the k-space symmetry in `gscratch` (see k_source_update<2> in engine.h)
template <bool GT>
__global__ __launch_bounds__(SC_BLOCK) void k_operator(OpArgs a, float *gscratch)
{
    extern __shared__ __align__(16) float lds[];
    const int c = blockIdx.x, H = a.H, W = a.W, HW = H * W;
    const int hp = round16(H), wp = round16(W);
    float *g = a.x + (size_t)c * HW;
    Tile t; t.H = H; t.W = W;
    float *scr, *av;
    if (GT) { t.LW = W; t.m = g; scr = gscratch + (size_t)c * hp * scratch_stride(wp); av = lds; }
    else    { t.LW = tile_stride(W); t.m = lds; scr = lds + H * t.LW; av = scr + hp * scratch_stride(wp); }
    // (sized by update_lds_bytes, or plane_lds_bytes for GT: prox_ops.h)
    float *bv = av + 2 * hp, *cv = bv + 2 * wp, *zv = cv + 2 * wp;
    float *stage = GT ? zv + wp : nullptr;
    __shared__ double red[SC_NWAVES];
    __shared__ int ctr[2];
    __shared__ double shf[2];
    __shared__ int stat;
    if (!GT)
        for (int i = threadIdx.x; i < HW; i += SC_BLOCK) t.m[(i / W) * t.LW + (i % W)] = g[i];
    if (threadIdx.x == 0) stat = 0;
    __syncthreads();
    const int cy = a.centers[2 * c], cx = a.centers[2 * c + 1];
    if (cy < 0 || cy >= H || cx < 0 || cx >= W) {
        // a centre outside the array (the reference raises IndexError): leave the array alone, flag it
        if (threadIdx.x == 0 && a.status) atomicOr(&a.status[c], SCARLET_STATUS_CENTER_AT_EDGE);
        return;
    }
    bool writeback = !GT;
    switch (a.op) {
    case OP_MONO_WEIGHTED: monotonic_tile<false, float>(t, cy, cx, a.thresh); break;
    case OP_MONO_NEAREST:  monotonic_tile<true, float>(t, cy, cx, a.thresh); break;
    case OP_SYMMETRY: {
        const double dy = a.shifts ? a.shifts[2 * c] : 0.0, dx = a.shifts ? a.shifts[2 * c + 1] : 0.0;
        symmetry_tile(t, cy, cx, a.algorithm, a.strength, dy, dx, a.use_fill != 0, a.fill,
                      scr, av, bv, cv, zv, stage, GT);
        break;
    }
    case OP_MAX_PIXEL:
        max_pixel_tile(t, cy, cx, ctr, &stat);
        if (threadIdx.x == 0) { a.centers[2 * c] = ctr[0]; a.centers[2 * c + 1] = ctr[1]; }
        writeback = false;
        break;
    case OP_CENTROID:
        centroid_tile(t, a.psf, a.P, cy, cx, red, ctr, shf, &stat);
        if (threadIdx.x == 0) {
            a.centers[2 * c] = ctr[0]; a.centers[2 * c + 1] = ctr[1];
            a.shifts[2 * c] = shf[0]; a.shifts[2 * c + 1] = shf[1];
        }
        writeback = false;
        break;
    }
    __syncthreads();
    if (writeback)
        for (int i = threadIdx.x; i < HW; i += SC_BLOCK) g[i] = t.m[(i / W) * t.LW + (i % W)];
    if (threadIdx.x == 0 && stat && a.status) atomicOr(&a.status[c], stat);
}

// the same operators, one wave per array (wave_ops.h), H, W <= 64
__global__ __launch_bounds__(SC_BLOCK) void k_operator_w(OpArgs a)
{
    extern __shared__ __align__(16) float lds[];
    const int wid = threadIdx.x / SC_WAVE, lane = threadIdx.x & (SC_WAVE - 1);
    const int c = blockIdx.x * SC_NWAVES + wid;
    if (c >= a.n) return;
    const int H = a.H, W = a.W, HW = H * W;
    Tile t; t.H = H; t.W = W; t.LW = tile_stride(W);
    t.m = lds + (size_t)wid * (H * t.LW + SC_WAVE_VEC_FLOATS);      // wave_tile_floats (wave_ops.h)
    float *vec = t.m + H * t.LW;
    float *g = a.x + (size_t)c * HW;
    for (int i = lane; i < HW; i += SC_WAVE) t.m[(i / W) * t.LW + (i % W)] = g[i];
    wave_sync();
    int cy = a.centers[2 * c], cx = a.centers[2 * c + 1];
    int stat = 0;
    bool writeback = true;
    if (cy < 0 || cy >= H || cx < 0 || cx >= W) {         // as in k_operator
        if (lane == 0 && a.status) atomicOr(&a.status[c], SCARLET_STATUS_CENTER_AT_EDGE);
        return;
    }
    switch (a.op) {
    case OP_MONO_WEIGHTED: wave_monotonic<float>(t, cy, cx, a.thresh); break;
    case OP_SYMMETRY: {
        const double dy = a.shifts ? a.shifts[2 * c] : 0.0, dx = a.shifts ? a.shifts[2 * c + 1] : 0.0;
        wave_symmetry(t, cy, cx, a.algorithm, a.strength, dy, dx, a.use_fill != 0, a.fill, vec);
        break;
    }
    case OP_MAX_PIXEL:
        wave_max_pixel(t, cy, cx, stat);
        if (lane == 0) { a.centers[2 * c] = cy; a.centers[2 * c + 1] = cx; }
        writeback = false;
        break;
    case OP_CENTROID: {
        double dy = 0, dx = 0;
        wave_centroid(t, a.psf, a.P, cy, cx, dy, dx, stat);
        if (lane == 0) {
            a.centers[2 * c] = cy; a.centers[2 * c + 1] = cx;
            a.shifts[2 * c] = dy; a.shifts[2 * c + 1] = dx;
        }
        writeback = false;
        break;
    }
    }
    wave_sync();
    if (writeback)
        for (int i = lane; i < HW; i += SC_WAVE) g[i] = t.m[(i / W) * t.LW + (i % W)];
    if (lane == 0 && stat && a.status) atomicOr(&a.status[c], stat);
}

static int launch_operator(OpArgs a, void *stream)
{
    if (!a.x || a.n < 0 || a.H <= 0 || a.W <= 0 || !a.centers)
        return set_err(SCARLET_E_ARG, "bad operator arguments");
    if (a.H > SCARLET_MAX_SIDE || a.W > SCARLET_MAX_SIDE)
        return set_err(SCARLET_E_TOO_LARGE, "arrays larger than 1024 x 1024 (SCARLET_MAX_SIDE) are not supported");
    if (a.n == 0) return SCARLET_OK;
    int rc = ensure_tables();
    if (rc) return rc;
    // the update's choice of form without a workspace behind it; this operator's nearest-neighbour sweep stays on the
    // workgroup form (the ring sweep on one wave, wave_nearest_monotonic, serves the update's options instance)
    const UpdatePlan p = update_plan(a.H, a.W, {a.op != OP_MONO_NEAREST && !opt(OPT_FORCE_BLOCK_UPDATE)});
    hipStream_t st = (hipStream_t)stream;
    DevBuf gscratch;                          // released on every path, after the kernel has finished
    switch (p.form) {
    case FORM_WAVE:
        rc = launch_lds(k_operator_w, dim3((a.n + SC_NWAVES - 1) / SC_NWAVES), dim3(SC_BLOCK), p.lds, st, a);
        break;
    case FORM_TILE:
        rc = launch_lds(k_operator<false>, dim3(a.n), dim3(SC_BLOCK), p.lds, st, a, (float *)nullptr);
        break;
    default:
        if (a.op == OP_SYMMETRY)
            DEV_ALLOC(gscratch, sizeof(float) * (size_t)a.n * round16(a.H) * scratch_stride(round16(a.W)));
        rc = launch_lds(k_operator<true>, dim3(a.n), dim3(SC_BLOCK), p.lds, st, a, gscratch.as<float>());   // (past 48 KB from ~512 columns on)
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    if (gscratch.p) HIP_TRY(hipStreamSynchronize(st));
    return SCARLET_OK;
}

extern "C" int scarlet_prox_weighted_monotonic(float *x, int n, int H, int W, const int32_t *centers,
                                               float thresh, void *stream)
{
    OpArgs a = {};
    a.x = x; a.n = n; a.H = H; a.W = W; a.centers = (int *)centers; a.op = OP_MONO_WEIGHTED;
    a.thresh = thresh;
    return launch_operator(a, stream);
}

extern "C" int scarlet_prox_nearest_monotonic(float *x, int n, int H, int W, const int32_t *centers,
                                              float thresh, void *stream)
{
    if (thresh != 0.f)   // operator.py:107-110 raises ValueError
        return set_err(SCARLET_E_ARG, "Thresholding does not work with nearest neighbor monotonicity");
    OpArgs a = {};
    a.x = x; a.n = n; a.H = H; a.W = W; a.centers = (int *)centers; a.op = OP_MONO_NEAREST;
    return launch_operator(a, stream);
}

extern "C" int scarlet_prox_symmetry(float *x, int n, int H, int W, const int32_t *centers,
                                     const double *shifts, int algorithm, float strength,
                                     int use_fill, float fill, void *stream)
{
    const int base_alg = algorithm & ~SCARLET_SYM_FULL_WINDOW;
    if (base_alg < 0 || base_alg > 2) return set_err(SCARLET_E_ARG, "algorithm must be one of 'soft', 'sdss', 'kspace'");
    if (base_alg == SCARLET_SYM_KSPACE && !shifts) return set_err(SCARLET_E_ARG, "kspace symmetry needs shifts");
    OpArgs a = {};
    a.x = x; a.n = n; a.H = H; a.W = W; a.centers = (int *)centers; a.shifts = (double *)shifts;
    a.op = OP_SYMMETRY; a.algorithm = algorithm; a.strength = strength; a.use_fill = use_fill; a.fill = fill;
    return launch_operator(a, stream);
}

extern "C" int scarlet_max_pixel(const float *x, int n, int H, int W, int32_t *centers_io,
                                 int32_t *status, void *stream)
{
    OpArgs a = {};
    a.x = (float *)x; a.n = n; a.H = H; a.W = W; a.centers = centers_io; a.status = status; a.op = OP_MAX_PIXEL;
    return launch_operator(a, stream);
}

extern "C" int scarlet_psf_weighted_centroid(const float *x, int n, int H, int W, const double *psf,
                                             int P, int32_t *centers_io, double *shifts_out,
                                             int32_t *status, void *stream)
{
    if (!psf || P <= 0 || !(P & 1) || !shifts_out) return set_err(SCARLET_E_ARG, "bad centroid arguments");
    OpArgs a = {};
    a.x = (float *)x; a.n = n; a.H = H; a.W = W; a.centers = centers_io; a.shifts = shifts_out;
    a.status = status; a.op = OP_CENTROID; a.psf = psf; a.P = P;
    return launch_operator(a, stream);
}

// ---- elementwise prox (proxmin semantics pinned by the reference's tests/test_update.py)
enum { EW_PLUS = 0, EW_HARD = 1, EW_SOFT = 2 };
__global__ void k_elementwise(float *x, int64_t count, int op, float t)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
         i += (int64_t)gridDim.x * blockDim.x) {
        float v = x[i];
        if (op == EW_PLUS) { if (v < 0.f) v = 0.f; }
        else if (op == EW_HARD) { if (fabsf(v) < t) v = 0.f; }
        else {
            const float mag = fabsf(v) - t;
            v = (v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f)) * (mag < 0.f ? 0.f : mag);
        }
        x[i] = v;
    }
}
static int launch_elementwise(float *x, int64_t count, int op, float t, void *stream)
{
    if (count < 0 || (count > 0 && !x)) return set_err(SCARLET_E_ARG, "bad elementwise arguments");
    if (count == 0) return SCARLET_OK;
    int64_t blocks = (count + SC_BLOCK - 1) / SC_BLOCK;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_elementwise, dim3((unsigned)blocks), dim3(SC_BLOCK), 0, (hipStream_t)stream, x, count, op, t);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}
extern "C" int scarlet_prox_plus(float *x, int64_t count, void *stream) { return launch_elementwise(x, count, EW_PLUS, 0.f, stream); }
extern "C" int scarlet_prox_hard(float *x, int64_t count, float t, void *stream) { return launch_elementwise(x, count, EW_HARD, t, stream); }
extern "C" int scarlet_prox_soft(float *x, int64_t count, float t, void *stream) { return launch_elementwise(x, count, EW_SOFT, t, stream); }

// ---- update.normalized (update.py:35-68): one workgroup per component
__global__ __launch_bounds__(SC_BLOCK) void k_normalize(float *sed, float *morph, int B, int HW, int type)
{
    __shared__ double red[SC_NWAVES];
    __shared__ float redf[SC_NWAVES];
    const int c = blockIdx.x;
    float *m = morph + (size_t)c * HW, *s = sed + (size_t)c * B;
    float norm;
    if (type == SCARLET_NORM_MORPH_MAX) {
        float vmax = -INFINITY; bool anynan = false;
        for (int i = threadIdx.x; i < HW; i += SC_BLOCK) { const float v = m[i]; anynan |= (v != v); vmax = fmaxf(vmax, v); }
        norm = block_max_nan(vmax, anynan, redf);
    } else if (type == SCARLET_NORM_MORPH) {
        double acc = 0;
        for (int i = threadIdx.x; i < HW; i += SC_BLOCK) acc += (double)m[i];
        norm = (float)block_sum(acc, red);
    } else {
        double acc = 0;
        for (int i = threadIdx.x; i < B; i += SC_BLOCK) acc += (double)s[i];
        norm = (float)block_sum(acc, red);
    }
    __syncthreads();
    const bool sed_type = (type == SCARLET_NORM_SED);
    for (int i = threadIdx.x; i < HW; i += SC_BLOCK) m[i] = sed_type ? m[i] * norm : m[i] / norm;
    for (int i = threadIdx.x; i < B; i += SC_BLOCK) s[i] = sed_type ? s[i] / norm : s[i] * norm;
}
extern "C" int scarlet_normalize(float *sed, float *morph, int n, int B, int HW, int type, void *stream)
{
    if (type < 0 || type > 2) return set_err(SCARLET_E_ARG, "Unrecognized normalization");
    if (!sed || !morph || n < 0 || B <= 0 || HW <= 0) return set_err(SCARLET_E_ARG, "bad normalize arguments");
    if (n == 0) return SCARLET_OK;
    hipLaunchKernelGGL(k_normalize, dim3(n), dim3(SC_BLOCK), 0, (hipStream_t)stream, sed, morph, B, HW, type);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}

// ---- measurement.threshold / update.threshold / bbox.trim / update.translation (extras.h)
extern "C" int scarlet_log_range(const float *x, int n, int64_t count, double *out, void *stream)
{
    if (n < 0 || count <= 0 || !x || !out) return set_err(SCARLET_E_ARG, "bad log_range arguments");
    if (n == 0) return SCARLET_OK;
    hipLaunchKernelGGL(k_log_range, dim3(n), dim3(SC_BLOCK), 0, (hipStream_t)stream, x, count, out);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}
extern "C" int scarlet_log_hist(const float *x, int n, int64_t count, const double *edges,
                                const int32_t *nbins, int32_t *hist, void *stream)
{
    if (n < 0 || count <= 0 || !x || !edges || !nbins || !hist) return set_err(SCARLET_E_ARG, "bad log_hist arguments");
    if (n == 0) return SCARLET_OK;
    hipLaunchKernelGGL(k_log_hist, dim3(n), dim3(SC_BLOCK), 0, (hipStream_t)stream, x, count, edges, nbins, hist);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}
extern "C" int scarlet_cut_below(float *x, int64_t count, double thresh, void *stream)
{
    if (count < 0 || (count > 0 && !x)) return set_err(SCARLET_E_ARG, "bad cut_below arguments");
    if (count == 0) return SCARLET_OK;
    int64_t blocks = (count + SC_BLOCK - 1) / SC_BLOCK;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_cut_below, dim3((unsigned)blocks), dim3(SC_BLOCK), 0, (hipStream_t)stream, x, count, thresh);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}
extern "C" int scarlet_trim(const float *x, int n, int H, int W, float min_value, int32_t *box, void *stream)
{
    if (n < 0 || H <= 0 || W <= 0 || !x || !box) return set_err(SCARLET_E_ARG, "bad trim arguments");
    if (n == 0) return SCARLET_OK;
    hipLaunchKernelGGL(k_trim, dim3(n), dim3(SC_BLOCK), 0, (hipStream_t)stream, x, H, W, min_value, box);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}
extern "C" int scarlet_resample(const float *in, float *out, int n, int H, int W, const double *taps,
                                const int32_t *win0, int ny, int nx, void *stream)
{
    if (n < 0 || H <= 0 || W <= 0 || !in || !out || in == out || !taps || !win0)
        return set_err(SCARLET_E_ARG, "bad resample arguments");
    if (ny < 1 || nx < 1 || ny > SC_TAPS_MAX || nx > SC_TAPS_MAX)
        return set_err(SCARLET_E_ARG, "resampling kernels have 1 to 12 taps");
    if (n == 0) return SCARLET_OK;
    int bx = (H * W + SC_BLOCK - 1) / SC_BLOCK;
    if (bx > 256) bx = 256;
    hipLaunchKernelGGL(k_resample, dim3(bx, n), dim3(SC_BLOCK), 0, (hipStream_t)stream, in, out, H, W, taps, win0, ny, nx);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}

// ---- apply_filter (operators_pybind11.cc:53-70): gather form, one thread per output pixel
template <typename T>
__global__ void k_apply_filter(const T *image, int H, int W, const T *values,
                               const int *y_start, const int *y_end, const int *x_start,
                               const int *x_end, int n, T *result)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    T acc = (T)0;
    for (int k = 0; k < n; ++k) {
        const int rows = H - y_start[k] - y_end[k], cols = W - x_start[k] - x_end[k];
        const int r = y - y_start[k], cc = x - x_start[k];
        if (r >= 0 && r < rows && cc >= 0 && cc < cols)
            acc += values[k] * image[(y_end[k] + r) * W + x_end[k] + cc];
    }
    result[i] = acc;
}
extern "C" int scarlet_apply_filter(const float *image, int H, int W, const float *values,
                                    const int32_t *y_start, const int32_t *y_end, const int32_t *x_start,
                                    const int32_t *x_end, int n, float *result, void *stream)
{
    if (!image || !result || H <= 0 || W <= 0 || n < 0) return set_err(SCARLET_E_ARG, "bad apply_filter arguments");
    hipLaunchKernelGGL(k_apply_filter<float>, dim3((H * W + SC_BLOCK - 1) / SC_BLOCK), dim3(SC_BLOCK), 0,
                       (hipStream_t)stream, image, H, W, values, y_start, y_end, x_start, x_end, n, result);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}

// =====================================================================================
// 1. host-pointer drop-ins for operators_pybind11 (stage through device memory)
// =====================================================================================
// The reference's loops take an explicit order (dist_idx) and weight table; to honour
// those arguments exactly, one wavefront replays the given order sequentially (the 8
// neighbour terms of a pixel are fetched by 8 lanes, accumulated in order i = 0..7).
// These entry points exist for drop-in completeness and tests; the batched engine uses
// the table-free, level-parallel sweep of prox_ops.h instead.
template <typename T>
__global__ __launch_bounds__(SC_WAVE) void k_host_weighted(T *x, int n, const T *weights, const int *offsets,
                                                           const int *dist_idx, int n_dist, T thresh)
{
    // sequential semantics, parallelised over the 8 neighbours: lane i < 8 fetches one term
    const int lane = threadIdx.x;
    const T one_minus = (T)1 - thresh;
    for (int d = 0; d < n_dist; ++d) {
        const int p = dist_idx[d];
        T term = 0; bool use = false;
        if (lane < 8) {
            const T w = weights[(size_t)lane * n + p];
            if (w > 0) { term = mul_rn(x[p + offsets[lane]], w); use = true; }
        }
        T ref = 0;
        for (int i = 0; i < 8; ++i) {                 // ordered accumulation i = 0..7
            const T ti = __shfl(term, i, SC_WAVE);
            const int ui = __shfl((int)use, i, SC_WAVE);
            if (ui) ref = add_rn(ref, ti);
        }
        if (lane == 0) {
            const T cap = ref * one_minus;
            if (cap < x[p]) x[p] = cap;
        }
        __threadfence();                 // lane 0's store visible to the next step's loads
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ void k_host_nearest(double *x, const int *ref_idx, const int *dist_idx, int n_dist, double thresh)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int d = 0; d < n_dist; ++d) {
        const int p = dist_idx[d];
        const double r = x[ref_idx[p]] * (1 - thresh);
        if (r < x[p]) x[p] = r;
    }
}

template <typename T>
static int dev_alloc_copy(DevBuf &buf, const T *host, size_t count)
{
    DEV_ALLOC(buf, count * sizeof(T) + 16);
    if (host) HIP_TRY(hipMemcpy(buf.p, host, count * sizeof(T), hipMemcpyHostToDevice));
    return SCARLET_OK;
}

template <typename T>
static int host_weighted(T *x, int n, const T *weights, const int *offsets, const int *dist_idx,
                         int n_dist, T thresh)
{
    if (!x || !weights || !offsets || !dist_idx || n <= 0 || n_dist < 0) return set_err(SCARLET_E_ARG, "bad arguments");
    for (int d = 0; d < n_dist; ++d)                       // the reference does not bounds-check (mutable_unchecked)
        if (dist_idx[d] < 0 || dist_idx[d] >= n) return set_err(SCARLET_E_ARG, "dist_idx out of range");
    DevBuf dx, dw, doff, dd;
    int rc;
    if ((rc = dev_alloc_copy(dx, x, n))) return rc;
    if ((rc = dev_alloc_copy(dw, weights, (size_t)8 * n))) return rc;
    if ((rc = dev_alloc_copy(doff, offsets, 8))) return rc;
    if ((rc = dev_alloc_copy(dd, dist_idx, n_dist > 0 ? n_dist : 1))) return rc;
    hipLaunchKernelGGL(k_host_weighted<T>, dim3(1), dim3(SC_WAVE), 0, 0, dx.as<T>(), n, dw.as<T>(), doff.as<int>(),
                       dd.as<int>(), n_dist, thresh);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(x, dx.p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost));
    return SCARLET_OK;
}

extern "C" int scarlet_host_prox_weighted_monotonic_f32(float *x, int n, const float *weights, const int *offsets,
                                                        const int *dist_idx, int n_dist, float thresh)
{ return host_weighted<float>(x, n, weights, offsets, dist_idx, n_dist, thresh); }
extern "C" int scarlet_host_prox_weighted_monotonic_f64(double *x, int n, const double *weights, const int *offsets,
                                                        const int *dist_idx, int n_dist, double thresh)
{ return host_weighted<double>(x, n, weights, offsets, dist_idx, n_dist, thresh); }

extern "C" int scarlet_host_prox_monotonic_f64(double *x, int n, const int *ref_idx, const int *dist_idx,
                                               int n_dist, double thresh)
{
    if (!x || !ref_idx || !dist_idx || n <= 0 || n_dist < 0) return set_err(SCARLET_E_ARG, "bad arguments");
    for (int d = 0; d < n_dist; ++d)
        if (dist_idx[d] < 0 || dist_idx[d] >= n || ref_idx[dist_idx[d]] < 0 || ref_idx[dist_idx[d]] >= n)
            return set_err(SCARLET_E_ARG, "dist_idx / ref_idx out of range");
    DevBuf dx, dr, dd;
    int rc;
    if ((rc = dev_alloc_copy(dx, x, n))) return rc;
    if ((rc = dev_alloc_copy(dr, ref_idx, n))) return rc;
    if ((rc = dev_alloc_copy(dd, dist_idx, n_dist > 0 ? n_dist : 1))) return rc;
    hipLaunchKernelGGL(k_host_nearest, dim3(1), dim3(SC_WAVE), 0, 0, dx.as<double>(), dr.as<int>(), dd.as<int>(), n_dist, thresh);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(x, dx.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return SCARLET_OK;
}

// both overloads of the reference (operators_pybind11.cc:87-88: apply_filter<float>, apply_filter<double>)
template <typename T>
static int host_apply_filter(const T *image, int H, int W, const T *values, const int *y_start, const int *y_end,
                             const int *x_start, const int *x_end, int n, T *result)
{
    if (!image || !result || H <= 0 || W <= 0 || n < 0) return set_err(SCARLET_E_ARG, "bad arguments");
    if (n > 0 && (!values || !y_start || !y_end || !x_start || !x_end)) return set_err(SCARLET_E_ARG, "bad arguments");
    DevBuf di, dv, dr, idx[4];
    const int *hidx[4] = {y_start, y_end, x_start, x_end};
    int rc;
    if ((rc = dev_alloc_copy(di, image, (size_t)H * W))) return rc;
    if ((rc = dev_alloc_copy(dv, values, n > 0 ? n : 1))) return rc;
    if ((rc = dev_alloc_copy(dr, (const T *)nullptr, (size_t)H * W))) return rc;
    for (int i = 0; i < 4; ++i) if ((rc = dev_alloc_copy(idx[i], hidx[i], n > 0 ? n : 1))) return rc;
    hipLaunchKernelGGL(k_apply_filter<T>, dim3((H * W + SC_BLOCK - 1) / SC_BLOCK), dim3(SC_BLOCK), 0, (hipStream_t)0,
                       di.as<T>(), H, W, dv.as<T>(), idx[0].as<int>(), idx[1].as<int>(), idx[2].as<int>(), idx[3].as<int>(),
                       n, dr.as<T>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(result, dr.p, (size_t)H * W * sizeof(T), hipMemcpyDeviceToHost));
    return SCARLET_OK;
}
extern "C" int scarlet_host_apply_filter_f32(const float *image, int H, int W, const float *values,
                                             const int *y_start, const int *y_end, const int *x_start,
                                             const int *x_end, int n, float *result)
{
    return host_apply_filter<float>(image, H, W, values, y_start, y_end, x_start, x_end, n, result);
}
extern "C" int scarlet_host_apply_filter_f64(const double *image, int H, int W, const double *values,
                                             const int *y_start, const int *y_end, const int *x_start,
                                             const int *x_end, int n, double *result)
{
    return host_apply_filter<double>(image, H, W, values, y_start, y_end, x_start, x_end, n, result);
}

// =====================================================================================
// 3. batched Blend.fit() engine
// =====================================================================================
// ---- optional per-kernel event timing (scarlet_profile_begin/end)
#define SC_NCLASS 8
struct Profiler {
    std::atomic<bool> on{false};
    std::vector<hipEvent_t> ev;     // pairs (start, stop)
    std::vector<int> cls, weight;   // weight: iterations one launch covers (k_fit2: several)
    int used = 0, cap = 0;
};
static Profiler g_prof;                // process-wide: one profiled fit at a time (documented in the header)
static std::mutex g_prof_mu;
static inline void prof_start(int cls, hipStream_t st, int weight = 1)
{
    if (!g_prof.on) return;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (g_prof.on && g_prof.used < g_prof.cap) {
        g_prof.cls[g_prof.used] = cls;
        g_prof.weight[g_prof.used] = weight;
        (void)hipEventRecord(g_prof.ev[2 * g_prof.used], st);
    }
}
static inline void prof_stop(hipStream_t st)
{
    if (!g_prof.on) return;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (g_prof.on && g_prof.used < g_prof.cap) {
        (void)hipEventRecord(g_prof.ev[2 * g_prof.used + 1], st);
        ++g_prof.used;
    }
}
extern "C" int scarlet_profile_begin(int max_iterations)
{
    if (max_iterations <= 0) return set_err(SCARLET_E_ARG, "max_iterations <= 0");
    std::lock_guard<std::mutex> lock(g_prof_mu);
    for (auto e : g_prof.ev) (void)hipEventDestroy(e);
    const int cap = max_iterations * 16;                 // (two half-batches per iteration when scarlet_fit pipelines them)
    g_prof.ev.assign((size_t)cap * 2, nullptr);
    g_prof.cls.assign(cap, 0);
    g_prof.weight.assign(cap, 1);
    for (auto &e : g_prof.ev) HIP_TRY(hipEventCreate(&e));
    g_prof.cap = cap; g_prof.used = 0; g_prof.on = true;
    return SCARLET_OK;
}
extern "C" int scarlet_profile_end_ex(double total_ms[SC_NCLASS], int64_t iterations[SC_NCLASS], int64_t launches[SC_NCLASS])
{
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (!g_prof.on) return set_err(SCARLET_E_ARG, "profiler not active");
    if (!total_ms) return set_err(SCARLET_E_ARG, "null total_ms");
    g_prof.on = false;
    for (int k = 0; k < SC_NCLASS; ++k) { total_ms[k] = 0; if (iterations) iterations[k] = 0; if (launches) launches[k] = 0; }
    for (int i = 0; i < g_prof.used; ++i) {
        HIP_TRY(hipEventSynchronize(g_prof.ev[2 * i + 1]));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]));
        total_ms[g_prof.cls[i]] += ms;
        if (iterations) iterations[g_prof.cls[i]] += g_prof.weight[i];
        if (launches) launches[g_prof.cls[i]] += 1;
    }
    for (auto e : g_prof.ev) (void)hipEventDestroy(e);
    g_prof.ev.clear(); g_prof.cls.clear(); g_prof.weight.clear(); g_prof.cap = g_prof.used = 0;
    return SCARLET_OK;
}
extern "C" int scarlet_profile_end(double total_ms[SC_NCLASS], int64_t launches[SC_NCLASS])
{
    return scarlet_profile_end_ex(total_ms, launches, nullptr);
}

// shape and limits alone: nothing here reads a pointer of the batch
// bmax: SC_BMAX everywhere but for the state of a wide entry point (SC_CMAX, multiobs_wide.h)
static int check_shape(const scarlet_batch *b, int bmax = SC_BMAX)
{
    if (!b) return set_err(SCARLET_E_ARG, "null batch");
    if (b->S <= 0 || b->K <= 0 || b->B <= 0 || b->H <= 0 || b->W <= 0) return set_err(SCARLET_E_ARG, "bad batch shape");
    if (b->K > SCARLET_MAX_COMPONENTS)
        return set_err(SCARLET_E_NOTIMPL, "K > 256 components per scene (SCARLET_MAX_COMPONENTS) is not supported");
    if (b->B > bmax)
        return set_err(SCARLET_E_NOTIMPL, bmax > SC_BMAX ? "a model frame of more than 32 channels (SCARLET_MAX_CHANNELS) is not supported"
                                                         : "B > 8 bands is not supported by this build of the gradient kernels");
    if (b->H > SCARLET_MAX_SIDE || b->W > SCARLET_MAX_SIDE)
        return set_err(SCARLET_E_TOO_LARGE, "frames larger than 1024 x 1024 (SCARLET_MAX_SIDE) are not supported");
    return SCARLET_OK;
}
static int check_batch(const scarlet_batch *b, int bmax = SC_BMAX)
{
    // Every entry point ends with a look at hipGetLastError(); that value is per thread and keeps whatever an EARLIER HIP
    // call of the thread left there.  Start from a clean slate: what is reported is ours.
    (void)hipGetLastError();
    const int rc = check_shape(b, bmax);
    if (rc) return rc;
    if (!b->images || !b->sed[0] || !b->sed[1] || !b->morph[0] || !b->morph[1] || !b->cur || !b->centers ||
        !b->shifts || !b->flags || !b->lipschitz || !b->mse || !b->it || !b->active || !b->status || !b->workspace)
        return set_err(SCARLET_E_ARG, "null pointer in batch");
    if (b->symmetric && (!b->centroid_psf || b->centroid_P <= 0 || !(b->centroid_P & 1)))
        return set_err(SCARLET_E_ARG, "symmetric pipeline needs an odd-sized centroid psf");
    return SCARLET_OK;
}

// ---- per-component constraint switches (scarlet_constraints).  Inside the library `c` may be NULL: the batch's scalars.
static bool cons_any(const scarlet_constraints *c) { return c && (c->symmetric || c->monotonic || c->l0_thresh || c->l1_thresh); }
static int check_prior(const scarlet_prior *p)
{
    if (!p) return set_err(SCARLET_E_ARG, "null prior");
    if (!p->L_comp) return set_err(SCARLET_E_ARG, "prior: L_comp is NULL (required output)");
    if (p->quad_sed_target && !p->quad_sed_weight) return set_err(SCARLET_E_ARG, "prior: quad_sed_target without quad_sed_weight");
    if (p->quad_morph_target && !p->quad_morph_weight)
        return set_err(SCARLET_E_ARG, "prior: quad_morph_target without quad_morph_weight");
    return SCARLET_OK;
}
// The host-side check of every entry point that steps, updates or fits, before anything is launched.
// need_c: a _constrained entry point (the struct is required, and a symmetric array needs what b->symmetric needs);
// need_p: a _prior entry point (`p` is checked whenever it is given);  max_iter: of the loops, 0 elsewhere
static int check_call(const scarlet_batch *b, bool need_c, const scarlet_constraints *c, bool need_p, const scarlet_prior *p,
                      int max_iter = 0, int bmax = SC_BMAX)
{
    if (!b) return set_err(SCARLET_E_ARG, "null batch");
    if (need_c && !c) return set_err(SCARLET_E_ARG, "constraints is NULL (pass a scarlet_constraints with NULL members for the batch's scalars)");
    if (need_c && c->symmetric && (!b->centroid_psf || b->centroid_P <= 0 || !(b->centroid_P & 1)))
        return set_err(SCARLET_E_ARG, "constraints.symmetric needs an odd-sized centroid_psf");
    int rc = check_batch(b, bmax);
    if (!rc && (need_p || p)) rc = check_prior(p);
    if (!rc && max_iter < 0) rc = set_err(SCARLET_E_ARG, "max_iter < 0");
    return rc;
}
// the arrays advanced to component `first` (split_views: a half-batch's first component)
static scarlet_constraints cons_view(const scarlet_constraints *c, size_t first)
{
    scarlet_constraints v = {};
    if (!c) return v;
    v.symmetric = c->symmetric ? c->symmetric + first : nullptr;
    v.monotonic = c->monotonic ? c->monotonic + first : nullptr;
    v.l0_thresh = c->l0_thresh ? c->l0_thresh + first : nullptr;
    v.l1_thresh = c->l1_thresh ? c->l1_thresh + first : nullptr;
    return v;
}

// Ragged batches: one small kernel per call of an entry point that iterates or initialises.  A scene whose count lies
// outside 1..K gets SCARLET_STATUS_BAD_COUNT and active = 0; the kernels then see no component of it (scene_ncomp).
__global__ void k_check_counts(const int *ncomp, int S, int K, int *status, int *active)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int n = ncomp[s];
    if (n < 1 || n > K) { status[s] |= SCARLET_STATUS_BAD_COUNT; active[s] = 0; }
}
static int check_counts(const scarlet_batch *b, void *stream)
{
    if (!b->n_components) return SCARLET_OK;
    hipLaunchKernelGGL(k_check_counts, dim3((b->S + SC_BLOCK - 1) / SC_BLOCK), dim3(SC_BLOCK), 0, (hipStream_t)stream,
                       b->n_components, b->S, b->K, b->status, b->active);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}

// Ragged frames: the same for frame_hw, before any kernel reads a plane.  A scene whose entry lies outside 1..H x 1..W
// gets SCARLET_STATUS_BAD_FRAME and active = 0.  The kernels that read frame_hw test the entry again themselves
// (frame_ok, engine.h) and return before they touch a plane, so no entry beyond the padded plane is ever a loop bound --
// also in the constructors' update, which ignores `active`.
__global__ void k_check_frames(const int *frame_hw, int S, int H, int W, int *status, int *active)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int h = frame_hw[2 * s], w = frame_hw[2 * s + 1];
    if (h < 1 || h > H || w < 1 || w > W) { status[s] |= SCARLET_STATUS_BAD_FRAME; active[s] = 0; }
}
static int check_frames(const scarlet_batch *b, const int32_t *frame_hw, void *stream)
{
    if (!frame_hw) return SCARLET_OK;
    hipLaunchKernelGGL(k_check_frames, dim3((b->S + SC_BLOCK - 1) / SC_BLOCK), dim3(SC_BLOCK), 0, (hipStream_t)stream,
                       (const int *)frame_hw, b->S, b->H, b->W, b->status, b->active);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}
// ---- update options (scarlet_update_options).  Inside the library `o` may be NULL, and one with every member NULL counts
// as none: the stock pipeline, the kernels and the paths of a batch without options.
static bool opts_any(const scarlet_update_options *o)
{
    return o && (o->sym_algorithm || o->sym_strength || o->mono_nearest || o->mono_thresh || o->positive || o->normalize);
}
template <> constexpr bool has_update_options<scarlet_update_options> = true;      // (comp_options reads the struct itself)
// One thread per scene, before anything else of the call: a scene one of whose present components has an inadmissible row
// (options_ok, engine.h; a `positive` beyond its two bits) gets SCARLET_STATUS_BAD_OPTION and active = 0.  The rows of
// inactive scenes (respect_active: the calls that iterate), of scenes a constructor call leaves alone (skip_status) and of
// absent components are not read.  also_status: an inactive scene with one of these bits is checked all the same
// (SCARLET_STATUS_BAD_FRAME with ragged frames: the frame check in front deactivates a scene, which then carries both bits).
__global__ void k_check_options(scarlet_update_options o, const int *ncomp, int S, int K, int respect_active, int skip_status,
                                int also_status, int *status, int *active)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    if (respect_active && !active[s] && !(status[s] & also_status)) return;
    if (skip_status && (status[s] & skip_status)) return;
    const int n = scene_ncomp(ncomp, s, K);
    bool ok = true;
    for (int k = 0; k < n; ++k) {
        const int c = s * K + k;
        ok = ok && options_ok(comp_options(o, c)) && !(o.positive && o.positive[c] > (SCARLET_POSITIVE_SED | SCARLET_POSITIVE_MORPH));
    }
    if (!ok) { status[s] |= SCARLET_STATUS_BAD_OPTION; active[s] = 0; }
}
static int check_options(const scarlet_batch *b, const scarlet_update_options *o, int respect_active, int skip_status, void *stream,
                         int also_status = 0)
{
    if (!opts_any(o)) return SCARLET_OK;
    hipLaunchKernelGGL(k_check_options, dim3((b->S + SC_BLOCK - 1) / SC_BLOCK), dim3(SC_BLOCK), 0, (hipStream_t)stream,
                       *o, (const int *)b->n_components, b->S, b->K, respect_active, skip_status, also_status, b->status, b->active);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}
// ... and for the `dims` table of a low-resolution observation of such scenes (scarlet_lowres_frames): a row outside
// 1..max in any column (max6: H, W, h, w, nfy, nfx of the padded blocks), or whose H_s, W_s are not frame_hw[s], marks
// the scene the same way.  k_lowres_planes_frames and k_lowres_products_frames test the row again (lr_scene_dims).
__global__ void k_check_lowres_frames(const int *dims, const int *frame_hw, int S, LowresDims max6, int *status, int *active)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int *q = dims + 6 * (size_t)s;
    const int mx[6] = {max6.H, max6.W, max6.h, max6.w, max6.nfy, max6.nfx};
    bool bad = q[0] != frame_hw[2 * s] || q[1] != frame_hw[2 * s + 1];
    for (int i = 0; i < 6; ++i) bad = bad || q[i] < 1 || q[i] > mx[i];
    if (bad) { status[s] |= SCARLET_STATUS_BAD_FRAME; active[s] = 0; }
}
static int check_lowres_frames(const scarlet_batch *b, const scarlet_lowres_frames *lf, const int32_t *frame_hw,
                               const LowresDims &max6, void *stream)
{
    hipLaunchKernelGGL(k_check_lowres_frames, dim3((b->S + SC_BLOCK - 1) / SC_BLOCK), dim3(SC_BLOCK), 0, (hipStream_t)stream,
                       (const int *)lf->dims, (const int *)frame_hw, b->S, max6, b->status, b->active);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}
// the host-side check of the _frames entry points, after check_call: the struct, and what a ragged-frame batch does not take
static int check_frames_call(const scarlet_batch *b, const scarlet_frames *f)
{
    if (!f) return set_err(SCARLET_E_ARG, "frames is NULL (pass a scarlet_frames with frame_hw = NULL for uniform frames)");
    if (f->frame_hw && b->group) return set_err(SCARLET_E_NOTIMPL, "frame_hw (ragged frames) with group: not implemented");
    return SCARLET_OK;
}

static int n_tiles(const scarlet_batch *b) { return (b->H * b->W + SC_TILE_PIX - 1) / SC_TILE_PIX; }

// ---- PSF path geometry (fft.py:68-106: next_fast_len(N + P + 3) per axis, last axis even)
// FFT shape of the device convolution.  The reference pads to next_fast_len(N + P + 3)
// (fft.py:68-106: 5-smooth, 3 pixels of slack); the cropped result is the LINEAR convolution, which
// any length >= N + P - 1 reproduces exactly, so the device takes the smallest 7-smooth length from
// there (rocFFT has radix-7 kernels: 168 x 168 instead of 180 x 180 for a 128 x 128 frame with a
// 41 x 41 kernel is 1.56 x faster per transform pair, measured).  Last axis even for the R2C layout.
static int smooth7_len(int n, bool even)
{
    for (int m = n;; ++m) {
        if (even && (m & 1)) continue;
        int r = m;
        for (int p : {2, 3, 5, 7}) while (r % p == 0) r /= p;
        if (r == 1) return m;
    }
}
static PsfGeom psf_geom(int H, int W, int Py, int Px)
{
    PsfGeom g;
    g.H = H; g.W = W;
    g.Fy = smooth7_len(H + Py - 1, false);
    g.Fx = smooth7_len(W + Px - 1, true);
    // placement of image and kernel inside the reference's padded arrays (centred pad + ifftshift,
    // fft.py:27-66): only these parities decide which pixel of an even-sized kernel is its centre
    g.Fry = scarlet_next_fast_len(H + Py + 3);
    g.Frx = scarlet_next_fast_len(W + Px + 3);
    while (g.Frx & 1) g.Frx = scarlet_next_fast_len(g.Frx + 1);
    g.Fxh = g.Fx / 2 + 1;
    g.oy = (g.Fry - H + 1) / 2 - g.Fry / 2;
    g.ox = (g.Frx - W + 1) / 2 - g.Frx / 2;
    return g;
}
static int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }
// ---- LDS-resident convolution (fftconv.h): plan = lengths, radices, kernel placement
// smallest circular length that reproduces the cropped linear convolution: image at 0..N-1, kernel at
// (q + o) mod F, output read at 0..N-1 (o <= 0 is the kernel's offset in the reference's padded array)
static int fft_len_min(int N, int P, int o)
{
    int m = P + N - 1 + o;
    if (N - o > m) m = N - o;
    if (N > m) m = N;
    if (P > m) m = P;
    return m;
}
// smallest L = r1 r2 >= Lmin with both radices on the menu; ties: odd r2 first when `prefer_odd_r2`
// (the contiguous run of pass B, bank conflicts), then the more balanced pair
static bool fft_choose(int Lmin, bool prefer_odd_r2, int *L, int *r1, int *r2)
{
    static const int menu[] = {4, 5, 6, 7, 8, 9, 10, 12, 14, 15, 16};
    long best = -1;
    for (int a : menu)
        for (int b : menu) {
            const int l = a * b;
            if (l < Lmin) continue;
            const int bal = a > b ? a - b : b - a;
            const long score = (long)l * 1000 + ((prefer_odd_r2 && !(b & 1)) ? 100 : 0) + bal;
            if (best < 0 || score < best) { best = score; *L = l; *r1 = a; *r2 = b; }
        }
    return best >= 0;
}
// plan for an H x W image and a Py x Px kernel; false when no menu length fits or the plane exceeds LDS
static bool fft_make_plan(int H, int W, int Py, int Px, FftPlan *p)
{
    const PsfGeom g = psf_geom(H, W, Py, Px);         // reference FFT shape -> kernel offsets
    const int oky = (g.Fry - Py + 1) / 2 - g.Fry / 2, okx = (g.Frx - Px + 1) / 2 - g.Frx / 2;
    const int Fy_min = fft_len_min(H, Py, oky), Fx_min = fft_len_min(W, Px, okx);
    int Fy, M, r1y, r2y, r1x, r2x;
    if (!fft_choose(Fy_min, false, &Fy, &r1y, &r2y)) return false;
    if (!fft_choose((Fx_min + 1) / 2, true, &M, &r1x, &r2x)) return false;
    p->H = H; p->W = W; p->Fy = Fy; p->Fx = 2 * M; p->M = M; p->RS = M + 1;
    // (A row stride == R2x (mod 32) -- 85 instead of 81 for BASELINE config 3 -- was tried so that the bank windows of
    // consecutive lines tile in the row passes: SQ_LDS_BANK_CONFLICT rose from 0.76e8 to 1.10e8 per launch and the
    // iteration took 8.19 ms instead of 8.00; the plane keeps its dense stride.  profiles/r03_notes.md)
    p->R1y = r1y; p->R2y = r2y; p->R1x = r1x; p->R2x = r2x;
    p->Py = Py; p->Px = Px; p->oky = oky; p->okx = okx;
    p->scale = (float)(1.0 / ((double)M * (double)Fy));
    p->tables = nullptr;
    p->stagger_wgs = 0;
    p->dma_image = 0;
    p->tab_off = fft_tab_off(Fy, p->RS, H, W, false);
    return fft_lds_bytes(Fy, M, p->RS) <= LDS_LIMIT - 4096;
}
// twiddle / permutation tables of a plan, float64 -> float32 (layout: fftconv.h FftPlan::tables)
static void fft_fill_tables(const FftPlan &p, std::vector<float2> &t)
{
    const double tau = 6.283185307179586476925286766559;
    const int NP = p.M / 2 + 1;
    t.assign(fft_table_float2s(p.Fy, p.M), make_float2(0.f, 0.f));
    // a twiddle w = c + i s is stored as (c, s, -s, s): fftconv.h cmul_t
    struct Tw4 { float c, s, ns, s2; };
    auto tw = [&](double num, double den) {
        const float c = (float)cos(tau * num / den), sn = (float)-sin(tau * num / den);
        return Tw4{c, sn, -sn, sn};
    };
    Tw4 *twy = (Tw4 *)t.data(), *twm = twy + p.Fy, *twx = twm + p.M, *twp = twx + NP;
    for (int j = 0; j < p.Fy; ++j) twy[j] = tw(j, p.Fy);
    for (int j = 0; j < p.M; ++j) twm[j] = tw(j, p.M);
    for (int k = 0; k < NP; ++k) twx[k] = tw(k, p.Fx);
    unsigned short *posx = (unsigned short *)(twp + NP);
    for (int k = 0; k < p.M; ++k) posx[k] = (unsigned short)(p.R2x * (k % p.R1x) + k / p.R1x);
    // the column pairs (k, M - k), k = 0 .. M/2, in the order of their first member's position (fftconv.h FftPair)
    FftPair *pair = (FftPair *)(t.data() + 2 * (p.Fy + p.M + 2 * NP) + (p.M + 3) / 4);
    std::vector<int> order(NP);
    for (int k = 0; k < NP; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return posx[a] < posx[b]; });
    for (int i = 0; i < NP; ++i) {
        const int k = order[i];
        const bool first = k == 0, mid = 2 * k == p.M;
        const int ra = posx[k], rb = (first || mid) ? ra : posx[p.M - k];
        pair[i].ra = (unsigned short)ra; pair[i].rb = (unsigned short)rb;
        pair[i].cb = (unsigned short)(first ? p.M : rb); pair[i].pad = 0;
        twp[i] = twx[k];
    }
}
static bool psf_lds_possible(const scarlet_batch *b, FftPlan *p)
{
    if (b->W & 1) return false;                       // k_psf_conv reads pixel pairs (float2)
    return fft_make_plan(b->H, b->W, b->psf_h, b->psf_w, p);
}

// k_psf_conv's view of the plan: where the image is staged; true when the exact-shape instance applies
static bool psf_conv_finish_plan(const scarlet_batch *b, FftPlan *fp)
{
    // the image plane is staged in LDS by LDS-DMA when it fits behind the H data rows (16-byte pieces)
    fp->dma_image = ((b->H * b->W) % 4 == 0 &&
                     fft_lds_bytes(fp->Fy, fp->M, fp->RS, b->H, b->W, true) <= LDS_LIMIT - 1024) ? 1 : 0;
    fp->tab_off = fft_tab_off(fp->Fy, fp->RS, b->H, b->W, fp->dma_image != 0);
    // BASELINE config 3's plan has an exact-shape instance with 1024 threads per workgroup (fftconv.h)
    return fp->H == 128 && fp->W == 128 && fp->Fy == 150 && fp->Fx == 150 && fp->M == 75 && fp->RS == 76 && fp->R1y == 10 &&
           fp->R2y == 15 && fp->R1x == 5 && fp->R2x == 15 && fp->dma_image == 1 && !opt(OPT_NO_EXACT);
}

// ---- the workspace: one device buffer, allocated by the caller (scarlet_batch_workspace_bytes) and zeroed once, holds
// every kernel's scratch.  ws_layout() is the one place that decides which regions a batch has and where they lie;
// every size and pointer comes from its result, computed once per entry-point call and passed down.
// Which PSF convolution runs is a function of the shapes alone -- the LDS-resident transform whenever the half-spectrum
// plane fits LDS, batched hipFFT otherwise (frames beyond ~150 + P pixels) -- except for the diagnostic switch
// PSF_HIPFFT, which forces the library path.
enum { GRAD_SMALL, GRAD_BIGK, GRAD_HUGEK };    // gradient step: K <= 8 (engine.h), chunks of eight (bigk.h), hugek.h
struct WsLayout {
    // the decisions that size regions
    int grad;                           // GRAD_HUGEK: K > 32, and 8 < K <= 32 under FORCE_HUGEK
    bool psf;                           // a diff_kernel of psf_h x psf_w (has_psf)
    bool psf_lds;                       // its convolution runs in LDS (`plan`); false: batched hipFFT (`geom`)
    bool has_gscratch, has_kscache;
    bool split;                         // two half-batch pipelines are possible (split_views)
    PsfGeom geom;
    FftPlan plan;
    int n0;                             // (split) scenes of the first half
    // byte offsets of the base area
    int64_t partials;                   // per-tile partials [S][T][P] (float64); at 0 for tools/stamps.py, tools/occupancy.py
    int64_t conv;                       // convergence sums [S][K][4] (float64); scarlet_fit_multi's Lipschitz sums
    int64_t box_fallback;               // per component: 1 = k_source_update_box left it to the full-frame kernel (int)
    int64_t box_list, box_count;        // the components the small box left to the large one [S * K], their number (int)
    int64_t gplanes;                    // K > 8: G = w^2 (model - image) [S][B][H][W] (float32)
    int64_t gscratch;                   // frames whose tile does not fit LDS: the k-space symmetry's GEMM scratch per component
    int64_t kscache;                    // k_iterate2's cache of the k-space symmetry's Hankel vectors (fused2.h); zero = empty
    int64_t gpart, gram, msq[2];        // hugek.h (float64): Gram blocks [S][pairs][C][32][32]; G and the two squaring
                                        // buffers [S][Kp][Kp]
    int64_t fit2x_queue;                // k_fit2x's scene queue (int)
    int64_t active_count;               // active scenes, counted for the host (int)
    int64_t base_end;
    // byte offsets of the PSF area
    int64_t loss;                       // per-plane loss sums [S][B] (float64)
    int64_t real;                       // hipFFT: padded planes [S][B][Fy][Fx]; LDS: compact gradient planes G [S][B][H][W]
    int64_t spec, khat;                 // hipFFT: spectra of the planes and of the kernels (float2)
    int64_t lds_khat, lds_tables;       // LDS: spectra of the kernels, twiddle / permutation tables (float2)
    int64_t stamps;                     // LDS under STAMPS: k_psf_conv's phase stamps [S][B][32] (int64)
    int64_t half[2];                    // (split) the workspace of each half-batch
    int64_t total;
};
static bool has_psf(const scarlet_batch *b) { return b->diff_kernel && b->psf_h > 0 && b->psf_w > 0; }
// How a call uses the layout.  WS_FIX: on a live batch -- the switches that placed its regions (FORCE_HUGEK for
// 8 < K <= 32, PSF_HIPFFT and STAMPS for a PSF batch) stay fixed from then on (see scarlet_set_option).  WS_PEEK: the
// call only reports, or reads regions no switch moves.  WS_HALF: one half of a split batch (no halves of its own).
enum LayoutUse { WS_PEEK, WS_FIX, WS_HALF };
static WsLayout ws_layout(const scarlet_batch *b, LayoutUse use)
{
    WsLayout l = {};
    const int64_t S = b->S, K = b->K, B = b->B, HW = (int64_t)b->H * b->W;
    int64_t at = 0;
    auto place = [&at](int64_t bytes) { const int64_t o = at; at += bytes; return o; };
    if (use == WS_FIX && K > SC_KMAX && K <= SC_KBIG) g_hugek_frozen.store(true);
    l.grad = K <= SC_KMAX ? GRAD_SMALL : (K > SC_KBIG || opt(OPT_FORCE_HUGEK)) ? GRAD_HUGEK : GRAD_BIGK;
    l.has_gscratch = update_plan(b->H, b->W, {}).reserve_gscratch;
    l.has_kscache = K <= 4 && B <= 5 && b->H <= 64 && b->W <= 64;
    l.partials = place(sizeof(double) * S * n_tiles(b) * n_partials(b->K, b->B));
    l.conv = place(sizeof(double) * S * K * 4);
    l.box_fallback = place(sizeof(int) * S * K);
    l.box_list = place(sizeof(int) * S * K);
    l.box_count = place(sizeof(int) * 64);             // (the count, then 63 spare ints)
    at = align256(at);
    l.gplanes = place(l.grad != GRAD_SMALL ? align256(sizeof(float) * S * B * HW) : 0);
    l.gscratch = place(l.has_gscratch ? align256(sizeof(float) * S * K * round16(b->H) * scratch_stride(round16(b->W))) : 0);
    l.kscache = place(l.has_kscache ? align256(sizeof(float) * S * K * 2 * SC_KSC_FLOATS) : 0);
    const bool huge = l.grad == GRAD_HUGEK;
    const int64_t Kp = (int64_t)huge_nblk(b->K) * SC_GBLK, gram = huge ? align256(sizeof(double) * S * Kp * Kp) : 0;
    l.gpart = place(huge ? align256(sizeof(double) * S * huge_npairs(b->K) * huge_nchunks(b->H * b->W) * SC_GBLK * SC_GBLK) : 0);
    l.gram = place(gram);
    l.msq[0] = place(gram);
    l.msq[1] = place(gram);
    const int64_t words = place(256);                  // the base area ends in 256 bytes that hold two words
    l.fit2x_queue = words + 128;
    l.active_count = words + 192;
    l.base_end = l.total = at;
    l.psf = has_psf(b);
    if (!l.psf) return l;

    if (use == WS_FIX) g_layout_frozen.store(true);
    const int64_t planes = S * B, nk = b->diff_kernel_per_scene ? planes : B;
    l.geom = psf_geom(b->H, b->W, b->psf_h, b->psf_w);
    const PsfGeom &g = l.geom;
    const FftPlan &p = l.plan;
    const bool lds_possible = psf_lds_possible(b, &l.plan);
    l.psf_lds = lds_possible && !opt(OPT_PSF_HIPFFT);
    const bool fft = !l.psf_lds;
    l.loss = place(align256(planes * (int64_t)sizeof(double)));
    l.real = place(align256(planes * (fft ? (int64_t)g.Fy * g.Fx : HW) * (int64_t)sizeof(float)));
    l.spec = place(fft ? align256(planes * g.Fy * g.Fxh * (int64_t)sizeof(float2)) : 0);
    l.khat = place(fft ? align256(nk * g.Fy * g.Fxh * (int64_t)sizeof(float2)) : 0);
    l.lds_khat = place(l.psf_lds ? align256(nk * p.Fy * (p.M + 1) * (int64_t)sizeof(float2)) : 0);
    l.lds_tables = place(l.psf_lds ? align256(fft_table_float2s(p.Fy, p.M) * (int64_t)sizeof(float2)) : 0);
    l.stamps = place((l.psf_lds && opt(OPT_STAMPS)) ? align256(planes * 32 * (int64_t)sizeof(long long)) : 0);
    place(256);
    // the regions of the halves follow (there under PSF_HIPFFT too, which runs one pipeline)
    l.split = use != WS_HALF && K <= SC_KMAX && S >= 1024 && !b->group && HW % 4 == 0 && lds_possible;
    if (l.split) {
        scarlet_batch h = *b;
        h.S = l.n0 = ((b->S / 2 + 7) / 8) * 8;        // (the convolution maps groups of eight scenes to the XCDs)
        l.half[0] = place(align256(ws_layout(&h, WS_HALF).total));
        h.S = b->S - l.n0;
        l.half[1] = place(ws_layout(&h, WS_HALF).total);
    }
    l.total = at;
    return l;
}
template <typename T> static T *ws_at(const scarlet_batch *b, int64_t offset) { return (T *)((char *)b->workspace + offset); }

// ---- two half-batches on two streams (scarlet_fit with a PSF, LDS-resident transform, K <= 8).
// The convolution kernel is bound by the latency of its passes at one workgroup per CU and moves under 1 TB/s;
// the passes around it (model planes, gradient step, constraints) stream at HBM rate and hardly use the ALUs.
// Scenes are independent, so scarlet_fit runs the two halves of a large batch as two pipelines, the second on the
// calling thread's second stream: one half's convolution overlaps the other half's streaming passes.  Each half
// is a VIEW of the batch (every per-scene array advanced to its first scene) with its own workspace region behind
// the batch's (its own K-hat and tables, prepared with the batch's): the kernels do not know.
static bool two_pipelines(const WsLayout &l)
{
    return l.split && l.psf_lds && !opt(OPT_NO_PIPELINE) && !opt(OPT_NO_SIDE_STREAM);
}
static scarlet_batch batch_view(const scarlet_batch *b, int s0, int n, void *ws)
{
    scarlet_batch v = *b;
    const size_t HW = (size_t)b->H * b->W, K = b->K, B = b->B;
    v.S = n;
    v.images += s0 * B * HW;
    if (v.weights) v.weights += s0 * B * HW;
    for (int i = 0; i < 2; ++i) { v.sed[i] += s0 * K * B; v.morph[i] += s0 * K * HW; }
    v.cur += s0; v.centers += s0 * K * 2; v.shifts += s0 * K * 2; v.flags += s0 * K;
    if (v.fix_sed) v.fix_sed += s0 * K;
    if (v.fix_morph) v.fix_morph += s0 * K;
    v.lipschitz += 2 * (size_t)s0; v.mse += (size_t)s0 * b->mse_capacity; v.it += s0; v.active += s0; v.status += s0;
    if (v.diff_kernel_per_scene) v.diff_kernel += s0 * B * (size_t)b->psf_h * b->psf_w;
    if (v.group) v.group += s0 * K;
    if (v.n_components) v.n_components += s0;
    v.workspace = ws;
    return v;
}
static void split_views(const scarlet_batch *b, const WsLayout &l, scarlet_batch v[2], WsLayout lv[2],
                        const scarlet_constraints *c, scarlet_constraints cv[2])
{
    v[0] = batch_view(b, 0, l.n0, ws_at<char>(b, l.half[0]));
    v[1] = batch_view(b, l.n0, b->S - l.n0, ws_at<char>(b, l.half[1]));
    cv[0] = cons_view(c, 0);
    cv[1] = cons_view(c, (size_t)l.n0 * b->K);
    for (int h = 0; h < 2; ++h) lv[h] = ws_layout(&v[h], WS_HALF);
}

// diagnostics: the plan of the LDS-resident convolution for this batch, 16 ints {H, W, Fy, Fx, M, RS, R1y, R2y, R1x, R2x,
// oky, okx, dma_image, exact-shape instance, LDS bytes, 0}; returns 0, or -1 when the batch takes another path
extern "C" int scarlet_debug_psf_plan(const scarlet_batch *b, int32_t *out16)
{
    if (!b || !out16) return -1;
    const WsLayout l = ws_layout(b, WS_PEEK);
    if (!l.psf_lds) return -1;
    FftPlan p = l.plan;
    const bool x = psf_conv_finish_plan(b, &p);
    const int v[16] = {p.H, p.W, p.Fy, p.Fx, p.M, p.RS, p.R1y, p.R2y, p.R1x, p.R2x, p.oky, p.okx, p.dma_image, x ? 1 : 0,
                       (int)fft_lds_bytes(p.Fy, p.M, p.RS, b->H, b->W, p.dma_image != 0), 0};
    for (int i = 0; i < 16; ++i) out16[i] = v[i];
    return 0;
}

// diagnostics (STAMPS switch): byte offset, inside the batch's workspace, of k_psf_conv's phase stamps
// ([S][B][32] int64 shader-clock values), or -1 when the batch has none
extern "C" int64_t scarlet_debug_psf_stamps_offset(const scarlet_batch *b)
{
    if (!b || !opt(OPT_STAMPS) || !ws_layout(b, WS_PEEK).psf_lds) return -1;
    return ws_layout(b, WS_FIX).stamps;               // (only a batch that has stamps fixes the switches)
}

extern "C" int scarlet_batch_pipelines(const scarlet_batch *b)
{
    if (!b) return 0;
    return two_pipelines(ws_layout(b, WS_PEEK)) ? 2 : 1;
}

extern "C" int64_t scarlet_batch_workspace_bytes(const scarlet_batch *b)
{
    return b ? ws_layout(b, WS_FIX).total : 0;
}

static GradArgs grad_args(const scarlet_batch *b, const WsLayout &l, int approximate_L, int raw_gradient)
{
    GradArgs a;
    a.S = b->S; a.K = b->K; a.B = b->B; a.HW = b->H * b->W; a.T = n_tiles(b);
    a.images = b->images; a.weights = b->weights; a.weight_scalar = b->weight_scalar;
    a.sed[0] = b->sed[0]; a.sed[1] = b->sed[1]; a.morph[0] = b->morph[0]; a.morph[1] = b->morph[1];
    a.cur = b->cur; a.fix_sed = b->fix_sed; a.fix_morph = b->fix_morph;
    a.partials = ws_at<double>(b, l.partials); a.lipschitz = b->lipschitz; a.mse = b->mse; a.mse_capacity = b->mse_capacity;
    a.it = b->it; a.active = b->active; a.approximate_L = approximate_L; a.raw_gradient = raw_gradient;
    a.ncomp = b->n_components;
    return a;
}

// ---- hipFFT plan cache: one (R2C, C2R) pair per (Fy, Fx, batch)
struct FftPlans { hipfftHandle r2c, c2r; };
static std::map<std::tuple<int, int, int>, FftPlans> g_plans;
static std::mutex g_plans_mu;          // guards the map; a plan's stream is set and used under g_fft_exec_mu
static std::mutex g_fft_exec_mu;
static int get_plans(int Fy, int Fx, int batch, FftPlans *out)
{
    std::lock_guard<std::mutex> lock(g_plans_mu);
    auto key = std::make_tuple(Fy, Fx, batch);
    auto it = g_plans.find(key);
    if (it == g_plans.end()) {
        FftPlans p;
        int n[2] = {Fy, Fx};
        if (hipfftPlanMany(&p.r2c, 2, n, nullptr, 1, 0, nullptr, 1, 0, HIPFFT_R2C, batch) != HIPFFT_SUCCESS ||
            hipfftPlanMany(&p.c2r, 2, n, nullptr, 1, 0, nullptr, 1, 0, HIPFFT_C2R, batch) != HIPFFT_SUCCESS)
            return set_err(SCARLET_E_HIP, "hipfftPlanMany failed");
        it = g_plans.emplace(key, p).first;
    }
    *out = it->second;
    return SCARLET_OK;
}
static int fft_r2c(const FftPlans &p, float *in, float2 *out, hipStream_t st)
{
    std::lock_guard<std::mutex> lock(g_fft_exec_mu);
    if (hipfftSetStream(p.r2c, st) != HIPFFT_SUCCESS ||
        hipfftExecR2C(p.r2c, (hipfftReal *)in, (hipfftComplex *)out) != HIPFFT_SUCCESS)
        return set_err(SCARLET_E_HIP, "hipfftExecR2C failed");
    return SCARLET_OK;
}
static int fft_c2r(const FftPlans &p, float2 *in, float *out, hipStream_t st)
{
    std::lock_guard<std::mutex> lock(g_fft_exec_mu);
    if (hipfftSetStream(p.c2r, st) != HIPFFT_SUCCESS ||
        hipfftExecC2R(p.c2r, (hipfftComplex *)in, (hipfftReal *)out) != HIPFFT_SUCCESS)
        return set_err(SCARLET_E_HIP, "hipfftExecC2R failed");
    return SCARLET_OK;
}
static unsigned grid_for(int64_t n) { int64_t g = (n + SC_BLOCK - 1) / SC_BLOCK; return (unsigned)(g > 4096 ? 4096 : (g < 1 ? 1 : g)); }

// One hipFFT convolution of `planes` planes, in place: real -> spec, times K-hat (adjoint: its conjugate) and `scale`,
// -> real.  `before_mul` enqueues what the product needs besides the planes' spectrum (scarlet_convolve_same: K-hat).
template <typename BeforeMul>
static int hipfft_convolve(const FftPlans &p, float *real, float2 *spec, const float2 *khat, int nk, int64_t planes,
                           int plane_elems, int adjoint, float scale, hipStream_t st, BeforeMul before_mul)
{
    int rc;
    if ((rc = fft_r2c(p, real, spec, st)) || (rc = before_mul())) return rc;
    hipLaunchKernelGGL(k_spec_mul, dim3(grid_for(planes * plane_elems)), dim3(SC_BLOCK), 0, st, spec, khat, nk, plane_elems,
                       planes * plane_elems, adjoint, scale);
    return fft_c2r(p, spec, real, st);
}
static int hipfft_convolve(const FftPlans &p, float *real, float2 *spec, const float2 *khat, int nk, int64_t planes,
                           int plane_elems, int adjoint, float scale, hipStream_t st)
{
    return hipfft_convolve(p, real, spec, khat, nk, planes, plane_elems, adjoint, scale, st, [] { return (int)SCARLET_OK; });
}

static int prepare_psf_impl(scarlet_batch *b, const WsLayout &l, void *stream)
{
    const PsfGeom &g = l.geom;
    hipStream_t st = (hipStream_t)stream;
    const int nk = b->diff_kernel_per_scene ? b->S * b->B : b->B;
    int rc;
    if (l.psf_lds) {
        // LDS-resident transform (fftconv.h): tables, then K-hat by the same forward code as the iteration
        FftPlan fp = l.plan;
        std::vector<float2> tab;
        fft_fill_tables(fp, tab);
        float2 *dtab = ws_at<float2>(b, l.lds_tables);
        HIP_TRY(hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(float2), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));            // `tab` is host memory of this call
        fp.tables = dtab;
        const size_t lds = fft_lds_bytes(fp.Fy, fp.M, fp.RS);
        if ((rc = allow_lds(k_fft_khat, lds))) return rc;
        hipLaunchKernelGGL(k_fft_khat, dim3(nk), dim3(SC_FFT_NT), lds, st, b->diff_kernel, fp, ws_at<float2>(b, l.lds_khat));
        HIP_TRY(hipGetLastError());
        return SCARLET_OK;
    }
    float *real = ws_at<float>(b, l.real);
    float2 *khat = ws_at<float2>(b, l.khat);
    const int oky = (g.Fry - b->psf_h + 1) / 2 - g.Fry / 2, okx = (g.Frx - b->psf_w + 1) / 2 - g.Frx / 2;
    hipLaunchKernelGGL(k_psf_pad_kernel, dim3(grid_for((int64_t)nk * g.Fy * g.Fx)), dim3(SC_BLOCK), 0, st,
                       b->diff_kernel, nk, b->psf_h, b->psf_w, g.Fy, g.Fx, oky, okx, real);
    FftPlans pk;
    if ((rc = get_plans(g.Fy, g.Fx, nk, &pk))) return rc;
    if ((rc = fft_r2c(pk, real, khat, st))) return rc;
    FftPlans pb;
    if ((rc = get_plans(g.Fy, g.Fx, b->S * b->B, &pb))) return rc;     // create the big plans now
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}
extern "C" int scarlet_batch_prepare_psf(scarlet_batch *b, void *stream)
{
    int rc = check_batch(b);
    if (rc) return rc;
    if (!has_psf(b)) return set_err(SCARLET_E_ARG, "no diff_kernel in batch");
    const WsLayout l = ws_layout(b, WS_FIX);
    rc = prepare_psf_impl(b, l, stream);
    if (rc == SCARLET_OK && l.split && l.psf_lds) {
        scarlet_batch v[2];
        WsLayout lv[2];
        scarlet_constraints cv[2];
        split_views(b, l, v, lv, nullptr, cv);
        for (int h = 0; h < 2 && rc == SCARLET_OK; ++h) rc = prepare_psf_impl(&v[h], lv[h], stream);
    }
    return rc;
}

// A second stream per calling thread for work that is off an iteration's critical path (fork / join by events, so a
// caller capturing its stream into a hipGraph captures both branches).
struct SideStream { hipStream_t st; hipEvent_t ev[3]; int device; };
static int side_stream(SideStream **out)
{
    static thread_local SideStream t_side[16];          // one per device this thread has used
    static thread_local int t_n = 0;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    for (int i = 0; i < t_n; ++i)
        if (t_side[i].device == dev) { *out = &t_side[i]; return SCARLET_OK; }
    if (t_n == 16) { *out = nullptr; return SCARLET_OK; }   // (more devices than that in one thread: no second stream)
    SideStream &n = t_side[t_n];
    HIP_TRY(hipStreamCreateWithFlags(&n.st, hipStreamNonBlocking));
    for (int i = 0; i < 3; ++i) {
        const hipError_t e = hipEventCreateWithFlags(&n.ev[i], hipEventDisableTiming);
        if (e != hipSuccess) {                                  // nothing of a half-built entry survives
            for (int j = 0; j < i; ++j) (void)hipEventDestroy(n.ev[j]);
            (void)hipStreamDestroy(n.st);
            n.st = nullptr;
            snprintf(g_err, sizeof(g_err), "HIP error: %s (side stream events)", hipGetErrorString(e));
            return SCARLET_E_HIP;
        }
    }
    n.device = dev;
    ++t_n;
    *out = &n;
    return SCARLET_OK;
}

// the Gram partials of the many-component path: one MFMA pass when the planes allow 16-byte loads
static void launch_bigk_gram(const GradArgs &a, int nch, hipStream_t st)
{
    if ((a.HW & 3) == 0 && !opt(OPT_NO_GRAM_MFMA))
        hipLaunchKernelGGL(k_bigk_gram_mfma, dim3(a.T, a.S), dim3(SC_BLOCK), 0, st, a);
    else
        hipLaunchKernelGGL(k_bigk_gram, dim3(a.T, nch * (nch + 1) / 2, a.S), dim3(SC_BLOCK), 0, st, a);
}

// k_bigk_step by band count (the accumulators of absent bands would cost occupancy)
static void launch_bigk_step(const GradArgs &a, int nch, const float *resid, hipStream_t st)
{
    const dim3 grid(a.T, nch, a.S);
    if (a.B <= 4) hipLaunchKernelGGL((k_bigk_step<4>), grid, dim3(SC_BLOCK), 0, st, a, resid);
    else if (a.B <= 6) hipLaunchKernelGGL((k_bigk_step<6>), grid, dim3(SC_BLOCK), 0, st, a, resid);
    else hipLaunchKernelGGL((k_bigk_step<SC_BMAX>), grid, dim3(SC_BLOCK), 0, st, a, resid);
}

// the Gram matrix and lambda_max of the many-component path on one stream; `mode` is k_bigk_lipschitz's
static void launch_bigk_lipschitz(const GradArgs &a, int nch, int mode, hipStream_t st)
{
    launch_bigk_gram(a, nch, st);
    hipLaunchKernelGGL(k_bigk_lipschitz, dim3(a.S), dim3(SC_BLOCK), 0, st, a, mode);
}

// The same on the second stream, beside what `st` does from here on.  `precede` enqueues on `st` what k_bigk_lipschitz
// has to wait for and says whether there was anything: the residual (whose loss it reads) in the chunked form, nothing
// in the fused form.  The SED step joins on ev[2].
template <typename Precede>
static int bigk_lipschitz_beside(SideStream *side, const GradArgs &a, int nch, int mode, hipStream_t st, Precede precede)
{
    HIP_TRY(hipEventRecord(side->ev[0], st));
    HIP_TRY(hipStreamWaitEvent(side->st, side->ev[0], 0));
    launch_bigk_gram(a, nch, side->st);
    if (precede()) {
        HIP_TRY(hipEventRecord(side->ev[1], st));
        HIP_TRY(hipStreamWaitEvent(side->st, side->ev[1], 0));
    }
    hipLaunchKernelGGL(k_bigk_lipschitz, dim3(a.S), dim3(SC_BLOCK), 0, side->st, a, mode);
    HIP_TRY(hipEventRecord(side->ev[2], side->st));
    return SCARLET_OK;
}

// the morphology step and the SED step (class 1); `join`: the SED step waits for the second stream's lambda_max
static int bigk_step_sed(const GradArgs &a, int nch, const float *resid, SideStream *join, hipStream_t st)
{
    prof_start(1, st);
    launch_bigk_step(a, nch, resid, st);
    if (join) HIP_TRY(hipStreamWaitEvent(st, join->ev[2], 0));
    hipLaunchKernelGGL(k_bigk_sed, dim3(a.S), dim3(SC_BLOCK), 0, st, a, 0);
    prof_stop(st);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}

// ---- K > SC_KBIG (hugek.h).  Its functions stand in the order of their passes: the code object lists a template kernel
// where the host code first names it, and a host-only change keeps that order.
// The residual planes and the loss record.  Without a PSF k_bigk_resid makes both from the morphologies; with one,
// `psf_planes` holds the compact gradient planes G [S][B][H][W], which serve as they are, and `psf_loss` the per-plane
// loss sums.
static const float *huge_resid(const scarlet_batch *b, const WsLayout &l, const GradArgs &a, const float *psf_planes,
                               const double *psf_loss, hipStream_t st)
{
    if (psf_planes) {
        hipLaunchKernelGGL(k_bigk_loss_from_planes, dim3((a.S + SC_BLOCK - 1) / SC_BLOCK), dim3(SC_BLOCK), 0, st, a, psf_loss);
        return psf_planes;
    }
    float *resid = ws_at<float>(b, l.gplanes);
    hipLaunchKernelGGL((k_bigk_resid<SC_KHUGE>), dim3(a.T, a.S), dim3(SC_BLOCK), 0, st, a, resid);
    return resid;
}

static HugeArgs huge_args(const scarlet_batch *b, const WsLayout &l)
{
    HugeArgs h;
    h.C = huge_nchunks(b->H * b->W);
    h.gpart = ws_at<double>(b, l.gpart); h.gram = ws_at<double>(b, l.gram);
    h.msq[0] = ws_at<double>(b, l.msq[0]); h.msq[1] = ws_at<double>(b, l.msq[1]);
    return h;
}

// the Gram matrix of K > SC_KBIG components (hugek.h) and its lambda_max: by repeated squaring, or its trace
static void launch_huge_lipschitz(const GradArgs &a, const HugeArgs &h, int approximate_L, hipStream_t st)
{
    const int nb = huge_nblk(a.K), npairs = huge_npairs(a.K);
    if ((a.HW & 3) == 0) hipLaunchKernelGGL((k_huge_gram<true>), dim3(h.C, npairs, a.S), dim3(SC_BLOCK), 0, st, a, h);
    else hipLaunchKernelGGL((k_huge_gram<false>), dim3(h.C, npairs, a.S), dim3(SC_BLOCK), 0, st, a, h);
    hipLaunchKernelGGL(k_huge_gram_reduce, dim3(npairs, a.S), dim3(SC_BLOCK), 0, st, a, h);
    const double *last = h.gram;
    if (!approximate_L)
        for (int q = 0; q < SC_HUGE_SQUARINGS; ++q) {
            hipLaunchKernelGGL(k_huge_square, dim3(nb, nb, a.S), dim3(SC_BLOCK), 0, st, a, last, h.msq[q & 1]);
            last = h.msq[q & 1];
        }
    hipLaunchKernelGGL(k_huge_lipschitz, dim3(a.S), dim3(SC_BLOCK), 0, st, a, h, last);
}

// The gradient step for K > SC_KBIG; psf_planes, psf_loss: as huge_resid takes them
static int backward_hugek(scarlet_batch *b, const WsLayout &l, int approximate_L, int raw_gradient, const float *psf_planes,
                          const double *psf_loss, hipStream_t st)
{
    const GradArgs a = grad_args(b, l, approximate_L, raw_gradient);
    prof_start(0, st);
    const float *resid = huge_resid(b, l, a, psf_planes, psf_loss, st);
    launch_huge_lipschitz(a, huge_args(b, l), approximate_L, st);
    hipLaunchKernelGGL(k_bigk_lmorph<SC_KHUGE>, dim3(a.S), dim3(SC_WAVE), 0, st, a);
    prof_stop(st);
    return bigk_step_sed(a, (b->K + SC_CHUNK - 1) / SC_CHUNK, resid, nullptr, st);
}

// The arguments of one PSF chain.  `ob` owns the images, weights, PSF workspace and lipschitz / mse; `state` owns morph,
// cur, active and it (a single-observation fit passes one batch for both).  sed0, sed1: the SED buffers the model planes
// are built from.
static PsfArgs psf_args(const scarlet_batch *ob, const WsLayout &l, const scarlet_batch *state, float *sed0, float *sed1,
                        const uint8_t *fix_sed, const uint8_t *fix_morph, int approximate_L, int raw_gradient)
{
    PsfArgs a = {};
    a.S = ob->S; a.K = ob->K; a.B = ob->B; a.T = n_tiles(ob); a.g = l.geom;
    a.images = ob->images; a.weights = ob->weights; a.weight_scalar = ob->weight_scalar;
    a.sed[0] = sed0; a.sed[1] = sed1; a.morph[0] = state->morph[0]; a.morph[1] = state->morph[1];
    a.cur = state->cur; a.fix_sed = fix_sed; a.fix_morph = fix_morph;
    a.real = ws_at<float>(ob, l.real);
    a.spec = ws_at<float2>(ob, l.spec);
    a.khat = ws_at<const float2>(ob, l.psf_lds ? l.lds_khat : l.khat);
    a.khat_per_scene = ob->diff_kernel_per_scene;
    a.partials = ws_at<double>(ob, l.partials); a.loss_part = ws_at<double>(ob, l.loss);
    a.lipschitz = ob->lipschitz; a.mse = ob->mse; a.mse_capacity = ob->mse_capacity;
    a.it = state->it; a.active = state->active; a.approximate_L = approximate_L; a.raw_gradient = raw_gradient;
    return a;
}

// The gradient planes of one PSF chain: model planes, render, residual + loss, adjoint.  On return G lies in a.real as
// planes [S][B][a.g.Fy][a.g.Fx] with the image at offset (a.g.oy, a.g.ox), and a.loss_part holds the per-plane losses:
// compact planes (Fy = H, Fx = W, no offset) from the LDS-resident form, the padded hipFFT planes otherwise.  a.g is
// also the geometry the gradient kernels after the stage read G through.
// `model`: which kernel writes the model planes.  PSF_MODEL_GRAM is the three-pass form's k_psf_model4g, which also leaves
// the Gram partials (K <= SC_KMAX, LDS-resident form, H W % 4 == 0: the caller's choice); PSF_MODEL_PLAIN takes
// k_psf_model4 or k_psf_model by H W % 4 and the K range.  Opens no profiler class: the callers bracket it.
enum PsfModel { PSF_MODEL_PLAIN, PSF_MODEL_GRAM };
static int psf_gradient_planes(const scarlet_batch *b, const WsLayout &l, PsfArgs &a, PsfModel model, hipStream_t st)
{
    const PsfGeom &g = l.geom;
    const int HW = b->H * b->W, planes = b->S * b->B;
    const bool huge = b->K > SC_KBIG;
    int rc;
    if (l.psf_lds) {
        // one kernel after the model's: render, residual + loss, adjoint
        FftPlan fp = l.plan;
        fp.tables = ws_at<const float2>(b, l.lds_tables);
        const bool x128 = psf_conv_finish_plan(b, &fp);
        const size_t lds = fft_lds_bytes(fp.Fy, fp.M, fp.RS, b->H, b->W, fp.dma_image != 0);
        if ((rc = allow_lds(k_psf_conv, lds))) return rc;
        // model planes, compact [S][B][H][W], into `real` (k_psf_model with the geometry of an unpadded plane)
        a.g.Fy = b->H; a.g.Fx = b->W; a.g.Fxh = b->W / 2 + 1; a.g.oy = 0; a.g.ox = 0;
        auto plain = [&](void (*k4)(PsfArgs), void (*k1)(PsfArgs)) {      // (four pixels per lane where the plane allows)
            if (HW % 4 == 0) hipLaunchKernelGGL(k4, dim3((HW / 4 + SC_BLOCK - 1) / SC_BLOCK, b->S), dim3(SC_BLOCK), 0, st, a);
            else hipLaunchKernelGGL(k1, dim3((HW + SC_BLOCK - 1) / SC_BLOCK, b->S), dim3(SC_BLOCK), 0, st, a);
        };
        if (huge) plain(k_psf_model4<SC_KHUGE>, k_psf_model<SC_KHUGE>);
        else if (model == PSF_MODEL_GRAM)
            hipLaunchKernelGGL(b->K <= 4 ? k_psf_model4g<4> : k_psf_model4g<SC_KMAX>, dim3(a.T, a.S), dim3(SC_BLOCK), 0, st, a);
        else plain(k_psf_model4<SC_KBIG>, k_psf_model<SC_KBIG>);
        long long *stamps = opt(OPT_STAMPS) ? ws_at<long long>(b, l.stamps) : nullptr;
        fp.stagger_wgs = 0;
        const int groups = (b->S + 7) / 8;
        if (x128) {
            // (the instance keeps the image in registers unless built with SC_X128_DMA: plane + tables only)
            const size_t lds_x = fft_lds_bytes(fp.Fy, fp.M, fp.RS, b->H, b->W, SC_X128_DMA != 0);
            if ((rc = allow_lds(k_psf_conv_x128, lds_x))) return rc;
            hipLaunchKernelGGL(k_psf_conv_x128, dim3(groups * 8 * b->B), dim3(SC_FFT_NT_X), lds_x, st, a, fp, a.real, stamps);
        } else
            hipLaunchKernelGGL(k_psf_conv, dim3(groups * 8 * b->B), dim3(SC_FFT_NT), lds, st, a, fp, a.real, stamps);
    } else {
        FftPlans p;
        if ((rc = get_plans(g.Fy, g.Fx, planes, &p))) return rc;
        const int plane_elems = g.Fy * g.Fxh, nkh = b->diff_kernel_per_scene ? planes : b->B;
        const float scale = 1.0f / ((float)g.Fy * (float)g.Fx);
        const dim3 grid((g.Fy * g.Fx + SC_BLOCK - 1) / SC_BLOCK, b->S);
        if (huge) hipLaunchKernelGGL(k_psf_model<SC_KHUGE>, grid, dim3(SC_BLOCK), 0, st, a);
        else hipLaunchKernelGGL(k_psf_model<SC_KBIG>, grid, dim3(SC_BLOCK), 0, st, a);
        if ((rc = hipfft_convolve(p, a.real, a.spec, a.khat, nkh, planes, plane_elems, 0, scale, st))) return rc;
        hipLaunchKernelGGL(k_psf_resid, dim3(planes), dim3(SC_BLOCK), 0, st, a);
        if ((rc = hipfft_convolve(p, a.real, a.spec, a.khat, nkh, planes, plane_elems, 1, scale, st))) return rc;
    }
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}

// G as the many-component passes read it, compact [S][B][H][W]: where the stage left it (LDS-resident form), or cropped
// out of the hipFFT planes once
static const float *psf_compact_planes(const scarlet_batch *b, const WsLayout &l, const PsfArgs &a, hipStream_t st)
{
    if (l.psf_lds) return a.real;
    float *out = ws_at<float>(b, l.gplanes);
    hipLaunchKernelGGL(k_plane_crop, dim3(grid_for((int64_t)a.S * a.B * b->H * b->W)), dim3(SC_BLOCK), 0, st,
                       (const float *)a.real, a.S * a.B, b->H, b->W, a.g.Fy, a.g.Fx, a.g.oy, a.g.ox, out);
    return out;
}

// the pair "gradient kernel, step kernel" over the tiles of every scene, each under its profiler class
template <typename Args>
static void launch_grad_step(void (*grad)(Args), void (*step)(Args), const Args &a, hipStream_t st)
{
    const dim3 grid(a.T, a.S);
    prof_start(0, st);
    hipLaunchKernelGGL(grad, grid, dim3(SC_BLOCK), 0, st, a);
    prof_stop(st); prof_start(1, st);
    hipLaunchKernelGGL(step, grid, dim3(SC_BLOCK), 0, st, a);
    prof_stop(st);
}

static int backward_step_psf(scarlet_batch *b, const WsLayout &l, int approximate_L, int raw_gradient, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    PsfArgs a = psf_args(b, l, b, b->sed[0], b->sed[1], b->fix_sed, b->fix_morph, approximate_L, raw_gradient);
    const bool vec4 = l.psf_lds && (b->H * b->W) % 4 == 0;         // compact gradient planes: 16 B per lane
    // three-pass form (psf_path.h): the model pass also leaves the Gram partials
    const bool three_pass = vec4 && l.grad == GRAD_SMALL && !opt(OPT_NO_PSF3PASS);
    int rc;
    prof_start(5, st);
    if ((rc = psf_gradient_planes(b, l, a, three_pass ? PSF_MODEL_GRAM : PSF_MODEL_PLAIN, st))) return rc;
    prof_stop(st);
    if (l.grad == GRAD_HUGEK)
        return backward_hugek(b, l, approximate_L, raw_gradient, psf_compact_planes(b, l, a, st), a.loss_part, st);
    if (l.grad == GRAD_BIGK) {
        // many components: the chunked passes of bigk.h over the compact planes, on the one stream
        const GradArgs ga = grad_args(b, l, approximate_L, raw_gradient);
        const int nch = (b->K + SC_CHUNK - 1) / SC_CHUNK;
        prof_start(0, st);
        const float *resid = psf_compact_planes(b, l, a, st);
        hipLaunchKernelGGL(k_bigk_loss_from_planes, dim3((b->S + SC_BLOCK - 1) / SC_BLOCK), dim3(SC_BLOCK), 0, st, ga,
                           (const double *)a.loss_part);
        launch_bigk_lipschitz(ga, nch, 0, st);
        prof_stop(st);
        return bigk_step_sed(ga, nch, resid, nullptr, st);
    }
    if (three_pass) {
        // morphology step + SED-gradient partials in one pass over G, then the per-scene scalar head
        auto step = [&](auto kc) {
            constexpr int KC = decltype(kc)::value;
            const dim3 grid(a.T, a.S);
            prof_start(1, st);
            // (instances by band count: the accumulators of absent bands would cost occupancy)
            if (b->B <= 4) hipLaunchKernelGGL((k_step_psf4f<KC, 4>), grid, dim3(SC_BLOCK), 0, st, a);
            else if (b->B <= 6) hipLaunchKernelGGL((k_step_psf4f<KC, 6>), grid, dim3(SC_BLOCK), 0, st, a);
            else hipLaunchKernelGGL((k_step_psf4f<KC, SC_BMAX>), grid, dim3(SC_BLOCK), 0, st, a);
            hipLaunchKernelGGL((k_sed_step<KC, SC_BMAX>), dim3(a.S), dim3(SC_BLOCK), 0, st, a);
            prof_stop(st);
        };
        if (b->K <= 4) step(std::integral_constant<int, 4>{});
        else step(std::integral_constant<int, SC_KMAX>{});
    } else if (vec4)
        launch_grad_step(b->K <= 4 ? k_grad_psf4<4, SC_BMAX> : k_grad_psf4<SC_KMAX, SC_BMAX>,
                         b->K <= 4 ? k_step_psf4<4, SC_BMAX> : k_step_psf4<SC_KMAX, SC_BMAX>, a, st);
    else if (b->K <= 4)
        launch_grad_step(k_grad_psf<4, SC_BMAX>, k_step_psf<4, SC_BMAX>, a, st);
    else
        launch_grad_step(k_grad_psf<SC_KMAX, SC_BMAX>, k_step_psf<SC_KMAX, SC_BMAX>, a, st);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}

extern "C" int scarlet_match_psfs(const float *psf1, int n, int P1y, int P1x, const float *psf2, int n2,
                                  int P2y, int P2x, float *out, void *stream)
{
    if (!psf1 || !psf2 || !out || n <= 0 || (n2 != n && n2 != 1) || P1y <= 0 || P1x <= 0 || P2y <= 0 || P2x <= 0)
        return set_err(SCARLET_E_ARG, "bad match_psfs arguments");
    // fft._get_fft_shape(psf1, psf2, padding=3): 5-smooth length of the SUM of the sizes + 3, last axis even.
    // (A spectrum ratio is a deconvolution on the periodic domain: unlike the convolutions of the fit it
    // depends on the FFT shape, so the reference's shape is used as is.)
    const int Fy = scarlet_next_fast_len(P1y + P2y + 3);
    int Fx = scarlet_next_fast_len(P1x + P2x + 3);
    while (Fx & 1) Fx = scarlet_next_fast_len(Fx + 1);
    const int64_t plane = (int64_t)Fy * Fx, splane = (int64_t)Fy * (Fx / 2 + 1);
    hipStream_t st = (hipStream_t)stream;
    DevBuf br1, br2, bs1, bs2;
    DEV_ALLOC(br1, n * plane * sizeof(float));
    DEV_ALLOC(br2, n2 * plane * sizeof(float));
    DEV_ALLOC(bs1, n * splane * sizeof(float2));
    DEV_ALLOC(bs2, n2 * splane * sizeof(float2));
    float *r1 = br1.as<float>(), *r2 = br2.as<float>(); float2 *s1 = bs1.as<float2>(), *s2 = bs2.as<float2>();
    const int o1y = (Fy - P1y + 1) / 2 - Fy / 2, o1x = (Fx - P1x + 1) / 2 - Fx / 2;
    const int o2y = (Fy - P2y + 1) / 2 - Fy / 2, o2x = (Fx - P2x + 1) / 2 - Fx / 2;
    hipLaunchKernelGGL(k_plane_pad, dim3(grid_for(n * plane)), dim3(SC_BLOCK), 0, st, psf1, n, P1y, P1x, Fy, Fx, o1y, o1x, r1);
    hipLaunchKernelGGL(k_plane_pad, dim3(grid_for(n2 * plane)), dim3(SC_BLOCK), 0, st, psf2, n2, P2y, P2x, Fy, Fx, o2y, o2x, r2);
    FftPlans pa, pb;
    int rc;
    if ((rc = get_plans(Fy, Fx, n, &pa)) == SCARLET_OK && (rc = get_plans(Fy, Fx, n2, &pb)) == SCARLET_OK &&
        (rc = fft_r2c(pa, r1, s1, st)) == SCARLET_OK && (rc = fft_r2c(pb, r2, s2, st)) == SCARLET_OK) {
        hipLaunchKernelGGL(k_spec_div, dim3(grid_for(n * splane)), dim3(SC_BLOCK), 0, st, s1, (const float2 *)s2, n2,
                           (int)splane, n * splane, 1.0f / ((float)Fy * (float)Fx));
        if ((rc = fft_c2r(pa, s1, r1, st)) == SCARLET_OK)
            hipLaunchKernelGGL(k_plane_crop, dim3(grid_for((int64_t)n * P1y * P1x)), dim3(SC_BLOCK), 0, st,
                               (const float *)r1, n, P1y, P1x, Fy, Fx, o1y, o1x, out);
    }
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(st);    // buffers outlive the kernels
    if (rc) return rc;
    HIP_TRY(e1); HIP_TRY(e2);
    return SCARLET_OK;
}

extern "C" int scarlet_convolve_same(const float *model, int n, int H, int W, const float *kernel, int nk,
                                     int Py, int Px, float *out, void *stream)
{
    if (!model || !kernel || !out || n <= 0 || H <= 0 || W <= 0 || Py <= 0 || Px <= 0 || (nk != n && nk != 1))
        return set_err(SCARLET_E_ARG, "bad convolve arguments");
    const PsfGeom g = psf_geom(H, W, Py, Px);
    hipStream_t st = (hipStream_t)stream;
    FftPlan fp;
    if (fft_make_plan(H, W, Py, Px, &fp) && !opt(OPT_PSF_HIPFFT)) {
        // LDS-resident transform (fftconv.h), one workgroup per plane
        std::vector<float2> tab;
        fft_fill_tables(fp, tab);
        DevBuf dtab, dkhat;
        DEV_ALLOC(dtab, tab.size() * sizeof(float2));
        DEV_ALLOC(dkhat, (size_t)nk * fp.Fy * (fp.M + 1) * sizeof(float2));
        HIP_TRY(hipMemcpy(dtab.p, tab.data(), tab.size() * sizeof(float2), hipMemcpyHostToDevice));
        fp.tables = dtab.as<float2>();
        const size_t lds = fft_lds_bytes(fp.Fy, fp.M, fp.RS);
        int rc;
        if ((rc = allow_lds(k_fft_khat, lds)) || (rc = allow_lds(k_fft_convolve, lds))) return rc;
        hipLaunchKernelGGL(k_fft_khat, dim3(nk), dim3(SC_FFT_NT), lds, st, kernel, fp, dkhat.as<float2>());
        hipLaunchKernelGGL(k_fft_convolve, dim3(n), dim3(SC_FFT_NT), lds, st, model, fp, (const float2 *)dkhat.as<float2>(), nk, out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));            // the temporaries outlive the kernels
        return SCARLET_OK;
    }
    const int64_t plane = (int64_t)g.Fy * g.Fx, splane = (int64_t)g.Fy * g.Fxh;
    DevBuf breal, bkreal, bspec, bkspec;
    DEV_ALLOC(breal, n * plane * sizeof(float));
    DEV_ALLOC(bkreal, nk * plane * sizeof(float));
    DEV_ALLOC(bspec, n * splane * sizeof(float2));
    DEV_ALLOC(bkspec, nk * splane * sizeof(float2));
    float *real = breal.as<float>(), *kreal = bkreal.as<float>(); float2 *spec = bspec.as<float2>(), *kspec = bkspec.as<float2>();
    const int oky = (g.Fry - Py + 1) / 2 - g.Fry / 2, okx = (g.Frx - Px + 1) / 2 - g.Frx / 2;
    hipLaunchKernelGGL(k_plane_pad, dim3(grid_for(n * plane)), dim3(SC_BLOCK), 0, st, model, n, H, W, g.Fy, g.Fx, g.oy, g.ox, real);
    hipLaunchKernelGGL(k_psf_pad_kernel, dim3(grid_for(nk * plane)), dim3(SC_BLOCK), 0, st, kernel, nk, Py, Px, g.Fy, g.Fx, oky, okx, kreal);
    FftPlans pm, pk;
    int rc;
    if ((rc = get_plans(g.Fy, g.Fx, n, &pm)) == SCARLET_OK && (rc = get_plans(g.Fy, g.Fx, nk, &pk)) == SCARLET_OK &&
        (rc = hipfft_convolve(pm, real, spec, kspec, nk, n, (int)splane, 0, 1.0f / ((float)g.Fy * (float)g.Fx), st,
                              [&] { return fft_r2c(pk, kreal, kspec, st); })) == SCARLET_OK)
        hipLaunchKernelGGL(k_plane_crop, dim3(grid_for((int64_t)n * H * W)), dim3(SC_BLOCK), 0, st, real, n, H, W,
                           g.Fy, g.Fx, g.oy, g.ox, out);
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(st);    // buffers outlive the kernels
    if (rc) return rc;
    HIP_TRY(e1); HIP_TRY(e2);
    return SCARLET_OK;
}

// The gradient step for SC_KMAX < K <= SC_KBIG without a PSF: passes over chunks of eight components (bigk.h), in one of
// three forms
static int backward_bigk(scarlet_batch *b, const WsLayout &l, int approximate_L, int raw_gradient, hipStream_t st)
{
    const GradArgs a = grad_args(b, l, approximate_L, raw_gradient);
    const int nch = (b->K + SC_CHUNK - 1) / SC_CHUNK;
    float *resid = ws_at<float>(b, l.gplanes);
    int rc;
    SideStream *side = nullptr;
    if (!opt(OPT_NO_SIDE_STREAM) && (rc = side_stream(&side))) return rc;
    if (!approximate_L && (a.HW & 63) == 0 && !opt(OPT_NO_BIGK_FUSED)) {
        // residual + morphology step + SED-gradient sums in one pass on the matrix cores (k_bigk_fused); the Gram
        // matrix and its eigenvalue beside it on the second stream:
        //   stream : lmorph . fused ..... (join) sed (+ loss record)
        //   side   : gram . lipschitz           (exact constants do not need the loss)
        if (side && (rc = bigk_lipschitz_beside(side, a, nch, 2, st, [] { return false; }))) return rc;
        prof_start(0, st);
        hipLaunchKernelGGL(k_bigk_lmorph<SC_KBIG>, dim3(a.S), dim3(SC_WAVE), 0, st, a);
        prof_stop(st); prof_start(1, st);
        hipLaunchKernelGGL(k_bigk_fused, dim3(a.T, a.S), dim3(SC_BLOCK), 0, st, a);
        if (side) HIP_TRY(hipStreamWaitEvent(st, side->ev[2], 0));
        else launch_bigk_lipschitz(a, nch, 2, st);
        hipLaunchKernelGGL(k_bigk_sed, dim3(a.S), dim3(SC_BLOCK), 0, st, a, 1);
        prof_stop(st);
        HIP_TRY(hipGetLastError());
        return SCARLET_OK;
    }
    auto launch_resid = [&] {
        hipLaunchKernelGGL(k_bigk_resid<SC_KBIG>, dim3(a.T, a.S), dim3(SC_BLOCK), 0, st, a, resid);
        return true;
    };
    prof_start(0, st);
    if (side) {
        // The morphology step needs the residual planes and lambda_max(A^T A) only; the Gram matrix S S^T and
        // its largest eigenvalue (for the SED step) run beside it on a second stream:
        //   stream : resid . lmorph . step ............ (join) sed
        //   side   : gram ......... (after resid: loss) lipschitz
        if ((rc = bigk_lipschitz_beside(side, a, nch, 1, st, launch_resid))) return rc;
        hipLaunchKernelGGL(k_bigk_lmorph<SC_KBIG>, dim3(a.S), dim3(SC_WAVE), 0, st, a);
    } else {
        launch_resid();
        launch_bigk_lipschitz(a, nch, 0, st);
    }
    prof_stop(st);
    return bigk_step_sed(a, nch, resid, side, st);
}

// raw_gradient = 0: buffer 1-cur receives the stepped factors; 1: the gradients themselves
static int backward_impl(scarlet_batch *b, const WsLayout &l, int approximate_L, int raw_gradient, void *stream)
{
    if (b->diff_kernel)            // (a kernel without a size has no PSF area in the workspace)
        return l.psf ? backward_step_psf(b, l, approximate_L, raw_gradient, stream)
                     : set_err(SCARLET_E_ARG, "diff_kernel without psf_h, psf_w");
    hipStream_t st = (hipStream_t)stream;
    if (l.grad == GRAD_HUGEK) return backward_hugek(b, l, approximate_L, raw_gradient, nullptr, nullptr, st);
    if (l.grad == GRAD_BIGK) return backward_bigk(b, l, approximate_L, raw_gradient, st);
    const GradArgs a = grad_args(b, l, approximate_L, raw_gradient);
    if (b->K <= 4) launch_grad_step(k_grad<4, SC_BMAX>, k_step<4, SC_BMAX>, a, st);
    else launch_grad_step(k_grad<SC_KMAX, SC_BMAX>, k_step<SC_KMAX, SC_BMAX>, a, st);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}

__global__ void k_zero_int(int *p) { *p = 0; }

// L_comp: the constants each component stepped with (scarlet_prior::L_comp), or NULL: the scene's
// cons: the components' own switches, or NULL: the batch's.  skip_status: status bits of the scenes a constructor call leaves alone
// frame_hw: scarlet_frames::frame_hw of the batch (or of the view: advanced to its first scene), or NULL
// upd: the batch's update options (never with a box stage; check_request says what they go with), or NULL: the stock pipeline
struct UpdateOpts { const double *L_comp; const scarlet_constraints *cons; int skip_status; const int32_t *frame_hw;
                    const scarlet_update_options *upd; };
// in_iteration = 0: the constructors' call (UpdateArgs::force_it0)
static int launch_update(scarlet_batch *b, const WsLayout &l, int in_iteration, void *stream, const UpdateOpts &o)
{
    int rc = ensure_tables();
    if (rc) return rc;
    UpdateArgs u;
    u.S = b->S; u.K = b->K; u.B = b->B; u.H = b->H; u.W = b->W;
    u.sed[0] = b->sed[0]; u.sed[1] = b->sed[1]; u.morph[0] = b->morph[0]; u.morph[1] = b->morph[1];
    u.cur = b->cur; u.in_iteration = in_iteration;
    u.centers = b->centers; u.shifts = b->shifts; u.lipschitz = b->lipschitz; u.it = b->it; u.active = b->active;
    u.status = b->status; u.symmetric = b->symmetric; u.monotonic = b->monotonic;
    u.l0_thresh = b->l0_thresh; u.l1_thresh = b->l1_thresh;
    u.centroid_psf = b->centroid_psf; u.centroid_P = b->centroid_P; u.conv = ws_at<double>(b, l.conv); u.force_it0 = !in_iteration;
    u.gscratch = nullptr;
    u.only_flagged = nullptr;
    u.group = b->group;
    u.ncomp = b->n_components;
    u.L_comp = o.L_comp;
    u.symmetric_c = o.cons ? o.cons->symmetric : nullptr; u.monotonic_c = o.cons ? o.cons->monotonic : nullptr;
    u.l0_c = o.cons ? o.cons->l0_thresh : nullptr; u.l1_c = o.cons ? o.cons->l1_thresh : nullptr;
    u.skip_status = o.skip_status;
    u.frame_hw = (const int *)o.frame_hw;
    const bool ragged = o.frame_hw != nullptr;
    // (ragged frames with group: only the _grouped / _mixed / _frames_options entry points get here -- check_frames_call
    // refuses the pair for every other one; options with group or ragged frames: only the _frames_options ones)
    u.hybrid_sweep = opt(OPT_NO_HYBRID_SWEEP) ? 0 : 1;
    // (a ragged-frame batch runs no box stage: the box kernels take their bounds from the batch's frame)
    const UpdatePlan p = update_plan(b->H, b->W, {!opt(OPT_FORCE_BLOCK_UPDATE), true, b->monotonic && !opt(OPT_NO_BOX) && !ragged && !o.upd,
                                                  !opt(OPT_NO_BOX2), !opt(OPT_NO_EXACT)});
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(b->S * b->K), block(SC_BLOCK);
    // MultiComponentSource: the shared centre of every source first (one wave per scene)
    // (ragged: on each scene's own frame, so that the centroid's radius is cut at the scene's ends)
    if (b->group && (rc = ragged ? launch_lds(k_group_centers<true>, dim3(b->S), dim3(SC_WAVE), group_centers_lds_bytes(b->centroid_P), st, u)
                                 : launch_lds(k_group_centers<false>, dim3(b->S), dim3(SC_WAVE), group_centers_lds_bytes(b->centroid_P), st, u)))
        return rc;
    if (p.box != BOX_NONE) {
        // frames beyond the wave-level tile: the pipeline on the box around each peak (boxupdate.h); the kernels below
        // then run only for the components that left the second box too
        long long *dbg = debug_stamps((size_t)b->S * b->K * 16);
        int *fb = ws_at<int>(b, l.box_fallback), *list = ws_at<int>(b, l.box_list), *count = ws_at<int>(b, l.box_count);
        if (p.box2) hipLaunchKernelGGL(k_zero_int, dim3(1), dim3(1), 0, st, count);   // (a 4-byte hipMemsetAsync costs 16 us)
        // the large box: workgroup i takes list[i]
        auto run = [&](auto small_k, auto listed_k) -> int {
            int r2;
            if ((r2 = allow_lds(small_k, p.box_lds[0])) || (r2 = allow_lds(listed_k, p.box_lds[1]))) return r2;
            hipLaunchKernelGGL(small_k, grid, block, p.box_lds[0], st, u, fb, p.box2 ? list : nullptr, count, dbg);
            if (p.box2)
                hipLaunchKernelGGL(listed_k, grid, block, p.box_lds[1], st, u, fb, (const int *)list, (const int *)count, dbg);
            return SCARLET_OK;
        };
        switch (p.box) {
        case BOX_STREAMED: rc = run(k_source_update_box<0, 0>, k_source_update_box_listed<0, 0>); break;
        case BOX_8_128: rc = run(k_source_update_box<8, 128>, k_source_update_box_listed<8, 128>); break;
        case BOX_16_256: rc = run(k_source_update_box<16, 256>, k_source_update_box_listed<16, 256>); break;
        case BOX_8: rc = run(k_source_update_box<8, 0>, k_source_update_box_listed<8, 0>); break;
        default: rc = run(k_source_update_box<16, 0>, k_source_update_box_listed<16, 0>);
        }
        if (rc) return rc;
        u.only_flagged = fb;
    }
    if (p.form == FORM_TILE_GSCRATCH || p.form == FORM_PLANE) {
        if (!l.has_gscratch) return set_err(SCARLET_E_ARG, "the workspace layout holds no symmetry scratch for this frame");
        u.gscratch = ws_at<float>(b, l.gscratch);
    }
    // the form's kernel out of the four instances of one (ragged, options) pair
    auto run_form = [&](auto wave_k, auto tile_gscratch_k, auto tile_k, auto plane_k, const auto &args) -> int {
        switch (p.form) {
        case FORM_WAVE:             // one wave per component, four components per workgroup (wave_ops.h)
            return launch_lds(wave_k, dim3((b->S * b->K + SC_NWAVES - 1) / SC_NWAVES), block, p.lds, st, args);
        case FORM_TILE_GSCRATCH: return launch_lds(tile_gscratch_k, grid, block, p.lds, st, args);
        case FORM_TILE: return launch_lds(tile_k, grid, block, p.lds, st, args);
        default:                    // operators in place on the plane in HBM / L2 (94 KB at 1024 x 1024)
            return launch_lds(plane_k, grid, block, p.lds, st, args);
        }
    };
    if (o.upd) {                // the options instances (engine.h UpdateArgsOpt); no box stage ran
        UpdateArgsOpt uo;
        static_cast<UpdateArgs &>(uo) = u;
        uo.sym_algorithm = o.upd->sym_algorithm; uo.sym_strength = o.upd->sym_strength;
        uo.mono_nearest = o.upd->mono_nearest; uo.mono_thresh = o.upd->mono_thresh;
        uo.positive = o.upd->positive; uo.normalize = o.upd->normalize;
        // (ragged: on each scene's own frame -- a catalogue batch)
        rc = ragged ? run_form(k_source_update_w_ragged_opt, k_source_update<1, true, UpdateArgsOpt>,
                               k_source_update<0, true, UpdateArgsOpt>, k_source_update<2, true, UpdateArgsOpt>, uo)
                    : run_form(k_source_update_w_opt, k_source_update<1, false, UpdateArgsOpt>,
                               k_source_update<0, false, UpdateArgsOpt>, k_source_update<2, false, UpdateArgsOpt>, uo);
    } else                      // the stock pipeline; ragged: the same forms on each scene's own frame (engine.h RAGGED)
        rc = ragged ? run_form(k_source_update_w_ragged, k_source_update<1, true>, k_source_update<0, true>, k_source_update<2, true>, u)
                    : run_form(k_source_update_w, k_source_update<1>, k_source_update<0>, k_source_update<2>, u);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}

static int launch_converge(scarlet_batch *b, const WsLayout &l, double e_rel, void *stream)
{
    hipLaunchKernelGGL(k_converge, dim3((b->S + SC_BLOCK - 1) / SC_BLOCK), dim3(SC_BLOCK), 0, (hipStream_t)stream,
                       b->S, b->K, ws_at<double>(b, l.conv), b->flags, b->active, b->it, b->cur, e_rel * e_rel,
                       (const int *)b->n_components);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}
extern "C" int scarlet_check_convergence(scarlet_batch *b, double e_rel, void *stream)
{
    int rc = check_batch(b);
    if (!rc) rc = check_counts(b, stream);
    return rc ? rc : launch_converge(b, ws_layout(b, WS_PEEK), e_rel, stream);
}

// workgroups of k_fit2x the current device keeps resident at once (occupancy query x compute units), per device
static int fit2x_resident_workgroups(size_t lds, int *out)
{
    static std::mutex mu;
    static int cached[64] = {0};
    static size_t cached_lds[64] = {0};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return set_err(SCARLET_E_HIP, "device index out of range");
    std::lock_guard<std::mutex> lock(mu);
    if (!cached[dev] || cached_lds[dev] != lds) {
        int per_cu = 0, cus = 0, rc = allow_lds(k_fit2x, lds);        // (the query counts with the LDS the launch will ask for)
        if (rc) return rc;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_fit2x, SC_FB2, lds));
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        if (per_cu < 1) per_cu = 1;
        cached[dev] = per_cu * cus; cached_lds[dev] = lds;
    }
    *out = cached[dev];
    return SCARLET_OK;
}

// ---- fused one-kernel iteration (fused.h, fused2.h): the batches fused_plan (launch_plan.h) has a kernel for
static FusedSwitches fused_switches(void)
{
    return {opt(OPT_NO_EXACT) != 0, opt(OPT_FUSED_V1) != 0, opt(OPT_NO_FUSED) != 0, opt(OPT_NO_PERSIST) != 0, opt(OPT_PERSIST_DBG),
            (size_t)opt(OPT_PAD_LDS)};
}
static bool fused_ok(const scarlet_batch *b, int approximate_L, bool ragged_frames = false)
{
    return fused_plan(b, approximate_L, false, 1, fused_switches(), ragged_frames).kernel != FUSED_NONE;
}
// n_iter > 1: that many iterations in ONE launch where the persistent form exists (k_fit2: the headline shape's
// exact instance); *done receives the number of iterations the launch covers
// frame_hw: the scenes' own frames (the frames instance of the four-wave kernel; per batch: no half-batch views here), or NULL
static int launch_fused(scarlet_batch *b, const WsLayout &l, double e_rel, void *stream, int n_iter, int *done,
                        const scarlet_constraints *cons, const int32_t *frame_hw = nullptr)
{
    if (done) *done = 1;
    int rc = ensure_tables();
    if (rc) return rc;
    FusedArgs f;
    f.S = b->S; f.K = b->K; f.B = b->B; f.H = b->H; f.W = b->W;
    f.images = b->images; f.weights = b->weights; f.weight_scalar = b->weight_scalar;
    f.sed[0] = b->sed[0]; f.sed[1] = b->sed[1]; f.morph[0] = b->morph[0]; f.morph[1] = b->morph[1];
    f.cur = b->cur; f.fix_sed = b->fix_sed; f.fix_morph = b->fix_morph;
    f.centers = b->centers; f.shifts = b->shifts; f.flags = b->flags;
    f.lipschitz = b->lipschitz; f.mse = b->mse; f.mse_capacity = b->mse_capacity;
    f.it = b->it; f.active = b->active; f.status = b->status;
    f.symmetric = b->symmetric; f.monotonic = b->monotonic; f.l0_thresh = b->l0_thresh; f.l1_thresh = b->l1_thresh;
    f.centroid_psf = b->centroid_psf; f.centroid_P = b->centroid_P; f.e_rel2 = e_rel * e_rel;
    f.ncomp = b->n_components;
    f.no_place = opt(OPT_NO_PLACE) != 0;
    // diagnostics: SCARLET_STAMPS=1 writes phase stamps into the (otherwise unused) partials area
    f.kscache = (!l.has_kscache || b->diff_kernel || opt(OPT_NO_KSCACHE)) ? nullptr : ws_at<float>(b, l.kscache);
    f.stamps = (opt(OPT_STAMPS) && n_partials(b->K, b->B) >= 16) ? ws_at<long long>(b, l.partials) : nullptr;
    if (n_iter > 0xffffff) n_iter = 0xffffff;
    const FusedSwitches sw = fused_switches();
    const FusedPlan p = fused_plan(b, 0, cons_any(cons), n_iter, sw, frame_hw != nullptr);
    if (p.kernel == FUSED_NONE) return set_err(SCARLET_E_ARG, "no fused kernel for this batch");
    if (!p.fits) return set_err(SCARLET_E_TOO_LARGE, "image tile does not fit in LDS");
    hipStream_t st = (hipStream_t)stream;
    // allow the LDS, profile class 4 (weight: the iterations the launch covers), launch
    auto run = [&](auto kern, int grid, int weight, const auto &... args) -> int {
        int r = allow_lds(kern, p.lds);
        if (r) return r;
        prof_start(4, st, weight);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(p.block), p.lds, st, args...);
        prof_stop(st);
        HIP_TRY(hipGetLastError());
        return SCARLET_OK;
    };
    switch (p.kernel) {
    case FUSED_PC_B6:
    case FUSED_PC_B8: {
        FusedArgsPC fp;
        static_cast<FusedArgs &>(fp) = f;
        fp.symmetric_c = cons->symmetric; fp.monotonic_c = cons->monotonic; fp.l0_c = cons->l0_thresh; fp.l1_c = cons->l1_thresh;
        return run(p.kernel == FUSED_PC_B6 ? k_iterate<4, 6, FusedArgsPC> : k_iterate<4, SC_BMAX, FusedArgsPC>, b->S, 1, fp);
    }
    case FUSED_FRAMES_B6:
    case FUSED_FRAMES_B8: {
        FusedArgsFrames ff;
        static_cast<FusedArgs &>(ff) = f;
        ff.symmetric_c = cons ? cons->symmetric : nullptr; ff.monotonic_c = cons ? cons->monotonic : nullptr;
        ff.l0_c = cons ? cons->l0_thresh : nullptr; ff.l1_c = cons ? cons->l1_thresh : nullptr;
        ff.frame_hw = (const int *)frame_hw;
        return run(p.kernel == FUSED_FRAMES_B6 ? k_iterate<4, 6, FusedArgsFrames> : k_iterate<4, SC_BMAX, FusedArgsFrames>, b->S, 1, ff);
    }
    case FUSED_FIT2X: {
        // as many workgroups as the chip keeps resident; the scenes beyond them come from the launch's queue
        // (a counter in the workspace, zeroed on the stream in front of the launch)
        int n_wg = 0;
        if ((rc = fit2x_resident_workgroups(p.lds, &n_wg))) return rc;
        if (n_wg > b->S || (sw.persist_dbg & 4)) n_wg = b->S;                  // (4: diagnostic, one workgroup per scene)
        int *queue = ws_at<int>(b, l.fit2x_queue);
        HIP_TRY(hipMemsetAsync(queue, 0, sizeof(int), st));
        if (done) *done = n_iter;
        return run(k_fit2x, n_wg, n_iter, f, n_iter | ((sw.persist_dbg & 1) << 30), queue, n_wg);
    }
    case FUSED_ITERATE2_EXACT: return run(k_iterate2<4, 5, 64>, b->S, 1, f);
    case FUSED_ITERATE2: return run(k_iterate2<4, 5>, b->S, 1, f);
    case FUSED_B6: return run(k_iterate<4, 6>, b->S, 1, f);
    default: return run(k_iterate<4, SC_BMAX>, b->S, 1, f);
    }
}

__global__ void k_count_active(const int *active, int S, int *out)
{
    int c = 0;
    for (int i = threadIdx.x; i < S; i += blockDim.x) c += active[i] != 0;
    c = (int)wave_sum((float)c);
    __shared__ int tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) atomicAdd(&tot, c);
    __syncthreads();
    if (threadIdx.x == 0) *out = tot;
}

// ---- the iteration driver.  Every fit entry point is fit_loop around a front half -- the fused launch, the general
// step, the prior step or the observation step -- that ends in iteration_tail (the fused kernels hold theirs).
// iterate(want, join, &did) runs at least one iteration: `want` is the number up to the next host look or the end (only
// the persistent k_fit2x launch covers more than one and says so in `did`); `join`: the look or the end comes next,
// so everything must be ordered on the caller's stream when it returns.  Returns the iterations launched.
template <typename Iterate>
static int fit_loop(const scarlet_batch *b, const WsLayout &l, int max_iter, int check_every, hipStream_t st, Iterate iterate)
{
    int rc, launched = 0;
    while (launched < max_iter) {
        int want = max_iter - launched, did = 1;
        if (check_every > 0 && check_every - launched % check_every < want) want = check_every - launched % check_every;
        if ((rc = iterate(want, want == 1, &did))) return rc;
        launched += did;
        if (check_every > 0 && launched % check_every == 0 && launched < max_iter) {
            // the host's look at `active`: every scene converged ends the call
            int h_count = 0, *d_count = ws_at<int>(b, l.active_count);
            hipLaunchKernelGGL(k_count_active, dim3(1), dim3(SC_BLOCK), 0, st, b->active, b->S, d_count);
            HIP_TRY(hipMemcpyAsync(&h_count, d_count, sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (h_count == 0) break;
        }
    }
    return launched;
}
// the constraint pipeline and the convergence test of one iteration
static int iteration_tail(scarlet_batch *b, const WsLayout &l, double e_rel, void *stream, const UpdateOpts &o)
{
    int rc;
    hipStream_t st = (hipStream_t)stream;
    prof_start(2, st);
    if ((rc = launch_update(b, l, 1, stream, o))) return rc;
    prof_stop(st); prof_start(3, st);
    if ((rc = launch_converge(b, l, e_rel, stream))) return rc;
    prof_stop(st);
    return SCARLET_OK;
}

// ---- components with a Prior (prior.h)
// buffer 1-cur holds the raw gradients (backward_impl with raw_gradient = 1): step them in place
static int launch_prior_step(const scarlet_batch *b, const scarlet_prior *p, void *stream)
{
    PriorArgs a;
    a.S = b->S; a.K = b->K; a.B = b->B; a.HW = b->H * b->W;
    a.sed[0] = b->sed[0]; a.sed[1] = b->sed[1]; a.morph[0] = b->morph[0]; a.morph[1] = b->morph[1];
    a.cur = b->cur; a.active = b->active; a.ncomp = b->n_components;
    a.fix_sed = b->fix_sed; a.fix_morph = b->fix_morph; a.lipschitz = b->lipschitz;
    a.p = *p;
    const uintptr_t bits = (uintptr_t)b->morph[0] | (uintptr_t)b->morph[1] | (uintptr_t)p->grad_morph | (uintptr_t)p->quad_morph_target;
    const bool vec = (a.HW & 3) == 0 && (bits & 15) == 0;
    const dim3 grid((unsigned)(b->S * b->K), (unsigned)((a.HW + SC_PRIOR_PIX - 1) / SC_PRIOR_PIX));
    hipStream_t st = (hipStream_t)stream;
    prof_start(6, st);
    if (vec) hipLaunchKernelGGL(k_prior_step<true>, grid, dim3(SC_BLOCK), 0, st, a);
    else hipLaunchKernelGGL(k_prior_step<false>, grid, dim3(SC_BLOCK), 0, st, a);
    prof_stop(st);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}


// The bodies of the entry points, each behind its host check.  `p` NULL: no prior; `c` NULL or all-NULL: the batch's scalars.
// raw_gradient = 1 with a prior: buffer 1-cur receives the gradients, the prior's step turns them into the stepped factors
static int backward_call(scarlet_batch *b, const scarlet_prior *p, int approximate_L, int raw_gradient, void *stream)
{
    int rc = check_counts(b, stream);
    if (!rc) rc = backward_impl(b, ws_layout(b, WS_FIX), approximate_L, raw_gradient, stream);
    return rc || !p ? rc : launch_prior_step(b, p, stream);
}
extern "C" int scarlet_backward_step(scarlet_batch *b, int approximate_L, void *stream)
{
    const int rc = check_call(b, false, nullptr, false, nullptr);
    return rc ? rc : backward_call(b, nullptr, approximate_L, 0, stream);
}
extern "C" int scarlet_backward_gradients(scarlet_batch *b, int approximate_L, void *stream)
{
    const int rc = check_call(b, false, nullptr, false, nullptr);
    return rc ? rc : backward_call(b, nullptr, approximate_L, 1, stream);
}
extern "C" int scarlet_backward_step_prior(scarlet_batch *b, const scarlet_prior *p, int approximate_L, void *stream)
{
    const int rc = check_call(b, false, nullptr, true, p);
    return rc ? rc : backward_call(b, p, approximate_L, 1, stream);
}

// ---- one request (scarlet_fit_request) behind every entry point that fits or updates.  A named entry point fills the
// request from its arguments and differs from the others only in its Rules; check_request (below, with the observations)
// is the one host-side check, and DESIGN.md 5i the table of what goes together.
enum {
    NEED_C = 1, NEED_P = 2, NEED_F = 4, NEED_O = 8, NEED_LOWRES = 16, NEED_LRF = 32,       // members that may not be NULL
    FRAMES_LATE = 64,        // frames = NULL is found after the batch's own checks (scarlet_fit_frames, _frames_grouped: they
                             // check the batch first), everywhere else before them
    GROUP_FRAMES = 128, GROUP_OPTIONS = 256,               // b->group is accepted with frame_hw / with options
    MULTI = 512,             // fits r.obs (n_obs 1..8); without: the batch's own images
    LARGE = 1024,            // low-resolution observations beyond LDS take the streamed form
    NO_COUNTS = 2048,        // scarlet_fit_multi: n_components on the state or an observation is refused first
};
struct Rules { unsigned flags; int bmax; };                // bmax: SC_BMAX, or SC_CMAX (the state's channel count then decides)
static const Rules RULES_ONE = {GROUP_FRAMES | GROUP_OPTIONS, SC_BMAX}, RULES_MANY = {MULTI | LARGE, SC_CMAX};   // scarlet_fit_with
static int check_request(const scarlet_batch *b, const scarlet_fit_request &r, const Rules &u);
static scarlet_fit_request loop_request(int max_iter, double e_rel, int approximate_L, int check_every,
                                        scarlet_batch *const *obs = nullptr, const int32_t *band0 = nullptr, int n_obs = 0)
{
    scarlet_fit_request r = {};
    r.obs = obs; r.band0 = band0; r.n_obs = n_obs;
    r.max_iter = max_iter; r.e_rel = e_rel; r.approximate_L = approximate_L; r.check_every = check_every;
    return r;
}
// what the constraint pipeline reads of a request: an all-NULL struct counts as none
static UpdateOpts update_opts(const scarlet_fit_request &r)
{
    return {r.prior ? r.prior->L_comp : nullptr, cons_any(r.constraints) ? r.constraints : nullptr, 0,
            r.frames ? r.frames->frame_hw : nullptr, opts_any(r.options) ? r.options : nullptr};
}

static int update_call(scarlet_batch *b, const scarlet_fit_request &r, int in_iteration, void *stream)
{
    UpdateOpts uo = update_opts(r);
    int rc = check_counts(b, stream);
    if (!rc) rc = check_frames(b, uo.frame_hw, stream);
    // the constructors' call (in_iteration = 0) ignores `active`: a scene the initialisation refused stays untouched
    // (BAD_COUNT scenes have no present component, scene_ncomp), and so does one whose options are refused here
    const int skip = ((uo.cons || uo.upd) && !in_iteration) ? SCARLET_STATUS_BAD_INIT | SCARLET_STATUS_BAD_COUNT : 0;
    if (!rc) rc = check_options(b, uo.upd, in_iteration ? 1 : 0, skip, stream, uo.frame_hw ? SCARLET_STATUS_BAD_FRAME : 0);
    if (rc) return rc;
    uo.skip_status = (uo.upd && !in_iteration) ? skip | SCARLET_STATUS_BAD_OPTION : skip;
    return launch_update(b, ws_layout(b, WS_PEEK), in_iteration ? 1 : 0, stream, uo);
}
// (of the request only constraints, prior, options and frames are read)
static int update_with(scarlet_batch *b, const scarlet_constraints *c, const scarlet_prior *p, const scarlet_update_options *o,
                       const scarlet_frames *f, const Rules &u, int in_iteration, void *stream)
{
    scarlet_fit_request r = {};
    r.constraints = c; r.prior = p; r.options = o; r.frames = f;
    const int rc = check_request(b, r, u);
    return rc ? rc : update_call(b, r, in_iteration, stream);
}
extern "C" int scarlet_source_update(scarlet_batch *b, int in_iteration, void *stream)
{
    return update_with(b, nullptr, nullptr, nullptr, nullptr, {0, SC_BMAX}, in_iteration, stream);
}
extern "C" int scarlet_source_update_prior(scarlet_batch *b, const scarlet_prior *p, int in_iteration, void *stream)
{
    return update_with(b, nullptr, p, nullptr, nullptr, {NEED_P, SC_BMAX}, in_iteration, stream);
}
extern "C" int scarlet_source_update_constrained(scarlet_batch *b, const scarlet_constraints *c, const scarlet_prior *p,
                                                 int in_iteration, void *stream)
{
    return update_with(b, c, p, nullptr, nullptr, {NEED_C, SC_BMAX}, in_iteration, stream);
}
extern "C" int scarlet_source_update_with(scarlet_batch *b, const scarlet_fit_request *r, int in_iteration, void *stream)
{
    if (!r) return set_err(SCARLET_E_ARG, "null request");
    return update_with(b, r->constraints, r->prior, r->options, r->frames, RULES_ONE, in_iteration, stream);
}

// One observation: the fused launch where it applies (never with a prior), two half-batches on two streams where the
// layout splits the batch (see split_views; never with a prior), the general step otherwise.
// frame_hw: the scenes' own frames (never with a prior), or NULL
// upd: update options (never with a prior): the general step on one pipeline -- no one-launch iteration, no box stage
static int fit_call(scarlet_batch *b, const scarlet_fit_request &r, void *stream)
{
    int rc;
    const UpdateOpts uo = update_opts(r);
    const scarlet_constraints *cons = uo.cons;
    const scarlet_prior *p = r.prior;
    const scarlet_update_options *upd = uo.upd;
    const int32_t *frame_hw = uo.frame_hw;
    const int max_iter = r.max_iter, approximate_L = r.approximate_L, check_every = r.check_every;
    const double e_rel = r.e_rel;
    if ((rc = check_counts(b, stream)) || (rc = check_frames(b, frame_hw, stream)) ||
        (rc = check_options(b, upd, 1, 0, stream, frame_hw ? SCARLET_STATUS_BAD_FRAME : 0)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const WsLayout l = ws_layout(b, WS_FIX);
    if (upd)     // gradients, step, the constraint kernels' options instances (on the scenes' own frames with frame_hw), convergence test
        return fit_loop(b, l, max_iter, check_every, st, [&](int, bool, int *) -> int {
            const int r = backward_impl(b, l, approximate_L, 0, stream);
            return r ? r : iteration_tail(b, l, e_rel, stream, uo);
        });
    if (p)       // gradients, prior step, constraints, convergence test
        return fit_loop(b, l, max_iter, check_every, st, [&](int, bool, int *) -> int {
            int r = backward_impl(b, l, approximate_L, 1, stream);
            if (!r) r = launch_prior_step(b, p, stream);
            return r ? r : iteration_tail(b, l, e_rel, stream, uo);
        });
    if (fused_ok(b, approximate_L, frame_hw != nullptr))      // up to the next host look in one launch where the persistent kernel applies
        return fit_loop(b, l, max_iter, check_every, st,
                        [&](int want, bool, int *did) { return launch_fused(b, l, e_rel, stream, want, did, cons, frame_hw); });
    SideStream *side = nullptr;
    if (two_pipelines(l) && (rc = side_stream(&side))) return rc;
    if (!side)
        return fit_loop(b, l, max_iter, check_every, st, [&](int, bool, int *) -> int {
            const int r = backward_impl(b, l, approximate_L, 0, stream);
            return r ? r : iteration_tail(b, l, e_rel, stream, uo);
        });
    scarlet_batch v[2];
    WsLayout lv[2];
    scarlet_constraints cv[2];
    split_views(b, l, v, lv, cons, cv);
    hipStream_t sv[2] = {st, side->st};
    bool forked = false;
    // the second stream's work ordered into the caller's (after an error too: whatever the caller enqueues next waits)
    auto join_side = [&]() {
        const bool ok = hipEventRecord(side->ev[1], side->st) == hipSuccess && hipStreamWaitEvent(st, side->ev[1], 0) == hipSuccess;
        forked = false;
        return ok;
    };
    auto bail = [&](int code) { if (forked) (void)join_side(); return code; };
    return fit_loop(b, l, max_iter, check_every, st, [&](int, bool join, int *) -> int {
        int r;
        if (!forked) {
            HIP_TRY(hipEventRecord(side->ev[0], st));
            HIP_TRY(hipStreamWaitEvent(side->st, side->ev[0], 0));
            forked = true;          // (from here on an error joins)
        }
        for (int h = 0; h < 2; ++h) {
            // (a view's frames: advanced to its first scene, where batch_view advances n_components)
            const UpdateOpts uh = {nullptr, cons ? &cv[h] : nullptr, 0, frame_hw ? frame_hw + 2 * (size_t)(h ? l.n0 : 0) : nullptr};
            if ((r = backward_impl(&v[h], lv[h], approximate_L, 0, sv[h])) || (r = iteration_tail(&v[h], lv[h], e_rel, sv[h], uh)))
                return bail(r);
        }
        if (join && !join_side()) return set_err(SCARLET_E_HIP, "HIP call failed in the two-pipeline loop: join");
        return SCARLET_OK;
    });
}
// check and body of the entry points that fit the batch's own images
static int fit_one(scarlet_batch *b, const scarlet_fit_request &r, const Rules &u, void *stream)
{
    const int rc = check_request(b, r, u);
    return rc ? rc : fit_call(b, r, stream);
}
extern "C" int scarlet_fit(scarlet_batch *b, int max_iter, double e_rel, int approximate_L,
                           int check_every, void *stream)
{
    return fit_one(b, loop_request(max_iter, e_rel, approximate_L, check_every), {0, SC_BMAX}, stream);
}
extern "C" int scarlet_fit_prior(scarlet_batch *b, const scarlet_prior *p, int max_iter, double e_rel, int approximate_L,
                                 int check_every, void *stream)
{
    scarlet_fit_request r = loop_request(max_iter, e_rel, approximate_L, check_every);
    r.prior = p;
    return fit_one(b, r, {NEED_P, SC_BMAX}, stream);
}
extern "C" int scarlet_fit_constrained(scarlet_batch *b, const scarlet_constraints *c, const scarlet_prior *p, int max_iter,
                                       double e_rel, int approximate_L, int check_every, void *stream)
{
    scarlet_fit_request r = loop_request(max_iter, e_rel, approximate_L, check_every);
    r.constraints = c; r.prior = p;
    return fit_one(b, r, {NEED_C, SC_BMAX}, stream);
}

// ---- update options (scarlet_update_options); one with every member NULL is the stock pipeline
extern "C" int scarlet_fit_options(scarlet_batch *b, const scarlet_constraints *c, const scarlet_update_options *o, int max_iter,
                                   double e_rel, int approximate_L, int check_every, void *stream)
{
    scarlet_fit_request r = loop_request(max_iter, e_rel, approximate_L, check_every);
    r.constraints = c; r.options = o;
    return fit_one(b, r, {NEED_O, SC_BMAX}, stream);
}
extern "C" int scarlet_source_update_options(scarlet_batch *b, const scarlet_constraints *c, const scarlet_update_options *o,
                                             int in_iteration, void *stream)
{
    return update_with(b, c, nullptr, o, nullptr, {NEED_O, SC_BMAX}, in_iteration, stream);
}

// ---- scenes with their own frames (scarlet_frames); the device check of the entries, alone, for callers that step
// phase by phase.  With group (_grouped: the layers of multi-component sources) k_group_centers<RAGGED> measures each
// source's shared centre on its scene's own frame in front of the RAGGED update kernels; with update options (_options:
// a catalogue batch whose sources carry the stock update functions' options) the RAGGED x OPTIONS instances of the
// constraint kernels run.  The device checks run in the order counts, frames, options (fit_call, update_call).
extern "C" int scarlet_fit_frames(scarlet_batch *b, const scarlet_frames *f, const scarlet_constraints *c, int max_iter,
                                  double e_rel, int approximate_L, int check_every, void *stream)
{
    scarlet_fit_request r = loop_request(max_iter, e_rel, approximate_L, check_every);
    r.frames = f; r.constraints = c;
    return fit_one(b, r, {NEED_F | FRAMES_LATE, SC_BMAX}, stream);
}
extern "C" int scarlet_source_update_frames(scarlet_batch *b, const scarlet_frames *f, const scarlet_constraints *c,
                                            int in_iteration, void *stream)
{
    return update_with(b, c, nullptr, nullptr, f, {NEED_F | FRAMES_LATE, SC_BMAX}, in_iteration, stream);
}
static int check_frames_grouped_call(const scarlet_frames *f)
{
    return f ? SCARLET_OK : set_err(SCARLET_E_ARG, "frames is NULL (pass a scarlet_frames with frame_hw = NULL for uniform frames)");
}
extern "C" int scarlet_fit_frames_grouped(scarlet_batch *b, const scarlet_frames *f, const scarlet_constraints *c, int max_iter,
                                          double e_rel, int approximate_L, int check_every, void *stream)
{
    scarlet_fit_request r = loop_request(max_iter, e_rel, approximate_L, check_every);
    r.frames = f; r.constraints = c;
    return fit_one(b, r, {NEED_F | FRAMES_LATE | GROUP_FRAMES, SC_BMAX}, stream);
}
extern "C" int scarlet_source_update_frames_grouped(scarlet_batch *b, const scarlet_frames *f, const scarlet_constraints *c,
                                                    int in_iteration, void *stream)
{
    return update_with(b, c, nullptr, nullptr, f, {NEED_F | FRAMES_LATE | GROUP_FRAMES, SC_BMAX}, in_iteration, stream);
}
extern "C" int scarlet_fit_frames_options(scarlet_batch *b, const scarlet_frames *f, const scarlet_constraints *c,
                                          const scarlet_update_options *o, int max_iter, double e_rel, int approximate_L,
                                          int check_every, void *stream)
{
    scarlet_fit_request r = loop_request(max_iter, e_rel, approximate_L, check_every);
    r.frames = f; r.constraints = c; r.options = o;
    return fit_one(b, r, {NEED_F | NEED_O | GROUP_FRAMES | GROUP_OPTIONS, SC_BMAX}, stream);
}
extern "C" int scarlet_source_update_frames_options(scarlet_batch *b, const scarlet_frames *f, const scarlet_constraints *c,
                                                    const scarlet_update_options *o, int in_iteration, void *stream)
{
    return update_with(b, c, nullptr, o, f, {NEED_F | NEED_O | GROUP_FRAMES | GROUP_OPTIONS, SC_BMAX}, in_iteration, stream);
}
extern "C" int scarlet_check_frames(scarlet_batch *b, const scarlet_frames *f, void *stream)
{
    int rc = check_call(b, false, nullptr, false, nullptr);
    if (!rc) rc = check_frames_call(b, f);
    return rc ? rc : check_frames(b, f->frame_hw, stream);
}

// ---- a low-resolution observation (lowres.h): the shapes, the workspace and the host checks
static LowresDims lowres_dims(const scarlet_lowres *lr, int H, int W, int B)
{
    LowresDims d;
    d.H = H; d.W = W; d.h = lr->h; d.w = lr->w; d.nfy = lr->nfy; d.nfx = lr->nfx; d.B = B;
    return d;
}
static LowresDims lowres_dims(const scarlet_batch *state, const scarlet_batch *ob, const scarlet_lowres *lr)
{
    return lowres_dims(lr, state->H, state->W, ob->B);
}
static LowresFactors lowres_factors(const scarlet_lowres *lr)
{
    LowresFactors f;
    f.uy = (const float2 *)lr->uy; f.ux = (const float2 *)lr->ux; f.vy = (const float2 *)lr->vy; f.vx = (const float2 *)lr->vx;
    f.dhat = (const float2 *)lr->dhat; f.v_per_scene = lr->v_per_scene; f.dhat_per_scene = lr->dhat_per_scene;
    return f;
}
// the G planes [S][B][H][W] come first, the per-plane losses [S][B] (float64) after them, 16-byte aligned
static int64_t lowres_loss_offset(const scarlet_batch *state, const scarlet_batch *ob)
{
    const int64_t g = (int64_t)state->S * ob->B * state->H * state->W * (int64_t)sizeof(float);
    return (g + 15) & ~(int64_t)15;
}
// shapes, pointers and limits of one scarlet_lowres for a model frame of H x W and B bands; no device call
static int check_lowres(const scarlet_lowres *lr, int H, int W, int B, bool need_workspace, bool large = false)
{
    if (!lr) return set_err(SCARLET_E_ARG, "null scarlet_lowres");
    if (lr->h < 1 || lr->w < 1 || lr->nfy < 1 || lr->nfx < 1 || H < 1 || W < 1 || B < 1 || lr->B != B)
        return set_err(SCARLET_E_ARG, "scarlet_lowres: bad shape");
    if (!lr->uy || !lr->ux || !lr->vy || !lr->vx || !lr->dhat)
        return set_err(SCARLET_E_ARG, "scarlet_lowres: null factor matrix");
    if (need_workspace && !lr->workspace) return set_err(SCARLET_E_ARG, "scarlet_lowres: null workspace");
    if (B > SC_BMAX) return set_err(SCARLET_E_NOTIMPL, "B > 8 bands is not supported by this build of the gradient kernels");
    const bool sides = H > SCARLET_MAX_SIDE || W > SCARLET_MAX_SIDE || lr->h > SCARLET_MAX_SIDE || lr->w > SCARLET_MAX_SIDE ||
                       lr->nfy > SCARLET_MAX_SIDE || lr->nfx > 2 * SCARLET_MAX_SIDE;
    if (large)           // (the streamed form of lowres_stream.h takes over where LDS ends)
        return sides ? set_err(SCARLET_E_NOTIMPL, "scarlet_lowres: sides above SCARLET_MAX_SIDE are not supported") : SCARLET_OK;
    if (sides)
        return set_err(SCARLET_E_NOTIMPL, "scarlet_lowres: the factor matrices and one model plane do not fit LDS");
    if (lowres_lds_bytes(lowres_dims(lr, H, W, B)) > LDS_LIMIT)
        return set_err(SCARLET_E_NOTIMPL, "scarlet_lowres: the factor matrices and one model plane do not fit LDS");
    return SCARLET_OK;
}

extern "C" int64_t scarlet_lowres_workspace_bytes(const scarlet_batch *state, const scarlet_batch *obs, const scarlet_lowres *lr)
{
    if (check_shape(state) || check_shape(obs)) return SCARLET_E_ARG;
    if (int rc = check_lowres(lr, state->H, state->W, obs->B, false)) return rc;
    return lowres_loss_offset(state, obs) + (int64_t)state->S * obs->B * (int64_t)sizeof(double);
}

static int lowres_op(bool adjoint, const float *in, int n, int H, int W, const scarlet_lowres *lr, const int32_t *band,
                     const int32_t *scene, float *out, void *stream)
{
    (void)hipGetLastError();
    if (n < 0) return set_err(SCARLET_E_ARG, "n < 0");
    if (int rc = check_lowres(lr, H, W, lr ? lr->B : 0, false)) return rc;
    if (!in || !out) return set_err(SCARLET_E_ARG, "null plane pointer");
    if (n == 0) return SCARLET_OK;
    LowresOpArgs a = {};
    a.d = lowres_dims(lr, H, W, lr->B); a.f = lowres_factors(lr); a.in = in; a.out = out; a.band = band; a.scene = scene; a.mfma = !opt(OPT_NO_LOWRES_MFMA);
    const size_t lds = lowres_lds_bytes(a.d);
    int rc;
    if (adjoint) {
        if ((rc = allow_lds(k_lowres_adjoint, lds))) return rc;
        hipLaunchKernelGGL(k_lowres_adjoint, dim3(n), dim3(SC_BLOCK), lds, (hipStream_t)stream, a);
    } else {
        if ((rc = allow_lds(k_lowres_render, lds))) return rc;
        hipLaunchKernelGGL(k_lowres_render, dim3(n), dim3(SC_BLOCK), lds, (hipStream_t)stream, a);
    }
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}
extern "C" int scarlet_lowres_render(const float *model, int n, int H, int W, const scarlet_lowres *lr, const int32_t *band,
                                     const int32_t *scene, float *out, void *stream)
{
    return lowres_op(false, model, n, H, W, lr, band, scene, out, stream);
}
extern "C" int scarlet_lowres_adjoint(const float *resid, int n, int H, int W, const scarlet_lowres *lr, const int32_t *band,
                                      const int32_t *scene, float *out, void *stream)
{
    return lowres_op(true, resid, n, H, W, lr, band, scene, out, stream);
}

// ---- the streamed form (lowres_stream.h): one launch per product over the planes of a chunk
static bool lowres_fits_lds(const LowresDims &d) { return lowres_lds_bytes(d) <= LDS_LIMIT; }
// the form a call of the *_large entry points takes: the LDS-resident kernels wherever they fit, unless LOWRES_STREAMED
static bool lowres_streamed(const LowresDims &d) { return opt(OPT_LOWRES_STREAMED) || !lowres_fits_lds(d); }
static LrsOperand lrs_real(const float *p, int rs, int cs, size_t plane)
{
    LrsOperand o = {p, rs, cs, 0, 0, plane, 0};
    return o;
}
// contiguous model planes [planes][H][W]
static LrsOperand lrs_planes(const float *p, const LowresDims &d) { return lrs_real(p, d.W, 1, (size_t)d.H * d.W); }
// a factor matrix of (re, im) pairs with strides in pairs, stacked along its first (1) or second (2) index
static LrsOperand lrs_factor(const float2 *p, int rs, int cs, int stack, int n, size_t scene)
{
    LrsOperand o = {(const float *)p, 2 * rs, 2 * cs, stack, n, 0, 2 * scene};
    return o;
}
static void lrs_gemm(hipStream_t st, bool mfma, const LrsOperand &a, const LrsOperand &b, float *c, int ldc, size_t c_plane,
                     int M, int N, int K, const LrsPlanes &pl, int planes)
{
    LrsGemm g = {a, b, c, ldc, c_plane, M, N, K, pl};
    const dim3 grid(((M + LRS_BM - 1) / LRS_BM) * ((N + LRS_BN - 1) / LRS_BN), planes);
    if (mfma) hipLaunchKernelGGL(k_lrs_gemm<true>, grid, dim3(SC_BLOCK), 0, st, g);
    else hipLaunchKernelGGL(k_lrs_gemm<false>, grid, dim3(SC_BLOCK), 0, st, g);
}
// the buffers of one chunk inside the scratch: the loss partials (float64) first, then M, A, B, Z, D
struct LrsBuffers {
    double *partials;
    float *m, *a, *b, *z, *d;
};
static LrsBuffers lrs_buffers(void *scratch, const LrsScratch &s, int chunk, bool fit)
{
    LrsBuffers u;
    u.partials = (double *)scratch;
    u.m = (float *)(u.partials + (fit ? (size_t)chunk * LRS_LOSS_BLOCKS : 0));
    u.a = u.m + chunk * s.m; u.b = u.a + chunk * s.a; u.z = u.b + chunk * s.b; u.d = u.z + chunk * s.b;
    return u;
}
static void lrs_expand(hipStream_t st, const LowresDims &d, const LowresFactors &f, const LrsBuffers &u, const LrsScratch &s,
                       const LrsPlanes &pl, int planes)
{
    LrsExpand e = {u.b, u.z, s.b, d.nfy, d.nfx, d.B, f, pl};
    hipLaunchKernelGGL(k_lrs_expand, dim3((d.nfy * d.nfx + SC_BLOCK - 1) / SC_BLOCK, planes), dim3(SC_BLOCK), 0, st, e);
}
// render of the chunk's planes: model (planes of H x W, an LrsOperand: lrs_planes for [planes][H][W]) -> out [planes][h][w]
// u_per_scene: uy and ux are one table per scene, as vy and vx are with v_per_scene (scenes with their own frames, whose
// tables are zero-padded to d: the chain runs on the padded extents and sums zeros there)
static void lrs_forward(hipStream_t st, bool mfma, const LowresDims &d, const LowresFactors &f, const LrsBuffers &u,
                        const LrsScratch &s, const LrsPlanes &pl, int planes, const LrsOperand &model, float *out,
                        bool u_per_scene = false)
{
    const int ny2 = 2 * d.nfy, nx2 = 2 * d.nfx;
    const size_t vy_scene = f.v_per_scene ? (size_t)d.h * d.nfy : 0, vx_scene = f.v_per_scene ? (size_t)d.w * d.nfx : 0;
    const size_t uy_scene = u_per_scene ? (size_t)d.nfy * d.H : 0, ux_scene = u_per_scene ? (size_t)d.nfx * d.W : 0;
    // T [H][2 nfx] = m [H][W] . (Re Ux | Im Ux)^T
    lrs_gemm(st, mfma, model, lrs_factor(f.ux, 1, d.W, 2, d.nfx, ux_scene), u.a, nx2, s.a, d.H, nx2, d.W, pl, planes);
    // C [2 nfy][2 nfx] = (Re Uy; Im Uy) [2 nfy][H] . T
    lrs_gemm(st, mfma, lrs_factor(f.uy, d.H, 1, 1, d.nfy, uy_scene), lrs_real(u.a, nx2, 1, s.a), u.b, nx2, s.b, ny2, nx2, d.H, pl,
             planes);
    lrs_expand(st, d, f, u, s, pl, planes);
    // R [2 nfy][w] = Z [2 nfy][2 nfx] . (Re Vx | Im Vx)^T = [Re R; -Im R]
    lrs_gemm(st, mfma, lrs_real(u.z, nx2, 1, s.b), lrs_factor(f.vx, 1, d.nfx, 1, d.nfx, vx_scene), u.a, d.w, s.a, ny2, d.w, nx2,
             pl, planes);
    // out [h][w] = (Re Vy | Im Vy) [h][2 nfy] . R
    lrs_gemm(st, mfma, lrs_factor(f.vy, d.nfy, 1, 2, d.nfy, vy_scene), lrs_real(u.a, d.w, 1, s.a), out, d.w, (size_t)d.h * d.w,
             d.h, d.w, ny2, pl, planes);
}
// adjoint of the chunk's planes: resid [planes][h][w] -> out [planes][H][W]
static void lrs_backward(hipStream_t st, bool mfma, const LowresDims &d, const LowresFactors &f, const LrsBuffers &u,
                         const LrsScratch &s, const LrsPlanes &pl, int planes, const float *resid, float *out,
                         bool u_per_scene = false)
{
    const int ny2 = 2 * d.nfy, nx2 = 2 * d.nfx;
    const size_t vy_scene = f.v_per_scene ? (size_t)d.h * d.nfy : 0, vx_scene = f.v_per_scene ? (size_t)d.w * d.nfx : 0;
    const size_t uy_scene = u_per_scene ? (size_t)d.nfy * d.H : 0, ux_scene = u_per_scene ? (size_t)d.nfx * d.W : 0;
    // A1 [2 nfy][w] = (Re Vy | Im Vy)^T . E
    lrs_gemm(st, mfma, lrs_factor(f.vy, 1, d.nfy, 1, d.nfy, vy_scene), lrs_real(resid, d.w, 1, (size_t)d.h * d.w), u.a, d.w, s.a,
             ny2, d.w, d.h, pl, planes);
    // C2 [2 nfy][2 nfx] = A1 . (Re Vx | Im Vx)
    lrs_gemm(st, mfma, lrs_real(u.a, d.w, 1, s.a), lrs_factor(f.vx, d.nfx, 1, 2, d.nfx, vx_scene), u.b, nx2, s.b, ny2, nx2, d.w,
             pl, planes);
    lrs_expand(st, d, f, u, s, pl, planes);
    // G1 [2 nfy][W] = Z [2 nfy][2 nfx] . (Re Ux; Im Ux) = [Re G1; -Im G1]
    lrs_gemm(st, mfma, lrs_real(u.z, nx2, 1, s.b), lrs_factor(f.ux, d.W, 1, 1, d.nfx, ux_scene), u.a, d.W, s.a, ny2, d.W, nx2, pl,
             planes);
    // G [H][W] = (Re Uy; Im Uy)^T . G1
    lrs_gemm(st, mfma, lrs_factor(f.uy, 1, d.H, 2, d.nfy, uy_scene), lrs_real(u.a, d.W, 1, s.a), out, d.W, (size_t)d.H * d.W, d.H, d.W,
             ny2, pl, planes);
}
// planes per chunk of a call: what the scratch was sized for, lowered by LOWRES_CHUNK (never raised)
static int lrs_chunk_now(const LrsScratch &s, int planes)
{
    const int sized = lrs_chunk(s, planes), asked = opt(OPT_LOWRES_CHUNK);
    return asked > 0 && asked < sized ? asked : sized;
}
// what one low-resolution observation of a fit runs per iteration in the streamed form
struct LrsFit {
    LowresArgs a;
    LrsScratch s;
    void *scratch;
    bool u_per_scene;               // scenes with their own frames (scarlet_lowres_frames): a.f.uy / ux hold one table per scene
};
static void lrs_fit_planes(hipStream_t st, const LrsFit &f)
{
    const LowresArgs &a = f.a;
    const LowresDims &d = a.d;
    const int planes = a.S * d.B, sized = lrs_chunk(f.s, planes), chunk = lrs_chunk_now(f.s, planes);
    const LrsBuffers u = lrs_buffers(f.scratch, f.s, sized, true);
    const size_t HW = (size_t)d.H * d.W;
    for (int p0 = 0; p0 < planes; p0 += chunk) {
        const int n = planes - p0 < chunk ? planes - p0 : chunk;
        const LrsPlanes pl = {nullptr, nullptr, a.active, d.B, p0};
        LrsModel m = {{a.sed[0], a.sed[1]}, {a.morph[0], a.morph[1]}, a.cur, a.ncomp, a.K, a.C, a.band0, (int)HW, u.m, f.s.m, pl};
        const int mblocks = (int)((HW + SC_BLOCK - 1) / SC_BLOCK);
        hipLaunchKernelGGL(k_lrs_model, dim3(mblocks < 1024 ? mblocks : 1024, n), dim3(SC_BLOCK), 0, st, m);
        lrs_forward(st, a.mfma != 0, d, a.f, u, f.s, pl, n, lrs_planes(u.m, d), u.d, f.u_per_scene);
        LrsResid r = {u.d, f.s.d, a.images, a.weights, a.weight_scalar, d.h * d.w, u.partials, a.loss_part, pl};
        hipLaunchKernelGGL(k_lrs_resid, dim3(LRS_LOSS_BLOCKS, n), dim3(SC_BLOCK), 0, st, r);
        hipLaunchKernelGGL(k_lrs_loss, dim3((n + SC_BLOCK - 1) / SC_BLOCK), dim3(SC_BLOCK), 0, st, r, n);
        lrs_backward(st, a.mfma != 0, d, a.f, u, f.s, pl, n, u.d, a.G + (size_t)p0 * HW, f.u_per_scene);
    }
}
static int64_t lowres_scratch_offset(const scarlet_batch *state, const scarlet_batch *ob)
{
    const int64_t o = lowres_loss_offset(state, ob) + (int64_t)state->S * ob->B * (int64_t)sizeof(double);
    return (o + 15) & ~(int64_t)15;
}

static int64_t lowres_large_workspace_bytes(const scarlet_batch *state, const scarlet_batch *obs, const scarlet_lowres *lr, int bmax)
{
    if (check_shape(state, bmax) || check_shape(obs)) return SCARLET_E_ARG;
    if (int rc = check_lowres(lr, state->H, state->W, obs->B, false, true)) return rc;
    // (the scratch of the streamed form always: an option changed between sizing and fitting cannot write past it)
    const LrsScratch s = lrs_scratch(lowres_dims(state, obs, lr), true);
    return lowres_scratch_offset(state, obs) + (int64_t)lrs_chunk(s, state->S * obs->B) * (int64_t)s.per_plane;
}
extern "C" int64_t scarlet_lowres_large_workspace_bytes(const scarlet_batch *state, const scarlet_batch *obs, const scarlet_lowres *lr)
{
    return lowres_large_workspace_bytes(state, obs, lr, SC_BMAX);
}
extern "C" int64_t scarlet_lowres_large_workspace_bytes_wide(const scarlet_batch *state, const scarlet_batch *obs,
                                                             const scarlet_lowres *lr)
{
    return lowres_large_workspace_bytes(state, obs, lr, SC_CMAX);
}

extern "C" int64_t scarlet_lowres_op_scratch_bytes(int n, int H, int W, const scarlet_lowres *lr)
{
    if (n < 0) return set_err(SCARLET_E_ARG, "n < 0");
    if (int rc = check_lowres(lr, H, W, lr ? lr->B : 0, false, true)) return rc;
    const LowresDims d = lowres_dims(lr, H, W, lr->B);
    if (n == 0 || !lowres_streamed(d)) return 0;
    const LrsScratch s = lrs_scratch(d, false);
    return (int64_t)lrs_chunk(s, n) * (int64_t)s.per_plane;
}

static int lowres_op_large(bool adjoint, const float *in, int n, int H, int W, const scarlet_lowres *lr, const int32_t *band,
                           const int32_t *scene, float *out, void *scratch, int64_t scratch_bytes, void *stream)
{
    (void)hipGetLastError();
    const int64_t need = scarlet_lowres_op_scratch_bytes(n, H, W, lr);
    if (need < 0) return (int)need;
    if (!in || !out) return set_err(SCARLET_E_ARG, "null plane pointer");
    if (need > 0 && (!scratch || scratch_bytes < need))
        return set_err(SCARLET_E_ARG, "scarlet_lowres: the scratch is smaller than scarlet_lowres_op_scratch_bytes()");
    if (n == 0) return SCARLET_OK;
    if (need == 0) return lowres_op(adjoint, in, n, H, W, lr, band, scene, out, stream);
    const LowresDims d = lowres_dims(lr, H, W, lr->B);
    const LowresFactors f = lowres_factors(lr);
    const LrsScratch s = lrs_scratch(d, false);
    const int sized = lrs_chunk(s, n), chunk = lrs_chunk_now(s, n);
    const LrsBuffers u = lrs_buffers(scratch, s, sized, false);
    const bool mfma = !opt(OPT_NO_LOWRES_MFMA);
    const size_t HW = (size_t)H * W, hw = (size_t)d.h * d.w;
    for (int p0 = 0; p0 < n; p0 += chunk) {
        const int m = n - p0 < chunk ? n - p0 : chunk;
        const LrsPlanes pl = {band, scene, nullptr, 0, p0};
        if (adjoint) lrs_backward((hipStream_t)stream, mfma, d, f, u, s, pl, m, in + p0 * hw, out + p0 * HW);
        else lrs_forward((hipStream_t)stream, mfma, d, f, u, s, pl, m, lrs_planes(in + p0 * HW, d), out + p0 * hw);
    }
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}
extern "C" int scarlet_lowres_render_large(const float *model, int n, int H, int W, const scarlet_lowres *lr, const int32_t *band,
                                           const int32_t *scene, float *out, void *scratch, int64_t scratch_bytes, void *stream)
{
    return lowres_op_large(false, model, n, H, W, lr, band, scene, out, scratch, scratch_bytes, stream);
}
extern "C" int scarlet_lowres_adjoint_large(const float *resid, int n, int H, int W, const scarlet_lowres *lr, const int32_t *band,
                                            const int32_t *scene, float *out, void *scratch, int64_t scratch_bytes, void *stream)
{
    return lowres_op_large(true, resid, n, H, W, lr, band, scene, out, scratch, scratch_bytes, stream);
}

// ---- several observations per blend (multiobs.h)
// L_sed of the state's current morphologies (blend.py:186-218, before the factor n_obs): the Gram matrix and its largest
// eigenvalue by the existing code of the K range, or its trace with approximate constants
static int obs_lipschitz_sed(scarlet_batch *state, const WsLayout &l, const GradArgs &ga, int approximate_L, hipStream_t st)
{
    if (l.grad == GRAD_HUGEK) launch_huge_lipschitz(ga, huge_args(state, l), approximate_L, st);
    else launch_bigk_lipschitz(ga, (state->K + SC_CHUNK - 1) / SC_CHUNK, approximate_L ? 1 : 2, st);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}

// the instance of k_obs_contract_wide that contract_plan chose
typedef void (*ObsKernel)(ObsArgs);
template <int CW, bool PRIOR>
static ObsKernel wide_contract_waves(int nw)
{
    return nw == 4 ? k_obs_contract_wide<CW, 4, PRIOR> : nw == 2 ? k_obs_contract_wide<CW, 2, PRIOR> : k_obs_contract_wide<CW, 1, PRIOR>;
}
static ObsKernel wide_contract_kernel(const ContractPlan &cp, bool prior)
{
    if (cp.cw == 16) return prior ? wide_contract_waves<16, true>(cp.nw) : wide_contract_waves<16, false>(cp.nw);
    return prior ? wide_contract_waves<32, true>(cp.nw) : wide_contract_waves<32, false>(cp.nw);
}

// Several observations: one pipeline, every iteration the observation step (the observations' G planes, the contraction
// over them, L x n_obs, the step) and the tail.  `p` NULL: no prior; given: the passes that write a step are the PRIOR
// instances (multiobs.h), which read the prior in the pass that already holds the factors and their gradients
// frame_hw: the scenes' own frames (no prior), or NULL.
// lrf: NULL, or n_obs pointers: the per-scene tables of the low-resolution observations of such scenes
// (check_request has checked them against `lowres` and frame_hw).
// Only the tail and the low-resolution kernels of such scenes read the frames: the morphologies and the observations' weights are zero outside a scene's frame, so the
// planes, the contraction and the Lipschitz constants sum nothing there, and what a PSF's adjoint and the step write
// outside is zeroed by the RAGGED constraint kernels before anything reads it
static int fit_observations_call(scarlet_batch *state, const scarlet_fit_request &r, bool large, void *stream)
{
    int rc;
    const UpdateOpts uo = update_opts(r);     // (with a prior the sparse_l0 / sparse_l1 cut uses each component's own step, update.py:71-82)
    const scarlet_update_options *upd = uo.upd;        // (update options of the state: the tail reads them)
    const scarlet_prior *p = r.prior;
    const int32_t *frame_hw = uo.frame_hw, *band0 = r.band0;
    scarlet_batch *const *obs = r.obs;
    const scarlet_lowres *const *lowres = r.lowres;
    const scarlet_lowres_frames *const *lrf = r.lowres_frames;
    const int n_obs = r.n_obs, max_iter = r.max_iter, approximate_L = r.approximate_L, check_every = r.check_every;
    const double e_rel = r.e_rel;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = check_counts(state, stream)) || (rc = check_frames(state, frame_hw, stream)) || (rc = check_options(state, upd, 1, 0, stream)))
        return rc;
    for (int o = 0; lrf && o < n_obs; ++o)
        if (lrf[o] && (rc = check_lowres_frames(state, lrf[o], frame_hw, lowres_dims(state, obs[o], lowres[o]), stream))) return rc;
    const WsLayout l = ws_layout(state, WS_FIX);
    WsLayout lo[SC_MAX_OBS];
    ObsArgs m = {};
    m.S = state->S; m.K = state->K; m.C = state->B; m.H = state->H; m.W = state->W; m.HW = state->H * state->W;
    m.T = n_tiles(state); m.n_obs = n_obs;
    m.sed[0] = state->sed[0]; m.sed[1] = state->sed[1]; m.morph[0] = state->morph[0]; m.morph[1] = state->morph[1];
    m.cur = state->cur; m.active = state->active; m.ncomp = state->n_components;
    m.fix_sed = state->fix_sed; m.fix_morph = state->fix_morph;
    m.partials = ws_at<double>(state, l.partials);
    m.lipschitz = state->lipschitz; m.mse = state->mse; m.mse_capacity = state->mse_capacity; m.it = state->it;
    if (p) m.p = *p;
    for (int o = 0; o < n_obs; ++o) {
        const scarlet_batch *ob = obs[o];
        lo[o] = ws_layout(ob, WS_FIX);
        ObsView &v = m.obs[o];
        v.images = ob->images; v.weights = ob->weights; v.weight_scalar = ob->weight_scalar;
        v.G = nullptr; v.loss_part = nullptr; v.Fy = ob->H; v.Fx = ob->W; v.oy = v.ox = 0;
        v.B = ob->B; v.band0 = band0[o];
        if (ob->diff_kernel && !lo[o].psf) return set_err(SCARLET_E_ARG, "diff_kernel without psf_h, psf_w");
    }
    // low-resolution observations (lowres.h): their G planes and per-plane losses lie in the scarlet_lowres workspace
    // (`large`, scarlet_fit_observations_lowres_large: those that do not fit LDS take the streamed form, lowres_stream.h)
    LowresFramesArgs la[SC_MAX_OBS] = {};
    size_t la_lds[SC_MAX_OBS] = {};
    LrsFit ls[SC_MAX_OBS] = {};
    bool streamed[SC_MAX_OBS] = {};
    for (int o = 0; o < n_obs; ++o) {
        const scarlet_lowres *lr = lowres ? lowres[o] : nullptr;
        if (!lr) continue;
        const scarlet_lowres_frames *lf = lrf ? lrf[o] : nullptr;
        LowresFramesArgs &a = la[o];
        a.d = lowres_dims(state, obs[o], lr); a.f = lowres_factors(lr);
        if (lf) {          // (a.d: the maxima, the shape of the padded blocks; every table is per scene)
            a.f.uy = (const float2 *)lf->uy; a.f.ux = (const float2 *)lf->ux;
            a.fr.dims = (const int *)lf->dims; a.fr.frame_hw = (const int *)frame_hw;
        }
        a.S = state->S; a.K = state->K; a.C = state->B; a.band0 = band0[o];
        a.sed[0] = state->sed[0]; a.sed[1] = state->sed[1]; a.morph[0] = state->morph[0]; a.morph[1] = state->morph[1];
        a.cur = state->cur; a.active = state->active; a.ncomp = state->n_components;
        a.images = obs[o]->images; a.weights = obs[o]->weights; a.weight_scalar = obs[o]->weight_scalar;
        a.G = (float *)lr->workspace;
        a.loss_part = (double *)((char *)lr->workspace + lowres_loss_offset(state, obs[o]));
        a.mfma = !opt(OPT_NO_LOWRES_MFMA);
        streamed[o] = large && lowres_planes_plan(a.d, opt(OPT_LOWRES_STREAMED) != 0).form == LOWRES_PLANES_STREAMED;
        if (streamed[o]) {
            ls[o].a = a; ls[o].s = lrs_scratch(a.d, true);
            ls[o].scratch = (char *)lr->workspace + lowres_scratch_offset(state, obs[o]);
            ls[o].u_per_scene = lf != nullptr;
        } else {
            la_lds[o] = lowres_lds_bytes(a.d);
            if ((rc = lf ? allow_lds(k_lowres_planes_frames, la_lds[o]) : allow_lds(k_lowres_planes, la_lds[o]))) return rc;
        }
        ObsView &v = m.obs[o];
        v.G = a.G; v.loss_part = a.loss_part; v.Fy = state->H; v.Fx = state->W; v.oy = v.ox = 0;
    }
    // the state's gradient arguments: its partials (engine.h layout over the C channels) feed the Gram / lambda_max code
    const GradArgs ga = grad_args(state, l, approximate_L, 0);
    // K <= 8: the contraction also sums the Gram matrix (no Gram pass); its lambda_max is found in k_obs_head
    // more than 8 model channels (scarlet_fit_observations_wide): the wide contraction and lambda_max (multiobs_wide.h);
    // the Gram comes from the Gram passes for every K
    const bool wide = state->B > SC_BMAX;
    const ContractPlan cp = contract_plan(state->K, state->B, p != nullptr);
    const bool small = !wide && state->K <= SC_KMAX && l.grad == GRAD_SMALL;
    ObsKernel contract = wide ? wide_contract_kernel(cp, false) : small ? k_obs_contract<SC_KMAX, false> : k_obs_contract<0, false>;
    // the pass that writes the step (OBS_FULL / OBS_STEP); OBS_PARTIALS writes none and stays the plain instance
    ObsKernel contract_step = !p ? contract : wide ? wide_contract_kernel(cp, true)
                                    : small ? k_obs_contract<SC_KMAX, true> : k_obs_contract<0, true>;
    auto head = p ? k_obs_head<true> : k_obs_head<false>;
    m.head_lsed = small && !approximate_L;
    const size_t lds = wide ? cp.lds : obs_contract_lds(state->K), lmorph_lds = wide ? wide_lmorph_lds(state->K, state->B) : 0;
    if (wide && (cp.kernel != CONTRACT_WIDE || lds > LDS_LIMIT))
        return set_err(SCARLET_E_NOTIMPL, "no form of the wide contraction for this K and C");
    if ((rc = allow_lds(contract, lds)) || (rc = allow_lds(contract_step, lds))) return rc;
    if (wide && (rc = allow_lds(k_wide_lmorph, lmorph_lds))) return rc;
    const dim3 grid(m.T, m.S), block(wide ? cp.block : SC_BLOCK);
    auto lmorph = [&]() {
        if (wide) hipLaunchKernelGGL(k_wide_lmorph, dim3(m.S), dim3(SC_BLOCK), lmorph_lds, st, ga);
        else hipLaunchKernelGGL(k_bigk_lmorph<SC_KHUGE>, dim3(m.S), dim3(SC_WAVE), 0, st, ga);
    };
    return fit_loop(state, l, max_iter, check_every, st, [&](int, bool, int *) -> int {
        prof_start(0, st);
        for (int o = 0; o < n_obs; ++o) {
            if (lowres && lowres[o]) {
                if (streamed[o]) lrs_fit_planes(st, ls[o]);
                else if (la[o].fr.dims) hipLaunchKernelGGL(k_lowres_planes_frames, dim3(m.S), dim3(SC_BLOCK), la_lds[o], st, la[o]);
                else hipLaunchKernelGGL(k_lowres_planes, dim3(m.S), dim3(SC_BLOCK), la_lds[o], st, (LowresArgs)la[o]);
                continue;
            }
            if (!lo[o].psf) continue;
            hipLaunchKernelGGL(k_obs_slice, dim3(m.S), dim3(SC_BLOCK), 0, st, m, band0[o], obs[o]->B, obs[o]->sed[0]);
            // model planes from the STATE's morphologies and the observation's band slice of the SEDs (its own sed[0])
            PsfArgs a = psf_args(obs[o], lo[o], state, obs[o]->sed[0], obs[o]->sed[0], nullptr, nullptr, 0, 0);
            if ((rc = psf_gradient_planes(obs[o], lo[o], a, PSF_MODEL_PLAIN, st))) return rc;
            ObsView &v = m.obs[o];
            v.G = a.real; v.loss_part = a.loss_part; v.Fy = a.g.Fy; v.Fx = a.g.Fx; v.oy = a.g.oy; v.ox = a.g.ox;
        }
        prof_stop(st); prof_start(1, st);
        if (!approximate_L) {
            lmorph();
            m.mode = OBS_FULL;
            hipLaunchKernelGGL(contract_step, grid, block, lds, st, m);
            if (!small && (rc = obs_lipschitz_sed(state, l, ga, 0, st))) return rc;
        } else {
            m.mode = OBS_PARTIALS;
            hipLaunchKernelGGL(contract, grid, block, lds, st, m);
            lmorph();
            if (small) hipLaunchKernelGGL(k_bigk_lipschitz, dim3(ga.S), dim3(SC_BLOCK), 0, st, ga, 1);   // (trace of the pass's Gram)
            else if ((rc = obs_lipschitz_sed(state, l, ga, 1, st))) return rc;
            m.mode = OBS_STEP;
            hipLaunchKernelGGL(contract_step, grid, block, lds, st, m);
        }
        hipLaunchKernelGGL(head, dim3(m.S), dim3(SC_BLOCK), 0, st, m);
        HIP_TRY(hipGetLastError());
        prof_stop(st);
        return iteration_tail(state, l, e_rel, stream, uo);
    });
}

// The host checks of the per-scene tables of low-resolution observations, after the observations' and the frames' own;
// no device call.  Either list may be NULL: no entry
static int check_lowres_frames_call(const int32_t *frame_hw, const scarlet_lowres *const *lowres,
                                    const scarlet_lowres_frames *const *lrf, int n_obs)
{
    for (int o = 0; o < n_obs; ++o) {
        const scarlet_lowres *lr = lowres ? lowres[o] : nullptr;
        const scarlet_lowres_frames *lf = lrf ? lrf[o] : nullptr;
        if (lf && !lr) return set_err(SCARLET_E_ARG, "scarlet_lowres_frames for an observation that has no scarlet_lowres");
        if (lr && !lf && frame_hw)
            return set_err(SCARLET_E_NOTIMPL, "frame_hw (ragged frames) with a low-resolution observation that has no "
                                              "scarlet_lowres_frames: its operator would be that of the padded frame");
        if (!lf) continue;
        if (!frame_hw) return set_err(SCARLET_E_ARG, "scarlet_lowres_frames without frame_hw");
        if (!lf->dims || !lf->uy || !lf->ux) return set_err(SCARLET_E_ARG, "scarlet_lowres_frames: null table");
        if (!lr->v_per_scene || !lr->dhat_per_scene)
            return set_err(SCARLET_E_ARG, "scarlet_lowres_frames: the scarlet_lowres needs v_per_scene = dhat_per_scene = 1");
    }
    return SCARLET_OK;
}
// scarlet_fit_multi: counts are refused right after the shape checks, before any pointer of the batches is looked at
static int refuse_counts(const scarlet_batch *b)
{
    const int rc = check_shape(b);
    if (!rc && b->n_components)
        return set_err(SCARLET_E_NOTIMPL, "scarlet_fit_multi does not take n_components (ragged batches): pass NULL");
    return rc;
}
static int refuse(const char *a, const char *b)
{
    char msg[160];
    snprintf(msg, sizeof msg, "%s with %s: not implemented", a, b);
    return set_err(SCARLET_E_NOTIMPL, msg);
}
// The one host-side check of a request, in this order: the members that must be there and those that do not go
// together; the observation list; the batch (check_call); every observation against it; then the prior of a joint fit,
// the frames (FRAMES_LATE: also their presence) and the low-resolution tables.  Nothing is launched.
static int check_request(const scarlet_batch *b, const scarlet_fit_request &r, const Rules &u)
{
    const auto has = [&](unsigned f) { return (u.flags & f) != 0; };
    const char *no_frames = "frames is NULL (pass a scarlet_frames with frame_hw = NULL for uniform frames)";
    const int32_t *frame_hw = r.frames ? r.frames->frame_hw : nullptr;
    const bool multi = has(MULTI);
    int rc = SCARLET_OK;
    if (has(NO_COUNTS)) {
        rc = refuse_counts(b);
        for (int o = 0; !rc && r.obs && r.n_obs <= SCARLET_MAX_OBSERVATIONS && o < r.n_obs; ++o)
            if (r.obs[o]) rc = refuse_counts(r.obs[o]);
        if (rc) return rc;
    }
    if (has(NEED_F) && !has(FRAMES_LATE) && !r.frames) return set_err(SCARLET_E_ARG, no_frames);
    if (has(NEED_O) && !r.options) return set_err(SCARLET_E_ARG, "options is NULL (pass a scarlet_update_options with NULL members for the defaults)");
    if (r.options && b && b->group && !has(GROUP_OPTIONS))
        return set_err(SCARLET_E_NOTIMPL, "update options with group: the layers of a multi-component source are tied to soft symmetry");
    if (r.options && multi && b && b->B > SC_BMAX)
        return set_err(SCARLET_E_NOTIMPL, "update options with a wide state (more than 8 model channels): not implemented");
    if (has(NEED_LOWRES) && (!r.lowres || (has(NEED_LRF) && !r.lowres_frames)))
        return set_err(SCARLET_E_ARG, has(NEED_LRF) ? "null low-resolution list (pass arrays of n_obs pointers, NULL = same grid / no tables of its own)"
                                                    : "null low-resolution list (pass an array of n_obs pointers, NULL = same grid)");
    // (what no named entry point's signature can say)
    if (!multi && (r.lowres || r.lowres_frames)) return set_err(SCARLET_E_ARG, "lowres / lowres_frames without observations (n_obs = 0)");
    if (r.prior && frame_hw) return refuse("a prior", "frame_hw (ragged frames)");
    if (r.prior && r.options) return refuse("a prior", "update options");
    if (multi && r.options && frame_hw) return refuse("update options of a joint fit", "frame_hw (ragged frames)");
    if (multi && r.options && r.lowres) return refuse("update options of a joint fit", "lowres (a low-resolution observation)");
    if (multi && (r.n_obs < 1 || r.n_obs > SCARLET_MAX_OBSERVATIONS)) return set_err(SCARLET_E_ARG, "1 to 8 observations");
    if (multi && (!r.obs || !r.band0)) return set_err(SCARLET_E_ARG, "null observation list");
    rc = check_call(b, has(NEED_C) || r.constraints, r.constraints, has(NEED_P) && !multi, multi ? nullptr : r.prior, r.max_iter, u.bmax);
    for (int o = 0; !rc && multi && o < r.n_obs; ++o) {
        const scarlet_batch *ob = r.obs[o];
        if (!ob) return set_err(SCARLET_E_ARG, "null observation batch");
        const scarlet_lowres *lr = r.lowres ? r.lowres[o] : nullptr;
        // a low-resolution observation: its batch has the observation's own h x w and no difference kernel
        if (ob->S != b->S || ob->K != b->K || ob->H != (lr ? lr->h : b->H) || ob->W != (lr ? lr->w : b->W) || ob->B < 1 ||
            r.band0[o] < 0 || r.band0[o] + ob->B > b->B || ob->mse_capacity < 1)
            return set_err(SCARLET_E_ARG, lr ? "a low-resolution observation does not fit the model frame or its scarlet_lowres"
                                             : "an observation does not fit the model frame");
        if (lr && ob->diff_kernel)
            return set_err(SCARLET_E_ARG, "a low-resolution observation takes no diff_kernel: its PSFs are in dhat");
        if (ob->n_components)
            return set_err(SCARLET_E_ARG, "an observation batch takes no n_components: the state's counts govern every observation");
        if (lr && (rc = check_lowres(lr, b->H, b->W, ob->B, true, has(LARGE)))) return rc;
        rc = check_batch(ob);
    }
    if (!rc && multi && (has(NEED_P) || r.prior)) rc = check_prior(r.prior);
    if (!rc && has(NEED_F) && !r.frames) rc = set_err(SCARLET_E_ARG, no_frames);
    if (!rc && frame_hw && b->group && !has(GROUP_FRAMES)) rc = set_err(SCARLET_E_NOTIMPL, "frame_hw (ragged frames) with group: not implemented");
    if (!rc && multi) rc = check_lowres_frames_call(frame_hw, r.lowres, r.lowres_frames, r.n_obs);
    return rc;
}
extern "C" int scarlet_fit_request_check(const scarlet_batch *b, const scarlet_fit_request *r)
{
    if (!r) return set_err(SCARLET_E_ARG, "null request");
    return check_request(b, *r, r->n_obs == 0 ? RULES_ONE : RULES_MANY);
}

// check and body of the entry points that fit the request's observations.  The named ones below are fixed shapes of
// scarlet_fit_with: what each requires and refuses is in its Rules, what the members mean in the header.
static int fit_many(scarlet_batch *state, const scarlet_fit_request &r, const Rules &u, void *stream)
{
    const int rc = check_request(state, r, u);
    return rc ? rc : fit_observations_call(state, r, (u.flags & LARGE) != 0, stream);
}
extern "C" int scarlet_fit_with(scarlet_batch *b, const scarlet_fit_request *r, void *stream)
{
    if (!r) return set_err(SCARLET_E_ARG, "null request");
    return r->n_obs == 0 ? fit_one(b, *r, RULES_ONE, stream) : fit_many(b, *r, RULES_MANY, stream);
}
extern "C" int scarlet_fit_observations(scarlet_batch *state, scarlet_batch *const *obs, const int32_t *band0, int n_obs,
                                        int max_iter, double e_rel, int approximate_L, int check_every, void *stream)
{
    return fit_many(state, loop_request(max_iter, e_rel, approximate_L, check_every, obs, band0, n_obs), {MULTI, SC_BMAX}, stream);
}
extern "C" int scarlet_fit_multi(scarlet_batch *state, scarlet_batch *const *obs, const int32_t *band0, int n_obs,
                                 int max_iter, double e_rel, int approximate_L, int check_every, void *stream)
{
    return fit_many(state, loop_request(max_iter, e_rel, approximate_L, check_every, obs, band0, n_obs), {MULTI | NO_COUNTS, SC_BMAX}, stream);
}
extern "C" int scarlet_fit_observations_constrained(scarlet_batch *state, const scarlet_constraints *c, scarlet_batch *const *obs,
                                                    const int32_t *band0, int n_obs, int max_iter, double e_rel,
                                                    int approximate_L, int check_every, void *stream)
{
    scarlet_fit_request r = loop_request(max_iter, e_rel, approximate_L, check_every, obs, band0, n_obs);
    r.constraints = c;
    return fit_many(state, r, {MULTI | NEED_C, SC_BMAX}, stream);
}
extern "C" int scarlet_fit_observations_options(scarlet_batch *state, const scarlet_constraints *c, const scarlet_update_options *o,
                                                scarlet_batch *const *obs, const int32_t *band0, int n_obs, int max_iter,
                                                double e_rel, int approximate_L, int check_every, void *stream)
{
    scarlet_fit_request r = loop_request(max_iter, e_rel, approximate_L, check_every, obs, band0, n_obs);
    r.constraints = c; r.options = o;
    return fit_many(state, r, {MULTI | NEED_O, SC_BMAX}, stream);
}
extern "C" int scarlet_fit_observations_lowres(scarlet_batch *state, const scarlet_constraints *c, scarlet_batch *const *obs,
                                               const scarlet_lowres *const *lowres, const int32_t *band0, int n_obs,
                                               int max_iter, double e_rel, int approximate_L, int check_every, void *stream)
{
    scarlet_fit_request r = loop_request(max_iter, e_rel, approximate_L, check_every, obs, band0, n_obs);
    r.constraints = c; r.lowres = lowres;
    return fit_many(state, r, {MULTI | NEED_C | NEED_LOWRES, SC_BMAX}, stream);
}
extern "C" int scarlet_fit_observations_lowres_large(scarlet_batch *state, const scarlet_constraints *c, scarlet_batch *const *obs,
                                                     const scarlet_lowres *const *lowres, const int32_t *band0, int n_obs,
                                                     int max_iter, double e_rel, int approximate_L, int check_every, void *stream)
{
    scarlet_fit_request r = loop_request(max_iter, e_rel, approximate_L, check_every, obs, band0, n_obs);
    r.constraints = c; r.lowres = lowres;
    return fit_many(state, r, {MULTI | NEED_C | NEED_LOWRES | LARGE, SC_BMAX}, stream);
}
extern "C" int scarlet_fit_observations_prior(scarlet_batch *state, const scarlet_constraints *c, const scarlet_prior *p,
                                              scarlet_batch *const *obs, const scarlet_lowres *const *lowres,
                                              const int32_t *band0, int n_obs, int max_iter, double e_rel,
                                              int approximate_L, int check_every, void *stream)
{
    scarlet_fit_request r = loop_request(max_iter, e_rel, approximate_L, check_every, obs, band0, n_obs);
    r.constraints = c; r.prior = p; r.lowres = lowres;
    return fit_many(state, r, {MULTI | NEED_P | LARGE, SC_BMAX}, stream);
}
extern "C" int scarlet_fit_observations_wide(scarlet_batch *state, const scarlet_constraints *c, const scarlet_prior *p,
                                             scarlet_batch *const *obs, const scarlet_lowres *const *lowres,
                                             const int32_t *band0, int n_obs, int max_iter, double e_rel,
                                             int approximate_L, int check_every, void *stream)
{
    scarlet_fit_request r = loop_request(max_iter, e_rel, approximate_L, check_every, obs, band0, n_obs);
    r.constraints = c; r.prior = p; r.lowres = lowres;
    return fit_many(state, r, {MULTI | LARGE, SC_CMAX}, stream);
}
extern "C" int scarlet_fit_observations_frames(scarlet_batch *state, const scarlet_frames *f, const scarlet_constraints *c,
                                               scarlet_batch *const *obs, const int32_t *band0, int n_obs, int max_iter,
                                               double e_rel, int approximate_L, int check_every, void *stream)
{
    scarlet_fit_request r = loop_request(max_iter, e_rel, approximate_L, check_every, obs, band0, n_obs);
    r.frames = f; r.constraints = c;
    return fit_many(state, r, {MULTI | NEED_F, SC_CMAX}, stream);
}
extern "C" int scarlet_fit_observations_frames_lowres(scarlet_batch *state, const scarlet_frames *f, const scarlet_constraints *c,
                                                      scarlet_batch *const *obs, const scarlet_lowres *const *lowres,
                                                      const scarlet_lowres_frames *const *lowres_frames, const int32_t *band0,
                                                      int n_obs, int max_iter, double e_rel, int approximate_L, int check_every,
                                                      void *stream)
{
    scarlet_fit_request r = loop_request(max_iter, e_rel, approximate_L, check_every, obs, band0, n_obs);
    r.frames = f; r.constraints = c; r.lowres = lowres; r.lowres_frames = lowres_frames;
    return fit_many(state, r, {MULTI | NEED_F | NEED_LOWRES | NEED_LRF | LARGE, SC_CMAX}, stream);
}

static int init_combined_sed_call(scarlet_batch *state, const float *images, int B, int band0, const float *obs_psf_peak,
                                  int peak_per_scene, const float *model_psf_max, void *stream, int bmax)
{
    int rc = check_batch(state, bmax);
    if (rc) return rc;
    if (!images || B < 1 || B > SC_BMAX || band0 < 0 || band0 + B > state->B)
        return set_err(SCARLET_E_ARG, "an observation does not fit the model frame");
    const int n = state->S * state->K;
    hipLaunchKernelGGL(k_combined_sed, dim3((n + SC_BLOCK - 1) / SC_BLOCK), dim3(SC_BLOCK), 0, (hipStream_t)stream,
                       state->S, state->K, state->B, state->H, state->W, (const int *)state->n_components,
                       (const int *)state->status, (const int *)state->cur, (const int *)state->centers, state->sed[0],
                       state->sed[1], images, B, band0, obs_psf_peak, peak_per_scene ? B : 0, model_psf_max);
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}
extern "C" int scarlet_init_combined_sed(scarlet_batch *state, const float *images, int B, int band0,
                                         const float *obs_psf_peak, int peak_per_scene, const float *model_psf_max,
                                         void *stream)
{
    return init_combined_sed_call(state, images, B, band0, obs_psf_peak, peak_per_scene, model_psf_max, stream, SC_BMAX);
}
extern "C" int scarlet_init_combined_sed_wide(scarlet_batch *state, const float *images, int B, int band0,
                                              const float *obs_psf_peak, int peak_per_scene, const float *model_psf_max,
                                              void *stream)
{
    return init_combined_sed_call(state, images, B, band0, obs_psf_peak, peak_per_scene, model_psf_max, stream, SC_CMAX);
}

// ------------------------------------------------------------------------------------
// ExtendedSource initialisation (source.py:139-180), float64 tile like the reference's
// float64 coadd (bg_rms is float64 there), one workgroup per component.
struct InitArgs {
    int S, K, B, H, W;
    const float *images;
    float *sed[2], *morph[2];
    const int *cur;
    const int *centers;
    int *flags;
    int *status;
    const int *ncomp;                 // [S] or NULL: absent components are left as they are (zero)
    double bg_rms[SC_BMAX];
    double sed_scale[SC_BMAX];
    int has_scale;
    int do_symmetric, do_monotonic;
    double thresh;
    int no_hybrid;                    // diagnostics: SCARLET_NO_HYBRID_SWEEP
    const int *frame_hw;              // scarlet_batch::frame_hw (NULL: every scene is H x W); read by the RAGGED instantiation
};

// GT: frames whose float64 tile does not fit LDS work on a tile in a temporary HBM buffer
// RAGGED: the scene's own frame (frame_hw) bounds the coadd, the symmetry window, the sweep and the centre test; the
// rest of the H x W plane is written as zero
template <bool GT, bool RAGGED = false>
__global__ __launch_bounds__(SC_BLOCK) void k_init_extended(InitArgs a, double *gtile)
{
    extern __shared__ __align__(16) double ldsd[];
    const int c = blockIdx.x, s = c / a.K, PH = a.H, PW = a.W, PHW = PH * PW, B = a.B;
    int fh = PH, fw = PW;
    if (RAGGED && !frame_ok(a.frame_hw, s, PH, PW, fh, fw)) return;
    const int H = fh, W = fw, HW = H * W;
    TileT<double> t; t.H = H; t.W = W; t.LW = PW + 1;
    t.m = GT ? gtile + (size_t)c * PH * (PW + 1) : ldsd;
    __shared__ double red[SC_NWAVES];
    __shared__ float sed_s[SC_BMAX];
    if (c - s * a.K >= scene_ncomp(a.ncomp, s, a.K)) return;        // absent component
    const int cy = a.centers[2 * c], cx = a.centers[2 * c + 1];
    if (cy < 0 || cy >= H || cx < 0 || cx >= W) {
        // a source outside the frame (IndexError in the reference, ValueError in BlendBatch): empty component
        const int wb = a.cur[s];
        float *gm0 = a.morph[wb] + (size_t)c * PHW;
        for (int i = threadIdx.x; i < PHW; i += SC_BLOCK) gm0[i] = 0.f;
        if (threadIdx.x < B) a.sed[wb][(size_t)c * B + threadIdx.x] = 0.f;
        if (threadIdx.x == 0) {
            a.flags[c] = SCARLET_FLAG_SED_NOT_CONVERGED | SCARLET_FLAG_MORPH_NOT_CONVERGED | SCARLET_FLAG_NO_VALID_PIXELS;
            atomicOr(&a.status[s], SCARLET_STATUS_CENTER_AT_EDGE);
        }
        return;
    }
    const float *img = a.images + (size_t)s * B * PHW;
    // get_psf_sed (source.py:41-71): float32 like the reference (images.dtype)
    if (threadIdx.x < B) {
        float v = img[(size_t)threadIdx.x * PHW + cy * PW + cx];
        if (a.has_scale) v = v * (float)a.sed_scale[threadIdx.x];
        sed_s[threadIdx.x] = v;
    }
    __syncthreads();
    // detection coadd, sdss symmetry, thresh=.1 monotone sweep (initsrc.h)
    double cutoff;
    const int lstop = init_detect_tile<GT, RAGGED>(t, img, B, cy, cx, sed_s, a.bg_rms, a.thresh, a.do_symmetric,
                                                   a.do_monotonic, a.no_hybrid, cutoff, PW, PHW);
    double cnt = 0;
    for (int i = threadIdx.x; i < HW; i += SC_BLOCK)
        if (t.m[(i / W) * t.LW + (i % W)] > cutoff && sweep_level(i / W, i % W, cy, cx) <= lstop) cnt += 1;
    cnt = block_sum(cnt, red);
    // morph[~mask] = 0 happens BEFORE the centre pixel is read (source.py:174-178)
    const double centre = t.m[cy * t.LW + cx] > cutoff ? t.m[cy * t.LW + cx] : 0.0;
    const int wbuf = a.cur[s];
    float *gm = a.morph[wbuf] + (size_t)c * PHW;
    for (int i = threadIdx.x; i < HW; i += SC_BLOCK) {
        const double v = t.m[(i / W) * t.LW + (i % W)];
        gm[RAGGED ? (i / W) * PW + (i % W) : i] = (float)((v > cutoff && sweep_level(i / W, i % W, cy, cx) <= lstop) ? v / centre : 0.0);
    }
    if (RAGGED) zero_outside_frame(gm, PH, PW, H, W, threadIdx.x, SC_BLOCK);
    if (threadIdx.x < B) a.sed[wbuf][(size_t)c * B + threadIdx.x] = sed_s[threadIdx.x];
    if (threadIdx.x == 0) {
        int f = SCARLET_FLAG_SED_NOT_CONVERGED | SCARLET_FLAG_MORPH_NOT_CONVERGED;
        if (cnt == 0) f |= SCARLET_FLAG_NO_VALID_PIXELS;          // SourceInitError in the reference
        a.flags[c] = f;
    }
}

static int init_extended_call(scarlet_batch *b, const float *bg_rms_host, float thresh,
                              const float *sed_scale_host, int init_symmetric, int init_monotonic,
                              int run_update, void *stream, const int32_t *frame_hw)
{
    int rc;
    if (!bg_rms_host) return set_err(SCARLET_E_ARG, "bg_rms is required");
    InitArgs a;
    a.S = b->S; a.K = b->K; a.B = b->B; a.H = b->H; a.W = b->W;
    a.images = b->images; a.sed[0] = b->sed[0]; a.sed[1] = b->sed[1];
    a.morph[0] = b->morph[0]; a.morph[1] = b->morph[1]; a.cur = b->cur; a.centers = b->centers; a.flags = b->flags;
    a.status = b->status; a.ncomp = b->n_components; a.frame_hw = (const int *)frame_hw;
    a.has_scale = sed_scale_host != nullptr; a.thresh = thresh;
    a.do_symmetric = init_symmetric; a.do_monotonic = init_monotonic;
    a.no_hybrid = opt(OPT_NO_HYBRID_SWEEP) ? 1 : 0;
    for (int i = 0; i < SC_BMAX; ++i) {
        a.bg_rms[i] = i < b->B ? (double)bg_rms_host[i] : 1.0;
        a.sed_scale[i] = (i < b->B && sed_scale_host) ? (double)sed_scale_host[i] : 1.0;
        if (i < b->B && !(a.bg_rms[i] > 0))
            return set_err(SCARLET_E_ARG, "bg_rms must be greater than zero in all channels");
    }
    if ((rc = check_counts(b, stream)) || (rc = check_frames(b, frame_hw, stream))) return rc;
    const InitTilePlan t = init_tile_plan(b->H, b->W, (size_t)b->S * b->K);
    const bool ragged = frame_hw != nullptr;
    if (t.in_lds) {
        if ((rc = ragged ? launch_lds(k_init_extended<false, true>, dim3(b->S * b->K), dim3(SC_BLOCK), t.lds, (hipStream_t)stream, a, (double *)nullptr)
                         : launch_lds(k_init_extended<false>, dim3(b->S * b->K), dim3(SC_BLOCK), t.lds, (hipStream_t)stream, a, (double *)nullptr)))
            return rc;
    } else {
        DevBuf gtile;                                  // one-time setup: a temporary float64 tile per component
        DEV_ALLOC(gtile, t.hbm);
        if (ragged) hipLaunchKernelGGL((k_init_extended<true, true>), dim3(b->S * b->K), dim3(SC_BLOCK), 0, (hipStream_t)stream, a, gtile.as<double>());
        else
        hipLaunchKernelGGL(k_init_extended<true>, dim3(b->S * b->K), dim3(SC_BLOCK), 0, (hipStream_t)stream, a, gtile.as<double>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    }
    HIP_TRY(hipGetLastError());
    // constructor's self.update()
    return run_update ? launch_update(b, ws_layout(b, WS_PEEK), 0, stream, {nullptr, nullptr, 0, frame_hw}) : SCARLET_OK;
}
extern "C" int scarlet_init_extended(scarlet_batch *b, const float *bg_rms_host, float thresh,
                                     const float *sed_scale_host, int init_symmetric, int init_monotonic,
                                     int run_update, void *stream)
{
    const int rc = check_batch(b);
    return rc ? rc : init_extended_call(b, bg_rms_host, thresh, sed_scale_host, init_symmetric, init_monotonic, run_update, stream, nullptr);
}
extern "C" int scarlet_init_extended_frames(scarlet_batch *b, const scarlet_frames *f, const float *bg_rms_host, float thresh,
                                            const float *sed_scale_host, int init_symmetric, int init_monotonic,
                                            int run_update, void *stream)
{
    int rc = check_batch(b);
    if (!rc) rc = check_frames_call(b, f);
    return rc ? rc : init_extended_call(b, bg_rms_host, thresh, sed_scale_host, init_symmetric, init_monotonic, run_update, stream,
                                        f->frame_hw);
}

// ---- scarlet_init_sources (initsrc.h): every stock source type, per-scene noise and PSF peaks
// mixed: scarlet_init_sources_frames_mixed -- with frame_hw, `kind` and b->group are honoured on each scene's own frame
static int init_sources_call(scarlet_batch *b, const scarlet_init_spec *spec, void *stream, const int32_t *frame_hw,
                             bool mixed = false)
{
    int rc;
    if (!spec) return set_err(SCARLET_E_ARG, "null init spec");
    if (!spec->bg_rms) return set_err(SCARLET_E_ARG, "bg_rms is required");
    if (spec->model_psf && (spec->model_psf_P <= 0 || !(spec->model_psf_P & 1) || spec->model_psf_P > 2 * SCARLET_MAX_SIDE + 1))
        return set_err(SCARLET_E_ARG, "model_psf must be P x P with P odd");
    InitSrcArgs a;
    a.S = b->S; a.K = b->K; a.B = b->B; a.H = b->H; a.W = b->W;
    a.images = b->images; a.sed[0] = b->sed[0]; a.sed[1] = b->sed[1];
    a.morph[0] = b->morph[0]; a.morph[1] = b->morph[1]; a.cur = b->cur; a.centers = b->centers;
    a.flags = b->flags; a.status = b->status; a.active = b->active;
    a.ncomp_in = b->n_components; a.group = b->group; a.kind = spec->kind;
    a.bg_rms = spec->bg_rms; a.bg_stride = spec->bg_rms_per_scene ? b->B : 0;
    a.obs_peak = spec->obs_psf_peak; a.peak_stride = spec->obs_psf_peak_per_scene ? b->B : 0;
    a.model_psf = spec->model_psf; a.P = spec->model_psf ? spec->model_psf_P : 0;
    a.perc = spec->flux_percentiles; a.thresh = spec->thresh;
    a.do_symmetric = spec->init_symmetric; a.do_monotonic = spec->init_monotonic; a.group_symmetric = b->symmetric;
    a.no_hybrid = opt(OPT_NO_HYBRID_SWEEP) ? 1 : 0;
    a.frame_hw = (const int *)frame_hw;
    const bool ragged = frame_hw != nullptr;
    // ragged frames: extended sources only -- `kind` must be NULL (it lives on the device: its values cannot be looked at
    // before the launch); check_frames_call refused groups.  scarlet_init_sources_frames_mixed (`mixed`) takes both
    if (ragged && !mixed && spec->kind)
        return set_err(SCARLET_E_NOTIMPL, "frame_hw (ragged frames): scarlet_init_sources_frames starts extended sources only (kind must be NULL)");
    const InitTilePlan t = init_tile_plan(b->H, b->W, (size_t)b->S * b->K);
    if (t.in_lds && ((rc = allow_lds(k_init_extended_rows<false>, t.lds)) || (rc = allow_lds(k_init_layers<false>, t.lds)) ||
                     (ragged && (rc = allow_lds(k_init_extended_rows<false, true>, t.lds))) ||
                     (ragged && b->group && (rc = allow_lds(k_init_layers<false, true>, t.lds)))))
        return rc;
    if ((rc = check_counts(b, stream)) || (rc = check_frames(b, frame_hw, stream))) return rc;
    hipStream_t st = (hipStream_t)stream;
    // the counts this call works with: a scene with bad input keeps none (one-time set-up: a temporary buffer)
    DevBuf ncomp, gtile;
    DEV_ALLOC(ncomp, sizeof(int) * (size_t)b->S);
    a.ncomp = ncomp.as<int>();
    hipLaunchKernelGGL(k_init_check, dim3((b->S + SC_BLOCK - 1) / SC_BLOCK), dim3(SC_BLOCK), 0, st, a);
    const dim3 grid(b->S * b->K);
    if (ragged) {
        if (t.in_lds) {
            hipLaunchKernelGGL((k_init_extended_rows<false, true>), grid, dim3(SC_BLOCK), t.lds, st, a, (double *)nullptr);
            if (b->group) hipLaunchKernelGGL((k_init_layers<false, true>), grid, dim3(SC_BLOCK), t.lds, st, a, (double *)nullptr);
        } else {
            DEV_ALLOC(gtile, t.hbm);
            hipLaunchKernelGGL((k_init_extended_rows<true, true>), grid, dim3(SC_BLOCK), 0, st, a, gtile.as<double>());
            if (b->group) hipLaunchKernelGGL((k_init_layers<true, true>), grid, dim3(SC_BLOCK), 0, st, a, gtile.as<double>());
        }
        if (spec->kind) hipLaunchKernelGGL(k_init_point<true>, grid, dim3(SC_BLOCK), 0, st, a);
    } else if (t.in_lds) {
        hipLaunchKernelGGL(k_init_extended_rows<false>, grid, dim3(SC_BLOCK), t.lds, st, a, (double *)nullptr);
        if (b->group) hipLaunchKernelGGL(k_init_layers<false>, grid, dim3(SC_BLOCK), t.lds, st, a, (double *)nullptr);
    } else {
        DEV_ALLOC(gtile, t.hbm);
        hipLaunchKernelGGL(k_init_extended_rows<true>, grid, dim3(SC_BLOCK), 0, st, a, gtile.as<double>());
        if (b->group) hipLaunchKernelGGL(k_init_layers<true>, grid, dim3(SC_BLOCK), 0, st, a, gtile.as<double>());
    }
    if (!ragged) hipLaunchKernelGGL(k_init_point<false>, grid, dim3(SC_BLOCK), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (spec->run_update) {                          // the constructors' self.update(), on the scenes initialised here
        scarlet_batch c = *b;
        c.n_components = a.ncomp;
        if ((rc = launch_update(&c, ws_layout(b, WS_PEEK), 0, stream, {nullptr, nullptr, 0, frame_hw}))) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
    }
    HIP_TRY(hipStreamSynchronize(st));               // before the temporary buffers go
    return SCARLET_OK;
}

extern "C" int scarlet_init_sources(scarlet_batch *b, const scarlet_init_spec *spec, void *stream)
{
    const int rc = check_batch(b);
    return rc ? rc : init_sources_call(b, spec, stream, nullptr);
}
extern "C" int scarlet_init_sources_frames(scarlet_batch *b, const scarlet_frames *f, const scarlet_init_spec *spec, void *stream)
{
    int rc = check_batch(b);
    if (!rc) rc = check_frames_call(b, f);
    return rc ? rc : init_sources_call(b, spec, stream, f->frame_hw);
}
// ... every stock source type on each scene's own frame: spec->kind and b->group are honoured (k_init_point<RAGGED>,
// k_init_layers<GT, RAGGED>); with frame_hw = NULL it is scarlet_init_sources
extern "C" int scarlet_init_sources_frames_mixed(scarlet_batch *b, const scarlet_frames *f, const scarlet_init_spec *spec, void *stream)
{
    int rc = check_batch(b);
    if (!rc) rc = check_frames_grouped_call(f);
    return rc ? rc : init_sources_call(b, spec, stream, f->frame_hw, true);
}

// ---- convergence sums for the Python-override path (the built-in pipeline computes them itself)
__global__ __launch_bounds__(SC_BLOCK) void k_conv_sums(int K, int B, int HW, float *const sed0, float *const sed1,
                                                        float *const morph0, float *const morph1, const int *cur,
                                                        const int *active, const int *ncomp, double *conv)
{
    __shared__ double red[SC_NWAVES];
    const int c = blockIdx.x, s = c / K;
    if (!active[s]) return;
    if (c - s * K >= scene_ncomp(ncomp, s, K)) {                     // absent component: zero sums
        if (threadIdx.x == 0) { conv[4 * c] = 0; conv[4 * c + 1] = 0; conv[4 * c + 2] = 0; conv[4 * c + 3] = 0; }
        return;
    }
    const int c0 = cur[s];
    const float *mn = (c0 ? morph0 : morph1) + (size_t)c * HW, *ml = (c0 ? morph1 : morph0) + (size_t)c * HW;
    const float *sn = (c0 ? sed0 : sed1) + (size_t)c * B, *sl = (c0 ? sed1 : sed0) + (size_t)c * B;
    double d2 = 0, n2 = 0, d2s = 0, n2s = 0;
    for (int i = threadIdx.x; i < HW; i += SC_BLOCK) {
        const float v = mn[i], d = ml[i] - v;
        d2 += (double)(d * d); n2 += (double)(v * v);
    }
    for (int i = threadIdx.x; i < B; i += SC_BLOCK) {
        const float v = sn[i], d = sl[i] - v;
        d2s += (double)(d * d); n2s += (double)(v * v);
    }
    d2 = block_sum(d2, red); n2 = block_sum(n2, red); d2s = block_sum(d2s, red); n2s = block_sum(n2s, red);
    if (threadIdx.x == 0) { conv[4 * c] = d2s; conv[4 * c + 1] = n2s; conv[4 * c + 2] = d2; conv[4 * c + 3] = n2; }
}

extern "C" int scarlet_convergence_sums(scarlet_batch *b, void *stream)
{
    int rc = check_batch(b);
    if (!rc) rc = check_counts(b, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_conv_sums, dim3(b->S * b->K), dim3(SC_BLOCK), 0, (hipStream_t)stream, b->K, b->B,
                       b->H * b->W, b->sed[0], b->sed[1], b->morph[0], b->morph[1], b->cur, b->active,
                       (const int *)b->n_components, ws_at<double>(b, ws_layout(b, WS_PEEK).conv));
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}

// =====================================================================================
// 4. products of a batch's state (products.h; what runs and where the scratch's regions lie: launch_plan.h products_plan)
// =====================================================================================
static bool products_any(const scarlet_products *o)
{
    return o->model || o->rendered || o->residual || o->loss || o->flux || o->component_models;
}
// the plan of one evaluation: the factors of a state with K components seen through `ob` (its shape, data and PSF)
static ProductsPlan products_plan_of(const scarlet_batch *ob, int K, const scarlet_products *o, LayoutUse use, WsLayout *layout)
{
    ProductsWants w = {};
    w.model = o->model != nullptr;
    w.observed = o->rendered || o->residual || o->loss;
    w.loss = o->loss != nullptr;
    w.flux = o->flux != nullptr;
    WsLayout l = {};
    int psf = PRODUCTS_PSF_NONE;
    if (w.observed && has_psf(ob)) {
        l = ws_layout(ob, use);
        psf = l.psf_lds ? PRODUCTS_PSF_LDS : PRODUCTS_PSF_HIPFFT;
    }
    if (layout) *layout = l;
    return products_plan(ob->S, K, ob->B, ob->H, ob->W, psf, l.geom, l.plan, w);
}
// host-side check of one evaluation, before anything is launched; band0: first channel of the state that `ob` sees
// bmax: the limit on the STATE's channels (SC_CMAX from the wide entry points); an observation keeps SC_BMAX
static int check_products(const scarlet_batch *state, const scarlet_batch *ob, int band0, const scarlet_products *o,
                          int bmax = SC_BMAX)
{
    if (!state || !ob) return set_err(SCARLET_E_ARG, "null batch");
    if (!o) return set_err(SCARLET_E_ARG, "products: out is NULL");
    if (!products_any(o)) return set_err(SCARLET_E_ARG, "products: every output is NULL");
    int rc = check_shape(state, bmax);
    if (!rc) rc = check_shape(ob, ob == state ? bmax : SC_BMAX);
    if (rc) return rc;
    if (ob->S != state->S || ob->K != state->K || ob->H != state->H || ob->W != state->W || band0 < 0 || band0 + ob->B > state->B)
        return set_err(SCARLET_E_ARG, "products: the observation's S, K, H, W or channels do not fit the state");
    if (o->n_select < 0) return set_err(SCARLET_E_ARG, "products: n_select < 0");
    if (o->n_select > SCARLET_MAX_COMPONENTS) return set_err(SCARLET_E_ARG, "products: more than 256 selected components");
    if (o->component_models && o->n_select == 0) return set_err(SCARLET_E_ARG, "products: component_models without a selection");
    for (int i = 0; i < o->n_select; ++i) {
        const int k = o->components ? o->components[i] : i;
        if (k < 0 || k >= state->K) return set_err(SCARLET_E_ARG, "products: a selected component lies outside 0 .. K - 1");
    }
    if (!state->sed[0] || !state->sed[1] || !state->morph[0] || !state->morph[1] || !state->cur)
        return set_err(SCARLET_E_ARG, "products: null factor pointer in batch");
    if ((o->residual || o->loss) && !ob->images) return set_err(SCARLET_E_ARG, "products: residual and loss need images");
    if ((o->rendered || o->residual || o->loss) && has_psf(ob) && !ob->workspace)
        return set_err(SCARLET_E_ARG, "products: a batch with a diff_kernel needs its prepared workspace");
    return SCARLET_OK;
}
static int check_products_scratch(const ProductsPlan &p, const void *scratch, int64_t scratch_bytes)
{
    if (p.total > 0 && (!scratch || scratch_bytes < p.total))
        return set_err(SCARLET_E_ARG, "products: scratch is too small (scarlet_products_scratch_bytes)");
    return SCARLET_OK;
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
// one evaluation, checked before: every launch of it on `st`
// frame_hw: the scenes' own frames (scarlet_batch_products_frames), or NULL
static int launch_products(const scarlet_batch *state, const scarlet_batch *ob, int band0, const scarlet_products *o,
                           void *scratch, hipStream_t st, const int32_t *frame_hw = nullptr)
{
    WsLayout l;
    const ProductsPlan p = products_plan_of(ob, state->K, o, WS_FIX, &l);
    const int S = ob->S, K = state->K, B = ob->B, HW = ob->H * ob->W;
    char *sc = (char *)scratch;
    const bool psf = p.psf != PRODUCTS_PSF_NONE, observed_data = o->residual || o->loss;
    ProdArgs a = {};
    a.S = S; a.K = K; a.B = B; a.HW = HW; a.T = p.T; a.C = state->B; a.band0 = band0;
    a.model_C = B; a.model_b0 = 0;
    a.sed[0] = state->sed[0]; a.sed[1] = state->sed[1]; a.morph[0] = state->morph[0]; a.morph[1] = state->morph[1];
    a.cur = state->cur; a.ncomp = state->n_components;
    a.images = observed_data ? ob->images : nullptr; a.weights = ob->weights; a.weight_scalar = ob->weight_scalar;
    a.loss_part = (o->loss && p.psf != PRODUCTS_PSF_LDS) ? (double *)(sc + p.loss_part) : nullptr;
    a.flux_part = p.flux_in_pass ? (double *)(sc + p.flux_part) : nullptr;
    const bool vec4 = HW % 4 == 0 && aligned16(a.morph[0]) && aligned16(a.morph[1]) && aligned16(a.images) && aligned16(a.weights) &&
                      aligned16(o->model) && aligned16(o->rendered) && aligned16(o->residual) && aligned16(o->component_models) &&
                      aligned16(scratch);
    // k_products over scenes s0 .. s0 + n - 1; with a PSF it leaves only the unconvolved planes (and the plane sums)
    auto main_pass = [&](int s0, int n, float *planes, int planes_s0) {
        ProdArgs m = a;
        m.s0 = s0; m.model = planes; m.model_s0 = planes_s0;
        if (psf) m.loss_part = nullptr;
        else { m.rendered = o->rendered; m.residual = o->residual; }
        const dim3 grid(p.T, n);
        auto k = vec4 ? (p.flux_in_pass ? k_products<true, true> : k_products<true, false>)
                      : (p.flux_in_pass ? k_products<false, true> : k_products<false, false>);
        hipLaunchKernelGGL(k, grid, dim3(SC_BLOCK), 0, st, m);
    };
    int rc;
    if (B > SC_BMAX) {
        // a state of more than 8 channels (scarlet_observations_products_wide; it has no observed outputs): k_products
        // in chunks of 8 bands, the plane sums with the first; the reduction and the component models take any B
        for (int b0 = 0; p.main_pass && b0 < B; b0 += SC_BMAX) {
            ProdArgs m = a;
            m.B = std::min(SC_BMAX, B - b0); m.band0 = b0; m.model = o->model; m.model_C = B; m.model_b0 = b0;
            if (b0 > 0) m.flux_part = nullptr;
            if (!m.model && !m.flux_part) break;
            auto k = vec4 ? (m.flux_part ? k_products<true, true> : k_products<true, false>)
                          : (m.flux_part ? k_products<false, true> : k_products<false, false>);
            hipLaunchKernelGGL(k, dim3(p.T, S), dim3(SC_BLOCK), 0, st, m);
        }
    } else if (p.main_pass && !p.stage) main_pass(0, S, o->model, 0);
    if (psf) {
        ProdObsArgs r = {};
        r.B = B; r.HW = HW; r.T = p.T;
        r.images = a.images; r.weights = ob->weights; r.weight_scalar = ob->weight_scalar;
        r.rendered = o->rendered; r.residual = o->residual;
        r.frame_hw = (const int *)frame_hw;      // scenes with their own frames: nothing outside them (the RAGGED instantiations)
        const int64_t kplane = p.psf == PRODUCTS_PSF_LDS ? (int64_t)l.plan.Fy * (l.plan.M + 1) : (int64_t)l.geom.Fy * l.geom.Fxh;
        const float2 *khat = ws_at<const float2>(ob, p.psf == PRODUCTS_PSF_LDS ? l.lds_khat : l.khat);
        for (int s0 = 0; s0 < S; s0 += p.chunk) {
            const int n = std::min(p.chunk, S - s0), planes = n * B;
            if (p.stage) main_pass(s0, n, (float *)(sc + p.staged), s0);
            const float *in = p.stage ? (const float *)(sc + p.staged) : o->model + (size_t)s0 * B * HW;
            r.plane0 = s0 * B;
            if (p.psf == PRODUCTS_PSF_LDS) {
                FftPlan fp = l.plan;
                fp.tables = ws_at<const float2>(ob, l.lds_tables);
                r.loss = o->loss;
                if ((rc = r.frame_hw ? launch_lds(k_products_conv<true>, dim3(planes), dim3(SC_FFT_NT), p.conv_lds, st, r, in, fp, khat,
                                                  (int)ob->diff_kernel_per_scene)
                                     : launch_lds(k_products_conv<false>, dim3(planes), dim3(SC_FFT_NT), p.conv_lds, st, r, in, fp, khat,
                                                  (int)ob->diff_kernel_per_scene)))
                    return rc;
            } else {
                const PsfGeom &g = l.geom;
                float *real = (float *)(sc + p.real);
                FftPlans plans;
                if ((rc = get_plans(g.Fy, g.Fx, planes, &plans))) return rc;
                hipLaunchKernelGGL(k_plane_pad, dim3(grid_for((int64_t)planes * g.Fy * g.Fx)), dim3(SC_BLOCK), 0, st, in, planes,
                                   ob->H, ob->W, g.Fy, g.Fx, g.oy, g.ox, real);
                const bool per_scene = ob->diff_kernel_per_scene != 0;
                if ((rc = hipfft_convolve(plans, real, (float2 *)(sc + p.spec), khat + (per_scene ? (size_t)s0 * B * kplane : 0),
                                          per_scene ? planes : B, planes, (int)kplane, 0, 1.0f / ((float)g.Fy * (float)g.Fx), st)))
                    return rc;
                r.loss_part = a.loss_part;
                if (r.frame_hw) hipLaunchKernelGGL(k_products_finish<true>, dim3(planes, p.T), dim3(SC_BLOCK), 0, st, r, (const float *)real, g);
                else hipLaunchKernelGGL(k_products_finish<false>, dim3(planes, p.T), dim3(SC_BLOCK), 0, st, r, (const float *)real, g);
            }
        }
    }
    if (a.loss_part || a.flux_part)
        hipLaunchKernelGGL(k_products_reduce, dim3(S), dim3(SC_BLOCK), 0, st, a, a.loss_part ? o->loss : nullptr,
                           a.flux_part ? o->flux : nullptr);
    if (o->component_models) {
        ProdSelection sel;
        sel.n = o->n_select;
        for (int i = 0; i < sel.n; ++i) sel.k[i] = o->components ? o->components[i] : i;
        hipLaunchKernelGGL(vec4 ? k_products_components<true> : k_products_components<false>, dim3(p.T * sel.n, S),
                           dim3(SC_BLOCK), 0, st, a, sel, o->component_models);
    }
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}

extern "C" int64_t scarlet_products_scratch_bytes(const scarlet_batch *b, const scarlet_products *out)
{
    if (!b || !out || check_shape(b)) return 0;
    return products_plan_of(b, b->K, out, WS_PEEK, nullptr).total;
}
extern "C" int64_t scarlet_products_scratch_bytes_wide(const scarlet_batch *state, const scarlet_products *out)
{
    if (!state || !out || check_shape(state, SC_CMAX)) return 0;
    return products_plan_of(state, state->K, out, WS_PEEK, nullptr).total;
}

extern "C" int scarlet_batch_products(const scarlet_batch *b, const scarlet_products *out, void *scratch, int64_t scratch_bytes,
                                      void *stream)
{
    int rc = check_products(b, b, 0, out);
    if (!rc) rc = check_products_scratch(products_plan_of(b, b->K, out, WS_PEEK, nullptr), scratch, scratch_bytes);
    if (rc) return rc;
    (void)hipGetLastError();              // (what is reported at the end is ours: see check_batch)
    return launch_products(b, b, 0, out, scratch, (hipStream_t)stream);
}
// ... of a batch whose scenes have their own frames: rendered and residual are zero outside them (the spill of a
// difference kernel is masked in the kernels; without one they are zero there because the morphologies and the images are)
extern "C" int scarlet_batch_products_frames(const scarlet_batch *b, const scarlet_frames *f, const scarlet_products *out,
                                             void *scratch, int64_t scratch_bytes, void *stream)
{
    int rc = check_products(b, b, 0, out);
    if (!rc && !f) rc = set_err(SCARLET_E_ARG, "frames is NULL (pass a scarlet_frames with frame_hw = NULL for uniform frames)");
    if (!rc) rc = check_products_scratch(products_plan_of(b, b->K, out, WS_PEEK, nullptr), scratch, scratch_bytes);
    if (rc) return rc;
    (void)hipGetLastError();
    return launch_products(b, b, 0, out, scratch, (hipStream_t)stream, f->frame_hw);
}

// ---- rendered / residual / loss of a LOW-RESOLUTION observation (lowres.h k_lowres_products, lowres_stream.h; the form,
// the chunks and the scratch: launch_plan.h lowres_products_plan)
static LowresProductsPlan lowres_products_plan_of(const scarlet_batch *state, const scarlet_batch *ob, const scarlet_lowres *lr,
                                                  bool have_model)
{
    const LowresProductsSwitches sw = {opt(OPT_LOWRES_STREAMED) != 0, opt(OPT_LOWRES_CHUNK)};
    return lowres_products_plan(state->S, lowres_dims(state, ob, lr), have_model, sw);
}
// host-side check of one such evaluation, before anything is launched (every refusal is SCARLET_E_ARG)
static int check_lowres_products(const scarlet_batch *state, const scarlet_batch *ob, const scarlet_lowres *lr, int band0,
                                 const scarlet_products *o, int bmax = SC_BMAX)
{
    if (!state || !ob || !lr) return set_err(SCARLET_E_ARG, "null batch");
    if (!o) return set_err(SCARLET_E_ARG, "products: out is NULL");
    if (ob->B > SC_BMAX || lr->B > SC_BMAX) return set_err(SCARLET_E_ARG, "products: a low-resolution observation has at most 8 bands");
    if (state->H > SCARLET_MAX_SIDE || state->W > SCARLET_MAX_SIDE || lr->h > SCARLET_MAX_SIDE || lr->w > SCARLET_MAX_SIDE ||
        lr->nfy > SCARLET_MAX_SIDE || lr->nfx > 2 * SCARLET_MAX_SIDE)
        return set_err(SCARLET_E_ARG, "products: sides above SCARLET_MAX_SIDE are not supported");
    if (int rc = check_shape(state, bmax)) return rc;
    if (ob->S != state->S || ob->K != state->K || ob->H != lr->h || ob->W != lr->w || ob->B < 1 || band0 < 0 ||
        band0 + ob->B > state->B)
        return set_err(SCARLET_E_ARG, "products: a low-resolution observation does not fit the model frame or its scarlet_lowres");
    if (ob->diff_kernel)
        return set_err(SCARLET_E_ARG, "a low-resolution observation takes no diff_kernel: its PSFs are in dhat");
    if (int rc = check_lowres(lr, state->H, state->W, ob->B, false, true)) return rc;
    if (!state->sed[0] || !state->sed[1] || !state->morph[0] || !state->morph[1] || !state->cur)
        return set_err(SCARLET_E_ARG, "products: null factor pointer in batch");
    if ((o->residual || o->loss) && !ob->images) return set_err(SCARLET_E_ARG, "products: residual and loss need images");
    return SCARLET_OK;
}
// one evaluation, checked before.  model: the state's `model` output [S][C][H][W] that this call has written, or NULL
// lf, frame_hw: the observation's per-scene tables and the scenes' frames (scarlet_observations_products_frames_lowres), or NULL
static int launch_lowres_products(const scarlet_batch *state, const scarlet_batch *ob, const scarlet_lowres *lr, int band0,
                                  const scarlet_products *o, const float *model, void *scratch, hipStream_t st,
                                  const scarlet_lowres_frames *lf = nullptr, const int32_t *frame_hw = nullptr)
{
    const LowresDims d = lowres_dims(state, ob, lr);          // (with lf: the maxima, the shape of the padded blocks)
    const LowresProductsPlan p = lowres_products_plan_of(state, ob, lr, model != nullptr);
    LowresFactors f = lowres_factors(lr);
    if (lf) { f.uy = (const float2 *)lf->uy; f.ux = (const float2 *)lf->ux; }
    const bool mfma = !opt(OPT_NO_LOWRES_MFMA);
    const float *images = (o->residual || o->loss) ? ob->images : nullptr;
    const int K = state->K, C = state->B, HW = d.H * d.W, hw = d.h * d.w;
    int rc;
    switch (p.form) {
    case LOWRES_PRODUCTS_LDS: {
        LowresProductsFramesArgs a = {};
        a.d = d; a.f = f; a.K = K; a.C = C; a.band0 = band0;
        a.sed[0] = state->sed[0]; a.sed[1] = state->sed[1]; a.morph[0] = state->morph[0]; a.morph[1] = state->morph[1];
        a.cur = state->cur; a.ncomp = state->n_components;
        a.images = images; a.weights = ob->weights; a.weight_scalar = ob->weight_scalar;
        a.rendered = o->rendered; a.residual = o->residual; a.loss = o->loss; a.mfma = mfma;
        if (lf) {
            a.fr.dims = (const int *)lf->dims; a.fr.frame_hw = (const int *)frame_hw;
            if ((rc = launch_lds(k_lowres_products_frames, dim3(state->S), dim3(SC_BLOCK), p.lds, st, a))) return rc;
        } else if ((rc = launch_lds(k_lowres_products, dim3(state->S), dim3(SC_BLOCK), p.lds, st, (LowresProductsArgs)a))) return rc;
        break;
    }
    case LOWRES_PRODUCTS_STREAMED: {
        const LrsBuffers u = lrs_buffers(scratch, p.s, p.sized, true);
        for (int p0 = 0; p0 < p.planes; p0 += p.chunk) {
            const int n = std::min(p.chunk, p.planes - p0);
            const LrsPlanes pl = {nullptr, nullptr, nullptr, d.B, p0};           // (no `active`: every scene is evaluated)
            LrsOperand m = lrs_planes(u.m, d);
            if (p.stage_model) {
                LrsModel lm = {{state->sed[0], state->sed[1]}, {state->morph[0], state->morph[1]}, state->cur, state->n_components,
                               K, C, band0, HW, u.m, p.s.m, pl};
                const int mblocks = (HW + SC_BLOCK - 1) / SC_BLOCK;
                hipLaunchKernelGGL(k_lrs_model, dim3(mblocks < 1024 ? mblocks : 1024, n), dim3(SC_BLOCK), 0, st, lm);
            } else {
                // plane p0 + i is channel band0 + band of its scene: (band0 + p0 + i) H W floats from the start, and
                // (C - B) H W more for every scene before
                m = lrs_planes(model + (size_t)(band0 + p0) * HW, d);
                m.scene = (size_t)(C - d.B) * HW;
            }
            lrs_forward(st, mfma, d, f, u, p.s, pl, n, m, u.d, lf != nullptr);
            LrsFinish fin = {u.d, p.s.d, images, ob->weights, ob->weight_scalar, hw, o->rendered, o->residual,
                             o->loss ? u.partials : nullptr, p0};
            hipLaunchKernelGGL(k_lrs_products_finish, dim3(LRS_LOSS_BLOCKS, n), dim3(SC_BLOCK), 0, st, fin);
            if (o->loss) {
                LrsResid r = {nullptr, 0, nullptr, nullptr, 0.f, hw, u.partials, o->loss, pl};
                hipLaunchKernelGGL(k_lrs_loss, dim3((n + SC_BLOCK - 1) / SC_BLOCK), dim3(SC_BLOCK), 0, st, r, n);
            }
        }
        break;
    }
    }
    HIP_TRY(hipGetLastError());
    return SCARLET_OK;
}

extern "C" int64_t scarlet_lowres_products_scratch_bytes(const scarlet_batch *state, const scarlet_batch *obs,
                                                         const scarlet_lowres *lr, const scarlet_products *out)
{
    if (!out || !products_any(out)) return 0;
    if (int rc = check_lowres_products(state, obs, lr, 0, out)) return rc;
    return lowres_products_plan_of(state, obs, lr, false).total;
}
extern "C" int64_t scarlet_lowres_products_scratch_bytes_wide(const scarlet_batch *state, const scarlet_batch *obs,
                                                              const scarlet_lowres *lr, const scarlet_products *out)
{
    if (!out || !products_any(out)) return 0;
    if (int rc = check_lowres_products(state, obs, lr, 0, out, SC_CMAX)) return rc;
    return lowres_products_plan_of(state, obs, lr, false).total;
}

// the evaluations of scarlet_observations_products; lowres: NULL, or n_obs pointers (NULL = on the model's grid)
// frame_hw: the scenes' own frames (scarlet_observations_products_frames, _frames_lowres), or NULL
// lrf: NULL, or n_obs pointers: the per-scene tables of the low-resolution observations of such scenes (checked by the caller)
static int observations_products_call(const scarlet_batch *state, scarlet_batch *const *obs, const scarlet_lowres *const *lowres,
                                      const int32_t *band0, int n_obs, const scarlet_products *state_out,
                                      const scarlet_products *out, void *scratch, int64_t scratch_bytes, void *stream,
                                      int bmax = SC_BMAX, const int32_t *frame_hw = nullptr,
                                      const scarlet_lowres_frames *const *lrf = nullptr)
{
    if (!state) return set_err(SCARLET_E_ARG, "null batch");
    if (n_obs < 0 || n_obs > SCARLET_MAX_OBSERVATIONS || (n_obs > 0 && (!obs || !band0 || !out)))
        return set_err(SCARLET_E_ARG, "products: bad observation list");
    bool any = state_out && products_any(state_out);
    for (int i = 0; i < n_obs; ++i) any = any || products_any(&out[i]);
    if (!any) return set_err(SCARLET_E_ARG, "products: every output is NULL");
    int rc;
    if (state_out && products_any(state_out)) {
        if (state_out->rendered || state_out->residual || state_out->loss)
            return set_err(SCARLET_E_ARG, "products: rendered, residual and loss belong to an observation, not to the state");
        if ((rc = check_products(state, state, 0, state_out, bmax)) ||
            (rc = check_products_scratch(products_plan_of(state, state->K, state_out, WS_PEEK, nullptr), scratch, scratch_bytes)))
            return rc;
    }
    const float *model = state_out ? state_out->model : nullptr;
    for (int i = 0; i < n_obs; ++i) {
        if (!products_any(&out[i])) continue;
        if (out[i].model || out[i].flux || out[i].component_models || out[i].n_select)
            return set_err(SCARLET_E_ARG, "products: model, flux and component_models belong to the state, not to an observation");
        if (lowres && lowres[i]) {
            if ((rc = check_lowres_products(state, obs[i], lowres[i], band0[i], &out[i], bmax))) return rc;
            const int64_t need = lowres_products_plan_of(state, obs[i], lowres[i], model != nullptr).total;
            if (need > 0 && (!scratch || scratch_bytes < need))
                return set_err(SCARLET_E_ARG, "products: scratch is too small (scarlet_lowres_products_scratch_bytes)");
            continue;
        }
        if ((rc = check_products(state, obs[i], band0[i], &out[i], bmax)) ||
            (rc = check_products_scratch(products_plan_of(obs[i], state->K, &out[i], WS_PEEK, nullptr), scratch, scratch_bytes)))
            return rc;
    }
    (void)hipGetLastError();
    if (state_out && products_any(state_out) &&
        (rc = launch_products(state, state, 0, state_out, scratch, (hipStream_t)stream, frame_hw)))
        return rc;
    for (int i = 0; i < n_obs; ++i) {
        if (!products_any(&out[i])) continue;
        if (lowres && lowres[i])
            rc = launch_lowres_products(state, obs[i], lowres[i], band0[i], &out[i], model, scratch, (hipStream_t)stream,
                                        lrf ? lrf[i] : nullptr, frame_hw);
        else rc = launch_products(state, obs[i], band0[i], &out[i], scratch, (hipStream_t)stream, frame_hw);
        if (rc) return rc;
    }
    return SCARLET_OK;
}

extern "C" int scarlet_observations_products(const scarlet_batch *state, scarlet_batch *const *obs, const int32_t *band0, int n_obs,
                                             const scarlet_products *state_out, const scarlet_products *out, void *scratch,
                                             int64_t scratch_bytes, void *stream)
{
    return observations_products_call(state, obs, nullptr, band0, n_obs, state_out, out, scratch, scratch_bytes, stream);
}

extern "C" int scarlet_observations_products_lowres(const scarlet_batch *state, scarlet_batch *const *obs,
                                                    const scarlet_lowres *const *lowres, const int32_t *band0, int n_obs,
                                                    const scarlet_products *state_out, const scarlet_products *out,
                                                    void *scratch, int64_t scratch_bytes, void *stream)
{
    if (!lowres) return set_err(SCARLET_E_ARG, "null low-resolution list (pass an array of n_obs pointers, NULL = same grid)");
    return observations_products_call(state, obs, lowres, band0, n_obs, state_out, out, scratch, scratch_bytes, stream);
}

// scarlet_observations_products_lowres for a state of up to SCARLET_MAX_CHANNELS channels; `lowres` may be NULL
extern "C" int scarlet_observations_products_wide(const scarlet_batch *state, scarlet_batch *const *obs,
                                                  const scarlet_lowres *const *lowres, const int32_t *band0, int n_obs,
                                                  const scarlet_products *state_out, const scarlet_products *out,
                                                  void *scratch, int64_t scratch_bytes, void *stream)
{
    return observations_products_call(state, obs, lowres, band0, n_obs, state_out, out, scratch, scratch_bytes, stream, SC_CMAX);
}

// scarlet_observations_products / _wide (the state's channel count decides) of scenes with their own frames: rendered
// and residual are zero outside them, as scarlet_batch_products_frames leaves them
extern "C" int scarlet_observations_products_frames(const scarlet_batch *state, const scarlet_frames *f, scarlet_batch *const *obs,
                                                    const int32_t *band0, int n_obs, const scarlet_products *state_out,
                                                    const scarlet_products *out, void *scratch, int64_t scratch_bytes,
                                                    void *stream)
{
    if (!f) return set_err(SCARLET_E_ARG, "frames is NULL (pass a scarlet_frames with frame_hw = NULL for uniform frames)");
    if (!state) return set_err(SCARLET_E_ARG, "null batch");
    if (int rc = check_frames_call(state, f)) return rc;
    return observations_products_call(state, obs, nullptr, band0, n_obs, state_out, out, scratch, scratch_bytes, stream,
                                      state->B > SC_BMAX ? SC_CMAX : SC_BMAX, f->frame_hw);
}

// scarlet_observations_products_lowres / _wide (the state's channel count decides) of scenes with their own frames whose
// low-resolution observations bring their own operators: their rendered and residual are zero outside each scene's own
// h_s x w_s pixels, the loss runs over those
extern "C" int scarlet_observations_products_frames_lowres(const scarlet_batch *state, const scarlet_frames *f,
                                                           scarlet_batch *const *obs, const scarlet_lowres *const *lowres,
                                                           const scarlet_lowres_frames *const *lowres_frames,
                                                           const int32_t *band0, int n_obs, const scarlet_products *state_out,
                                                           const scarlet_products *out, void *scratch, int64_t scratch_bytes,
                                                           void *stream)
{
    if (!f) return set_err(SCARLET_E_ARG, "frames is NULL (pass a scarlet_frames with frame_hw = NULL for uniform frames)");
    if (!state) return set_err(SCARLET_E_ARG, "null batch");
    if (!lowres || !lowres_frames)
        return set_err(SCARLET_E_ARG, "null low-resolution list (pass arrays of n_obs pointers, NULL = same grid / no tables of its own)");
    if (n_obs < 0 || n_obs > SCARLET_MAX_OBSERVATIONS) return set_err(SCARLET_E_ARG, "products: bad observation list");
    if (int rc = check_frames_call(state, f)) return rc;
    if (int rc = check_lowres_frames_call(f->frame_hw, lowres, lowres_frames, n_obs)) return rc;
    return observations_products_call(state, obs, lowres, band0, n_obs, state_out, out, scratch, scratch_bytes, stream,
                                      state->B > SC_BMAX ? SC_CMAX : SC_BMAX, f->frame_hw, lowres_frames);
}

// diagnostics: contract_plan (launch_plan.h) of a joint fit with K components over C model channels:
// {kernel (ContractKernel), channel width, waves, threads, dynamic LDS bytes, LDS limit, prior, 0}
extern "C" int scarlet_debug_contract_plan(int K, int C, int prior, int32_t *out8)
{
    if (!out8) return -1;
    const ContractPlan p = contract_plan(K, C, prior != 0);
    const int v[8] = {p.kernel, p.cw, p.nw, p.block, (int)p.lds, (int)LDS_LIMIT, p.prior ? 1 : 0, 0};
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    return p.kernel == CONTRACT_NONE ? -1 : 0;
}

// diagnostics: fused_plan (launch_plan.h) of a fit of batch b -- with the frames and constraints scarlet_fit_frames /
// scarlet_fit_constrained would get -- under the options in force: {kernel (FusedKernel), threads, dynamic LDS bytes,
// fits, LDS limit, ragged, 0, 0}.  Reads the structs' host fields only; no device pointer is dereferenced.
extern "C" int scarlet_debug_fused_plan(const scarlet_batch *b, const scarlet_frames *f, const scarlet_constraints *c,
                                        int approximate_L, int n_iter, int32_t *out8)
{
    if (!b || !out8) return -1;
    const bool ragged = f && f->frame_hw;
    const FusedPlan p = fused_plan(b, approximate_L, cons_any(c), n_iter, fused_switches(), ragged);
    const int v[8] = {p.kernel, p.block, (int)p.lds, p.fits ? 1 : 0, (int)LDS_LIMIT, ragged ? 1 : 0, 0, 0};
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    return 0;
}
