// launch_plan.h -- which form of a kernel a shape takes and the dynamic LDS that form asks for, decided once.
// Host code: pure functions of the shapes and the diagnostic switches (UpdateWants, FusedSwitches), no device call.
// The sizes come from the functions that stand beside the kernels (prox_ops.h, wave_ops.h, boxupdate.h, fused.h,
// fused2.h, initsrc.h); the launch sites of scarlet_hip.hip switch on the plan and compute nothing of their own.
// tools/native/launch_forms.hip prints the shapes at which the forms begin (the table of DESIGN.md "One plan").
#pragma once
#include "boxupdate.h"
#include "fused2.h"
#include "initsrc.h"
#include "lowres_stream.h"
#include "products.h"
#include "multiobs_wide.h"
#include <algorithm>

static const size_t LDS_LIMIT = 160 * 1024 - 1024;   // leave room for static __shared__

// ---- the constraint update (launch_update), the stand-alone operators (launch_operator), the layout (ws_layout)
// FORM_WAVE: one wave per component, its tile in LDS (sides up to 64).  FORM_TILE: one workgroup per component, tile
// and GEMM scratch in LDS.  FORM_TILE_GSCRATCH: the tile in LDS, the scratch in HBM.  FORM_PLANE: both in HBM.
enum UpdateForm { FORM_WAVE, FORM_TILE, FORM_TILE_GSCRATCH, FORM_PLANE };
// k_source_update_box<NB, XS> and its _listed twin; BOX_STREAMED = <0, 0>, frames with a side over 256
enum BoxInstance { BOX_NONE, BOX_STREAMED, BOX_8_128, BOX_16_256, BOX_8, BOX_16 };
struct UpdateWants {
    bool wave;              // the wave form is allowed (an operator without one, FORCE_BLOCK_UPDATE: false)
    bool gscratch;          // a workspace with `gscratch` stands behind the launch (the operators have none)
    bool box, box2, exact;  // the box stage (monotonic batches with uniform frames), its second box, the exact-shape instances
};
struct UpdatePlan {
    int form;
    size_t lds;             // that form's dynamic LDS
    bool reserve_gscratch;  // the workspace holds the scratch in HBM (a function of the shape alone: ws_layout)
    int box;                // BOX_NONE: no box stage
    bool box2;              // the 127 x 127 box runs for what the 63 x 63 box listed
    size_t box_lds[2];
};
inline UpdatePlan update_plan(int H, int W, const UpdateWants &w)
{
    UpdatePlan p = {};
    const bool beyond_wave = H > 64 || W > 64;
    // (frames up to 80 KB of LDS run two workgroups per CU without the scratch)
    p.reserve_gscratch = beyond_wave && update_lds_bytes(H, W) > 80 * 1024;
    if (!beyond_wave && w.wave) { p.form = FORM_WAVE; p.lds = wave_tile_lds_bytes(H, W); }
    else if (update_lds_bytes(H, W) > LDS_LIMIT) { p.form = FORM_PLANE; p.lds = plane_lds_bytes(H, W); }
    else if (w.gscratch && p.reserve_gscratch && tile_stage_lds_bytes(H, W) <= 78 * 1024) {
        p.form = FORM_TILE_GSCRATCH; p.lds = tile_stage_lds_bytes(H, W);     // two workgroups per CU instead of one
    } else { p.form = FORM_TILE; p.lds = update_lds_bytes(H, W); }
    // the pipeline on the box around each peak (boxupdate.h): 63 x 63 for every component, 127 x 127 for those whose
    // footprint left it; frames with a side over 256 take the streamed instance
    const bool streamed = H > 256 || W > 256;
    for (int i = 0; i < 2; ++i)
        p.box_lds[i] = sizeof(float) * (streamed ? ub_lds_floats_streamed(H, W, i ? 63 : 31) : ub_lds_floats(H, W, i ? 63 : 31));
    if (beyond_wave && w.box && p.box_lds[1] <= LDS_LIMIT) {
        // instances: bands of X per frame height (8: up to 128 rows, 16: up to 256), and the two BASELINE frame
        // shapes (128 x 128, 256 x 256) as compile-time constants
        p.box = streamed ? BOX_STREAMED : (w.exact && H == 128 && W == 128) ? BOX_8_128 : (w.exact && H == 256 && W == 256) ? BOX_16_256
                : (H <= 128 && W <= 128) ? BOX_8 : BOX_16;
        p.box2 = w.box2;
    }
    return p;
}

// ---- the fused one-kernel iteration (launch_fused); FUSED_NONE: the batch takes the general path
struct FusedSwitches {      // (scarlet_hip.hip fused_switches() reads them from the options)
    bool no_exact, fused_v1, no_fused, no_persist;
    int persist_dbg;
    size_t pad_lds;
};
enum FusedKernel { FUSED_NONE, FUSED_PC_B6, FUSED_PC_B8,        // k_iterate<4, 6 / SC_BMAX, FusedArgsPC>
                   FUSED_FIT2X, FUSED_ITERATE2_EXACT, FUSED_ITERATE2, // k_fit2x, k_iterate2<4, 5, 64>, k_iterate2<4, 5>
                   FUSED_B6, FUSED_B8,                          // k_iterate<4, 6 / SC_BMAX>
                   FUSED_FRAMES_B6, FUSED_FRAMES_B8 };          // k_iterate<4, 6 / SC_BMAX, FusedArgsFrames>
struct FusedPlan {
    int kernel, block;
    size_t lds;             // what the launch asks for, PAD_LDS included
    bool fits;              // ... is within LDS_LIMIT
};
// per_component: the components carry their own switches (scarlet_constraints); n_iter: the iterations wanted of
// one launch (only k_fit2x covers more than one)
// ragged_frames: the scenes have their own frames (scarlet_frames::frame_hw).  The four-wave kernel's frames instance
// takes them for every B, under its own conditions read off the padded frame (it reads the per-component switches where
// there are any); no eight-wave kernel does.  Every other ragged-frame batch takes the general path.
inline FusedPlan fused_plan(const scarlet_batch *b, int approximate_L, bool per_component, int n_iter, const FusedSwitches &sw,
                            bool ragged_frames = false)
{
    FusedPlan p = {FUSED_NONE, SC_BLOCK, 0, true};
    // K > 4: eight tiles leave one workgroup per CU and the general path is faster (measured at K = 6, 8:
    // 2.44 vs 2.58 ms and 3.25 vs 3.90 ms per iteration of 4000 scenes)
    if (approximate_L || b->diff_kernel || b->K > 4 || b->group || sw.no_fused) return p;
    if (b->H > 64 || b->W > 64 || (b->W & 3) || b->H < 3 || b->W < 3) return p;
    // admission by the four-wave kernel's size; the eight-wave kernel's K <= 4 sets of vectors ask for at most 1 KB
    // more and its exact shape for 76 KB, so without PAD_LDS every admitted launch fits
    if (fused_lds_bytes(b->K, b->H, b->W) > LDS_LIMIT - 4096) return p;
    // the headline shape (BASELINE configs[1]/[3]: 4 sources, 5 bands, 64 x 64, default pipeline) has an instance
    // with every shape and switch folded at compile time
    const bool exact64 = b->K == 4 && b->B == 5 && b->H == 64 && b->W == 64 && !b->weights && b->weight_scalar == 1.0f && b->symmetric &&
                         b->monotonic && b->l0_thresh < 0.f && b->l1_thresh < 0.f && !sw.no_exact;
    if (ragged_frames) {
        p.kernel = b->B <= 6 ? FUSED_FRAMES_B6 : FUSED_FRAMES_B8; p.lds = fused_lds_bytes(b->K, b->H, b->W);
    } else if (per_component) {
        // the four-wave kernel's per-component instance for every B (wave k reads component k's four settings in
        // phase 2), never k_iterate2 / k_fit2x
        p.kernel = b->B <= 6 ? FUSED_PC_B6 : FUSED_PC_B8; p.lds = fused_lds_bytes(b->K, b->H, b->W);
    } else if (b->B <= 5 && !sw.fused_v1) {
        // K <= 4, B <= 5: eight waves per scene, a pair of waves per component (fused2.h; its 128-VGPR budget does
        // not hold a sixth band's accumulators); persistent where more than one iteration is wanted
        const bool persist = (n_iter > 1 || (sw.persist_dbg & 2)) && !sw.no_persist;
        p.kernel = !exact64 ? FUSED_ITERATE2 : persist ? FUSED_FIT2X : FUSED_ITERATE2_EXACT;
        p.block = SC_FB2;
        p.lds = exact64 ? fused2_exact_lds_bytes(4, 64) : fused2_lds_bytes(b->K, b->H, b->W);
    } else {
        p.kernel = b->B <= 6 ? FUSED_B6 : FUSED_B8; p.lds = fused_lds_bytes(b->K, b->H, b->W);
    }
    p.lds += sw.pad_lds;    // experiment knob: SCARLET_PAD_LDS=<bytes> lowers the number of co-resident workgroups
    p.fits = p.lds <= LDS_LIMIT;
    return p;
}

// ---- the contraction over the observations of a joint fit (fit_observations_call).  Up to 8 model channels: the
// kernels of multiobs.h, register-tiled for K <= 8.  Above: k_obs_contract_wide<CW, NW> (multiobs_wide.h) for the
// channel width that holds C, with the most waves whose float64 slots fit LDS.  CONTRACT_NONE: no form (C > 32).
enum ContractKernel { CONTRACT_NONE, CONTRACT_K8, CONTRACT_ANYK, CONTRACT_WIDE };
struct ContractPlan {
    int kernel;
    int cw, nw;             // CONTRACT_WIDE: channels the instance is built for (16, 32) and its waves (4, 2, 1)
    int block;              // threads per workgroup
    bool prior;             // the passes that write a step are the PRIOR instances
    size_t lds;
};
inline ContractPlan contract_plan(int K, int C, bool prior)
{
    ContractPlan p = {CONTRACT_NONE, 0, 0, SC_BLOCK, prior, 0};
    if (K < 1 || K > SCARLET_MAX_COMPONENTS || C < 1 || C > SC_CMAX) return p;
    if (C <= SC_BMAX) {
        p.kernel = K <= SC_KMAX ? CONTRACT_K8 : CONTRACT_ANYK;
        p.nw = SC_NWAVES;
        p.lds = obs_contract_lds(K);
        return p;
    }
    p.kernel = CONTRACT_WIDE;
    p.cw = C <= 16 ? 16 : 32;
    for (p.nw = SC_NWAVES; p.nw > 1 && obs_contract_wide_lds(K, C, p.cw, p.nw) > LDS_LIMIT; p.nw /= 2) {}
    p.block = p.nw * SC_WAVE;
    p.lds = obs_contract_wide_lds(K, C, p.cw, p.nw);
    return p;
}

// ---- the read-only products of a batch's state (products.h, launch_products): which kernels run, the LDS of the
// rendering one, and where each region of the caller's scratch lies.  Without a difference kernel k_products writes every
// output itself.  With one it writes the unconvolved planes -- into the caller's `model` output when there is one,
// otherwise into scratch, the scenes taken in chunks that keep the staged planes (and the hipFFT chain's buffers)
// within LRS_SCRATCH_CAP, at least one scene -- and the LDS-resident transform or the hipFFT chain renders them.
enum ProductsPsf { PRODUCTS_PSF_NONE, PRODUCTS_PSF_LDS, PRODUCTS_PSF_HIPFFT };
struct ProductsWants {
    bool model;             // the unconvolved planes are an output
    bool observed;          // rendered, residual or loss: what an observation sees
    bool loss, flux;
};
struct ProductsPlan {
    int T;                  // tiles of PR_TILE_PIX pixels per scene
    int psf;                // ProductsPsf: what renders the observed outputs
    bool main_pass;         // k_products runs
    bool flux_in_pass;      // ... and leaves the plane sums [S][T][K]
    bool stage;             // the unconvolved planes go to scratch
    int chunk;              // scenes per chunk of the rendering stage (S without one)
    size_t conv_lds;        // dynamic LDS of k_products_conv
    int64_t loss_part, flux_part, staged, real, spec, total;   // byte offsets into the scratch, and its size
};
// geom: the hipFFT chain's shape (PRODUCTS_PSF_HIPFFT); fft: the LDS-resident plan (PRODUCTS_PSF_LDS)
inline ProductsPlan products_plan(int S, int K, int B, int H, int W, int psf, const PsfGeom &geom, const FftPlan &fft,
                                  const ProductsWants &w)
{
    ProductsPlan p = {};
    const int64_t HW = (int64_t)H * W;
    p.T = (int)((HW + PR_TILE_PIX - 1) / PR_TILE_PIX);
    p.psf = w.observed ? psf : PRODUCTS_PSF_NONE;
    p.flux_in_pass = w.flux;
    p.main_pass = w.model || w.observed || p.flux_in_pass;
    p.stage = p.psf != PRODUCTS_PSF_NONE && !w.model;
    p.conv_lds = p.psf == PRODUCTS_PSF_LDS ? fft_lds_bytes(fft.Fy, fft.M, fft.RS) : 0;
    int64_t at = 0;
    auto place = [&at](int64_t bytes) { const int64_t o = at; at += (bytes + 255) & ~(int64_t)255; return o; };
    // the loss leaves k_products and k_products_finish as tile partials; k_products_conv owns whole planes
    p.loss_part = place(w.loss && p.psf != PRODUCTS_PSF_LDS ? (int64_t)sizeof(double) * S * p.T * B : 0);
    p.flux_part = place(p.flux_in_pass ? (int64_t)sizeof(double) * S * p.T * K : 0);
    const bool fft_chain = p.psf == PRODUCTS_PSF_HIPFFT;
    const int64_t per_scene = B * ((p.stage ? HW * (int64_t)sizeof(float) : 0) +
                                   (fft_chain ? (int64_t)geom.Fy * geom.Fx * (int64_t)sizeof(float) +
                                                (int64_t)geom.Fy * geom.Fxh * (int64_t)sizeof(float2) + 512 : 0));
    p.chunk = S;
    if (per_scene > 0 && per_scene * S > (int64_t)LRS_SCRATCH_CAP) p.chunk = (int)std::max<int64_t>(1, (int64_t)LRS_SCRATCH_CAP / per_scene);
    p.staged = place(p.stage ? (int64_t)sizeof(float) * p.chunk * B * HW : 0);
    p.real = place(fft_chain ? (int64_t)sizeof(float) * p.chunk * B * geom.Fy * geom.Fx : 0);
    p.spec = place(fft_chain ? (int64_t)sizeof(float2) * p.chunk * B * geom.Fy * geom.Fxh : 0);
    p.total = at;
    return p;
}

// ---- the gradient planes of a LOW-RESOLUTION observation in a fit of the *_large kind (fit_observations_call):
// k_lowres_planes, one workgroup per scene with the factor matrices in LDS, wherever they fit; beyond, and everywhere
// under LOWRES_STREAMED, the streamed chain of lowres_stream.h.  For scenes with their own frames
// (scarlet_lowres_frames, k_lowres_planes_frames) `d` holds the per-dimension MAXIMA over the scenes -- the shape of the
// padded blocks -- and never one scene's row of `dims`: the largest h, w and the largest H, W may belong to different
// scenes, and every workgroup lays its LDS out the same way.  lowres_products_plan below takes the same `d`.
enum LowresPlanesForm { LOWRES_PLANES_LDS, LOWRES_PLANES_STREAMED };
struct LowresPlanesPlan {
    int form;
    size_t lds;             // dynamic LDS of k_lowres_planes / k_lowres_planes_frames (0 streamed)
};
inline LowresPlanesPlan lowres_planes_plan(const LowresDims &d, bool streamed)
{
    LowresPlanesPlan p = {LOWRES_PLANES_LDS, lowres_lds_bytes(d)};
    if (streamed || p.lds > LDS_LIMIT) { p.form = LOWRES_PLANES_STREAMED; p.lds = 0; }
    return p;
}

// ---- the read-only products of a LOW-RESOLUTION observation (launch_lowres_products): k_lowres_products, one workgroup
// per scene with the factor matrices in LDS, wherever they fit; beyond, and everywhere under LOWRES_STREAMED, the
// streamed chain of lowres_stream.h on the S B band planes, taken in chunks that keep the caller's scratch within
// LRS_SCRATCH_CAP (one plane at the least; LOWRES_CHUNK lowers the chunk of the launches, never the size).
enum LowresProductsForm { LOWRES_PRODUCTS_LDS, LOWRES_PRODUCTS_STREAMED };
struct LowresProductsSwitches {     // (scarlet_hip.hip reads them from the options)
    bool streamed;          // LOWRES_STREAMED
    int chunk;              // LOWRES_CHUNK: planes per chunk, 0 = automatic
};
struct LowresProductsPlan {
    int form;
    size_t lds;             // dynamic LDS of k_lowres_products
    int planes;             // S B
    int sized, chunk;       // planes per chunk that the scratch holds / that a launch takes
    bool stage_model;       // k_lrs_model writes the band models into the scratch (false: the caller's `model` output has them)
    LrsScratch s;           // the chunk's buffers (lrs_buffers)
    int64_t total;          // bytes of the caller's scratch
};
// have_model: the same call writes the state's `model` output before this evaluation runs
inline LowresProductsPlan lowres_products_plan(int S, const LowresDims &d, bool have_model, const LowresProductsSwitches &sw)
{
    LowresProductsPlan p = {};
    p.planes = S * d.B;
    p.lds = lowres_lds_bytes(d);
    if (!sw.streamed && p.lds <= LDS_LIMIT) { p.form = LOWRES_PRODUCTS_LDS; return p; }
    p.form = LOWRES_PRODUCTS_STREAMED;
    p.lds = 0;
    p.s = lrs_products_scratch(d);
    p.sized = std::min(lrs_chunk(p.s, p.planes), 65535);           // (the planes of a chunk are the grid's y)
    p.chunk = sw.chunk > 0 && sw.chunk < p.sized ? sw.chunk : p.sized;
    p.stage_model = !have_model;
    p.total = (int64_t)p.sized * (int64_t)p.s.per_plane;
    return p;
}

// ---- the initialisers' float64 tile (initsrc.h): in LDS, or one per component in a temporary HBM buffer
struct InitTilePlan { bool in_lds; size_t lds, hbm; };
inline InitTilePlan init_tile_plan(int H, int W, size_t components)
{
    const size_t tile = init_tile_bytes(H, W);
    const bool in_lds = tile <= LDS_LIMIT;
    return {in_lds, in_lds ? tile : 0, in_lds ? 0 : tile * components};
}
