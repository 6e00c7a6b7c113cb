"""Shared machinery of the long-run / converged-regime parity tests (tests/test_gpu_parity_long.py: the headline
shape; tests/test_gpu_parity_configs.py: BASELINE configs 3 and 5): GPU engine vs the CPU oracle started from the
device's own initial state, tolerance north_star's 1e-5 max-norm relative for sed / morph / loss history; centres,
iteration counts and flags bit-exact.

The algorithm tests pixel values against the threshold 0 in two places: the k-space symmetry zeroes its output
wherever its INPUT, the stepped morphology, is <= 0 (`result[X <= 0] = 0`, operator.py:285-287) -- a jump: just
above 0 the output is the average with the mirrored pixel -- and prox_plus (update.py:27-32).  A pixel whose value
sits on the threshold to within float32 rounding can land on either side; after it switches on it differs for a few
iterations before the two runs meet again.  Such a scene is NOT waived in prose: `straddles_threshold` re-runs it
iteration by iteration on the GPU, in the float32 oracle and in the float64 oracle and accepts it only if,
mechanically,
  (i)   GPU and float32 oracle agree within 1e-5 on every array at every iteration before t0,
  (ii)  at t0 they disagree about the SUPPORT of the morphology in some pixel p (one is exactly 0), and
  (iii) the float64 trajectory's value at p at one of the two threshold tests of iteration t0 (the stepped value
        entering the symmetry mask, or the value entering prox_plus) lies within 1e-5 x max|morph| of 0 -- i.e. the
        exact trajectory itself is undecided at the tolerance, so both outcomes are admissible float32 evaluations
        of the reference.
The number of scenes a run may pass this way is a FIXED count per test (not a fraction of the batch), and every use
is printed and appended to the file named by SCARLET_LOG_REL_ERR.
"""
import os

import numpy as np

from conftest import rel_err

TOL = 1e-5


class Workload(object):
    """shape + PSF + pipeline switches of one BASELINE configuration"""

    def __init__(self, B=5, H=64, W=64, K=4, psf=False, l0=None, min_sep=4):
        self.B, self.H, self.W, self.K, self.psf, self.l0, self.min_sep = B, H, W, K, psf, l0, min_sep
        self.obs_psfs = self.model_psf = self.diff = self.scale = None
        if psf:
            from oracle import pgm
            from scarlet_amd import synth
            self.obs_psfs = np.array([synth.gaussian_psf((41, 41), 1.2 + 0.15 * b) for b in range(B)])
            self.model_psf = synth.gaussian_psf((41, 41), 0.9)
            self.diff = pgm.match_psfs(self.obs_psfs.astype(np.float32), self.model_psf[None].astype(np.float32))
            self.scale = (self.model_psf.max() / self.obs_psfs.max(axis=(1, 2))).astype(np.float32)

    def scenes(self, first, n):
        from scarlet_amd import synth
        kw = dict(B=self.B, H=self.H, W=self.W, K=self.K, min_sep=self.min_sep)
        if self.psf:
            kw["psfs"] = self.obs_psfs
        sc = [synth.make_scene(first + i, **kw) for i in range(n)]
        return np.stack([s["images"] for s in sc]), np.stack([s["centers"] for s in sc])

    def batch(self, scarlet, images, centers, mse_capacity):
        kw = dict(mse_capacity=mse_capacity, l0_thresh=self.l0)
        if self.psf:
            kw["centroid_weight"] = self.model_psf.astype(np.float32)
        b = scarlet.BlendBatch(images, centers, **kw)
        if self.psf:
            b.set_diff_kernel(self.diff)
        b.init_extended(np.ones(self.B) * 0.1, sed_scale=self.scale)
        return b

    def oracle_kwargs(self):
        kw = dict(l0_thresh=self.l0)
        if self.psf:
            kw.update(diff_kernel=self.diff, centroid_weight=self.model_psf.astype(np.float32))
        return kw


def oracle_fit(args):
    """worker (spawned, never touches the GPU): oracle fit from a given state"""
    from oracle import pgm
    images, sed0, morph0, cen0, sh0, iters, e_rel, dt, okw = args
    okw = dict(okw)
    approx = okw.pop("approximate_L", False)
    if okw.get("diff_kernel") is not None:
        okw["diff_kernel"] = okw["diff_kernel"].astype(dt)
    sc = pgm.scene_from_state(images.astype(dt), sed0.astype(dt), morph0.astype(dt), cen0, sh0, **okw)
    pgm.fit(sc, iters, e_rel=e_rel, approximate_L=approx)
    return (np.array([s.sed for s in sc.sources]), np.array([s.morph for s in sc.sources]), np.array(sc.mse),
            np.array([s.center for s in sc.sources]), len(sc.mse), [int(s.flags) for s in sc.sources])


def oracle_trace(images, sed0, morph0, cen0, sh0, iters, dt, okw):
    """per-iteration (morph after the iteration, morph as prox_plus saw it) of one scene"""
    from oracle import pgm
    okw = dict(okw)
    approx = okw.pop("approximate_L", False)
    if okw.get("diff_kernel") is not None:
        okw["diff_kernel"] = okw["diff_kernel"].astype(dt)
    sc = pgm.scene_from_state(images.astype(dt), sed0.astype(dt), morph0.astype(dt), cen0, sh0, **okw)
    for s in sc.sources:
        s.trace = dict(step=[], pre_plus=[])
    post = []
    pgm.fit(sc, iters, e_rel=0, approximate_L=approx, callback=lambda scn: post.append(np.array([s.morph.copy() for s in scn.sources])))
    pre = [(np.array([s.trace["step"][t] for s in sc.sources]), np.array([s.trace["pre_plus"][t] for s in sc.sources]))
           for t in range(iters)]
    return post, pre


def gpu_fit(scarlet, wl, images, centers, iters, e_rel, per_iteration=False, check_every=10):
    import torch
    b = wl.batch(scarlet, images, centers, iters + 1)
    st0 = [t.cpu().numpy() for t in (b.sed_current, b.morph_current, b.centers, b.shifts)]
    snaps = []
    approx = bool(wl.oracle_kwargs().get("approximate_L"))       # (a workload may ask for the approximate constants)
    if per_iteration:
        for _ in range(iters):
            b.fit(1, e_rel=e_rel, approximate_L=approx)
            snaps.append(b.morph_current.cpu().numpy().copy())
    else:
        b.fit(iters, e_rel=e_rel, approximate_L=approx, check_every=check_every)
    torch.cuda.synchronize()
    out = dict(sed=b.sed_current.cpu().numpy(), morph=b.morph_current.cpu().numpy(), cen=b.centers.cpu().numpy(),
               it=b.it.cpu().numpy(), flags=b.flags.cpu().numpy(), mse=b.mse_buf.cpu().numpy(), snaps=snaps,
               status=b.status.cpu().numpy())
    return st0, out


def straddle_verdict(snaps, o32, o64, pre64, iters):
    """conditions (i) - (iii) of the module docstring for ONE scene: snaps[t], o32[t], o64[t] its morphologies after
    iteration t + 1 on the GPU (re-run alone, iteration by iteration) and in the two oracles, pre64[t] the float64
    oracle's (stepped morphologies, morphologies as prox_plus saw them); returns (ok, message)"""
    for t in range(iters):
        gm = snaps[t]
        mismatch = (gm == 0) != (o32[t] == 0)
        close = rel_err(gm, o32[t]) <= TOL
        if mismatch.any():
            scale = np.abs(o64[t]).max()
            near = np.minimum(np.abs(pre64[t][0][mismatch]), np.abs(pre64[t][1][mismatch]))
            on_threshold = near <= TOL * scale
            if on_threshold.any():
                k, y, x = (int(v[np.argmax(on_threshold)]) for v in np.nonzero(mismatch))
                return True, ("iteration %d, component %d pixel (%d, %d): float64 values at the threshold tests: stepped "
                              "%.3e, before prox_plus %.3e (tolerance 1e-5 x %.3g); gpu %.3e, float32 oracle %.3e" % (
                                  t + 1, k, y, x, pre64[t][0][k, y, x], pre64[t][1][k, y, x], scale, gm[k, y, x],
                                  o32[t][k, y, x]))
        if not close:
            return False, "iteration %d: gpu and float32 oracle differ by %.2e with no pixel on a threshold" % (
                t + 1, rel_err(gm, o32[t]))
    return False, "no divergence found when re-running the scene alone"


def straddles_threshold(scarlet, wl, images, centers, iters):
    """the f64-anchored exemption of the module docstring for ONE scene; returns (ok, message)"""
    st0, g = gpu_fit(scarlet, wl, images[None], centers[None], iters, 0.0, per_iteration=True)
    sed0, morph0, cen0, sh0 = (a[0] for a in st0)
    okw = wl.oracle_kwargs()
    o32, _ = oracle_trace(images, sed0, morph0, cen0, sh0, iters, np.float32, okw)
    o64, pre64 = oracle_trace(images, sed0, morph0, cen0, sh0, iters, np.float64, okw)
    return straddle_verdict([m[0] for m in g["snaps"]], o32, o64, pre64, iters)


def log_exemptions(test, exempt, cap):
    line = "%s: %d of at most %d scene(s) passed through the float64-anchored threshold exemption: %s" % (
        test, len(exempt), cap, exempt)
    print("\n" + line)
    log = os.environ.get("SCARLET_LOG_REL_ERR")
    if log:
        with open(log, "a") as f:
            f.write("exempt    %s\n" % line)


def compare_fixed_iterations(g, ref, iters, straddle, max_exempt, test, exempt=None, flags=False):
    """a device run `g` (gpu_fit's result: status, it, cen, sed, morph, mse, flags; `iters` iterations at e_rel = 0)
    against the float32 oracle's results `ref` (oracle_fit's tuples, one per scene): status 0, the iteration count,
    centres bit-exact (and, if asked, the flags and the oracle's own count), sed / morph / loss history within TOL.
    A scene beyond TOL must pass `straddle(i)` -> (ok, message), the exemption of the module docstring; at most
    `max_exempt` scenes may, counted in `exempt` (a list a module can share between its tests).  Returns the worst
    errors."""
    S = len(ref)
    exempt = [] if exempt is None else exempt
    assert int(np.abs(g["status"]).sum()) == 0
    assert (g["it"] == iters).all()
    worst = dict(sed=0.0, morph=0.0, mse=0.0)
    for i in range(S):
        np.testing.assert_array_equal(g["cen"][i], ref[i][3])
        if flags:
            assert ref[i][4] == iters, (i, ref[i][4])
            np.testing.assert_array_equal(g["flags"][i], ref[i][5])
        e = dict(sed=rel_err(g["sed"][i], ref[i][0]), morph=rel_err(g["morph"][i], ref[i][1]),
                 mse=rel_err(g["mse"][i][:iters], ref[i][2]))
        if max(e.values()) <= TOL:
            for k in worst:
                worst[k] = max(worst[k], e[k])
            continue
        ok, msg = straddle(i)
        assert ok, "scene %d beyond 1e-5 (%s) and not a threshold straddle: %s" % (i, e, msg)
        exempt.append((i, e, msg))
    log_exemptions(test, exempt, max_exempt)
    assert len(exempt) <= max_exempt, exempt
    print("%d iterations x %d scenes: worst errors %s" % (iters, S, worst))
    return worst


def check_fixed_iterations(scarlet, wl, images, centers, pool, iters, max_exempt, test):
    """`iters` iterations at e_rel = 0 of every scene against the float32 oracle; returns the worst errors"""
    S = len(images)
    st0, g = gpu_fit(scarlet, wl, images, centers, iters, 0.0)
    okw = wl.oracle_kwargs()
    ref = pool.map(oracle_fit, [(images[i], st0[0][i], st0[1][i], st0[2][i], st0[3][i], iters, 0.0, np.float32, okw)
                                for i in range(S)])
    return compare_fixed_iterations(g, ref, iters, lambda i: straddles_threshold(scarlet, wl, images[i], centers[i], iters),
                                    max_exempt, test)
