"""Shared by tests/test_observations_prior_abi.py (CPU) and tests/test_gpu_observations_prior.py (GPU): the cases of
the joint fit with priors and their oracle.

A `Case` is host data only: the observations of S scenes, a start state computed on the host (the device receives it
through set_state and hands the same bits back, so the CPU test and the GPU tests describe the same fits), the prior's
weights and targets, and the switches of the fit.  `case.spec(st0, i)` is scene i for the oracle:
tests/prior_common.py's dict (images are zeros: the data are in `obs`) plus
  obs : the scene's observations as oracle.pgm.fit reads them from `scene.observations` (images, band_slice, weights,
        diff_kernel), a low-resolution one with `factors` instead of `diff_kernel` (tests/lowres_common.py)
  l1  : l1_thresh or None
Without a low-resolution observation the oracle is oracle.pgm.fit itself; with one it is tests/lowres_common.fit's loop
restated with the prior (oracle/pgm.py:747-764).
"""
import numpy as np

from conftest import rel_err
import prior_common as prc

TOL = prc.TOL
F32 = np.float32


class Case(object):
    def __init__(self, name, obs, centers, sed0, morph0, counts=None, iters=5, e_rel=0.0, **kw):
        self.name, self.obs, self.iters, self.e_rel = name, obs, iters, e_rel
        self.sed0, self.morph0 = sed0.astype(F32), morph0.astype(F32)
        self.centers = np.asarray(centers, np.int32)
        self.S, self.K, self.C = self.sed0.shape
        self.H, self.W = self.morph0.shape[-2:]
        self.ragged = counts is not None
        self.n = np.full(self.S, self.K, np.int32) if counts is None else np.asarray(counts, np.int32)
        self.ws = self.wm = self.ts = self.tm = None
        self.fix_sed = self.fix_morph = self.group = self.l0 = self.l1 = self.cw = None
        self.approximate_L = False
        for key, v in kw.items():
            assert hasattr(self, key), key
            setattr(self, key, v)

    def host_state(self):
        """the start as the device reports it after set_state (no centroid shift yet)"""
        return dict(sed=self.sed0, morph=self.morph0, cen=self.centers, sh=np.full((self.S, self.K, 2), np.nan))

    def spec(self, st0, i, prior=True):
        n = int(self.n[i])
        cut = lambda a: None if a is None else np.asarray(a)[i][:n]
        obs = []
        for o in self.obs:
            w = o.get("weights")
            d = dict(images=o["images"][i], band_slice=slice(o["band0"], o["band0"] + o["images"].shape[1]),
                     weights=1 if w is None else (w if np.ndim(w) == 0 else w[i]))
            if o.get("lowres") is not None:
                d["factors"] = o["lowres"].factors
            else:
                d["diff_kernel"] = o.get("diff")
            obs.append(d)
        sh = st0["sh"][i][:n]
        okw = dict(l0_thresh=self.l0)
        if self.cw is not None:
            okw["centroid_weight"] = self.cw
        return dict(images=np.zeros((self.C, self.H, self.W), F32), sed0=st0["sed"][i][:n], morph0=st0["morph"][i][:n],
                    cen0=st0["cen"][i][:n], sh0=None if np.isnan(sh).any() else sh,
                    ws=cut(self.ws) if prior else None, wm=cut(self.wm) if prior else None, ts=cut(self.ts), tm=cut(self.tm),
                    fix_sed=cut(self.fix_sed), fix_morph=cut(self.fix_morph), group=cut(self.group), okw=okw,
                    approximate_L=self.approximate_L, obs=obs, l1=self.l1)


# ------------------------------------------------------------------ the oracle
def build_scene(spec, dt):
    sc = prc.build_scene(spec, dt)
    sc.observations = []
    for o in spec["obs"]:
        d = dict(o, images=np.asarray(o["images"]).astype(dt))
        if np.ndim(d["weights"]):
            d["weights"] = np.asarray(d["weights"]).astype(dt)
        if d.get("diff_kernel") is not None:
            d["diff_kernel"] = np.asarray(d["diff_kernel"]).astype(dt)
        sc.observations.append(d)
    if spec.get("l1") is not None:
        for s in sc.sources:
            s.l1_thresh = spec["l1"]
    return sc


def lowres_fit(scene, max_iter, e_rel=0, approximate_L=False, callback=None):
    """tests/lowres_common.fit with the prior of every component (oracle/pgm.py:747-764) and pgm.fit's callback"""
    from oracle import pgm
    import lowres_common as lc
    for _ in range(max_iter):
        seds = [c.sed for c in scene.sources]
        morphs = [c.morph for c in scene.sources]
        loss = 0
        gs = [np.zeros_like(sd) for sd in seds]
        gm = [np.zeros_like(m) for m in morphs]
        for ob in scene.observations:
            sl = ob["band_slice"]
            sub = [sd[sl] for sd in seds]
            if "factors" in ob:
                l_, gs_, gm_ = lc.lowres_loss_and_gradients(sub, morphs, ob)
            else:
                l_, gs_, gm_ = pgm.loss_and_gradients(sub, morphs, ob["images"], ob.get("weights", 1), ob.get("diff_kernel"))
            loss = loss + l_
            for k in range(len(seds)):
                gs[k][sl] += gs_[k]
                gm[k] = gm[k] + gm_[k]
        scene.mse.append(loss)
        L_sed, L_morph = pgm.lipschitz(seds, morphs, len(scene.observations), approximate_L, scene.mse)
        for c, g_s, g_m in zip(scene.sources, gs, gm):
            c.L_sed, c.L_morph = L_sed, L_morph
            prior = getattr(c, "prior", None)
            if prior is not None:
                p_gs, p_gm = prior[0](c.sed, c.morph)
                p_Ls, p_Lm = prior[1](c.sed, c.morph)
                if not c.fix_morph:
                    g_m = g_m + p_gm
                    c.L_morph = c.L_morph + p_Lm
                if not c.fix_sed:
                    g_s = g_s + p_gs
                    c.L_sed = c.L_sed + p_Ls
            if not c.fix_sed:
                c.sed = c.sed - (1 / c.L_sed) * g_s
            if not c.fix_morph:
                c.morph = c.morph - (1 / c.L_morph) * g_m
        for c in scene.sources:
            pgm.source_update(c, scene.it)
        if callback is not None:
            callback(scene)
        if pgm.check_convergence(scene, e_rel):
            break
    return scene


def run(sc, spec, iters, e_rel, callback=None):
    from oracle import pgm
    approx = bool(spec.get("approximate_L"))
    if any("factors" in o for o in spec["obs"]):
        return lowres_fit(sc, iters, e_rel, approx, callback)
    return pgm.fit(sc, iters, e_rel=e_rel, approximate_L=approx, callback=callback)


def oracle_fit(args):
    """(spec, iters, e_rel, dtype) -> sed, morph, mse, centres, it, flags (a worker of a spawned pool: no GPU)"""
    spec, iters, e_rel, dt = args
    sc = build_scene(spec, dt)
    run(sc, spec, iters, e_rel)
    return (np.array([s.sed for s in sc.sources]), np.array([s.morph for s in sc.sources]), np.array(sc.mse),
            np.array([s.center for s in sc.sources]), len(sc.mse), [int(s.flags) for s in sc.sources])


def oracle_trace(args):
    """(spec, iters, dtype) -> per iteration: the morphologies after it, and (stepped, as prox_plus saw them)"""
    spec, iters, dt = args
    sc = build_scene(spec, dt)
    for s in sc.sources:
        s.trace = dict(step=[], pre_plus=[])
    post = []
    run(sc, spec, iters, 0, callback=lambda scn: post.append(np.array([s.morph.copy() for s in scn.sources])))
    # (the layers of a multi-component source leave no trace: inf there, so the threshold rule never excuses them)
    at = lambda s, key, t: s.trace[key][t] if len(s.trace[key]) > t else np.full_like(s.morph, np.inf)
    pre = [(np.array([at(s, "step", t) for s in sc.sources]), np.array([at(s, "pre_plus", t) for s in sc.sources]))
           for t in range(iters)]
    return post, pre


def straddles_threshold(gpu_snaps, spec, iters):
    """prior_common.straddles_threshold with this module's oracle: accepts the scene only if GPU and float32 oracle agree
    within 1e-5 before t0, disagree about the SUPPORT in a pixel at t0, and the float64 trajectory's value at that pixel
    at one of the two threshold tests of t0 lies within 1e-5 x max|morph| of 0.  Returns (ok, message)."""
    o32, _ = oracle_trace((spec, iters, np.float32))
    o64, pre64 = oracle_trace((spec, iters, np.float64))
    for t in range(iters):
        gm = gpu_snaps[t]
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


def supports_agree(args):
    """(spec, iters) -> None, or where the float32 and float64 oracles first disagree about a morphology's support"""
    spec, iters = args
    o32, _ = oracle_trace((spec, iters, np.float32))
    o64, _ = oracle_trace((spec, iters, np.float64))
    for t in range(iters):
        bad = (o32[t] == 0) != (o64[t] == 0)
        if bad.any():
            k, y, x = (int(v[0]) for v in np.nonzero(bad))
            return "iteration %d, component %d, pixel (%d, %d): float32 %.3e, float64 %.3e" % (
                t + 1, k, y, x, o32[t][k, y, x], o64[t][k, y, x])
    return None


# ------------------------------------------------------------------ the cases
def _scenes(first, S, C=5, H=64, W=64, K=3, min_sep=4):
    """S synthetic scenes and a host start: the true morphologies widened and cut to a support, the true SEDs x 0.8"""
    from scarlet_amd import synth
    sc = [synth.make_scene(first + i, B=C, H=H, W=W, K=K, min_sep=min_sep) for i in range(S)]
    images = np.stack([s["images"] for s in sc])
    centers = np.stack([s["centers"] for s in sc])
    morph = np.stack([s["true_morphs"] for s in sc]) ** 0.6
    morph[morph < 0.03] = 0
    sed = 0.8 * np.stack([s["true_seds"] for s in sc])
    return images.astype(F32), centers, sed.astype(F32), morph.astype(F32)


def _sliced(images):
    return [dict(images=images[:, :3], band0=0), dict(images=images[:, 3:], band0=3)]


def _epochs(images, seed):
    rng = np.random.default_rng(seed)
    return [dict(images=images, band0=0),
            dict(images=(images + 0.05 * rng.standard_normal(images.shape)).astype(F32), band0=0)]


def _prior_on(case, comps, ws=20.0, wm=2000.0):
    """weights on the components `comps` of every scene, targets = the start"""
    on = np.zeros((case.S, case.K), F32)
    on[:, list(comps)] = 1
    case.ws, case.wm = F32(ws) * on, F32(wm) * on
    case.ts, case.tm = case.sed0.copy(), case.morph0.copy()
    return case


def two_obs(layout="sliced", first=6000, H=30, W=34, S=4, **kw):
    images, centers, sed, morph = _scenes(first, S, H=H, W=W)
    obs = _sliced(images) if layout == "sliced" else _epochs(images, first)
    name = kw.pop("name", "%s_%dx%d" % (layout, H, W))
    return _prior_on(Case(name, obs, centers, sed, morph, **kw), (0, 2))


def many_components(K, side, first, min_sep):
    images, centers, sed, morph = _scenes(first, 2, H=side, W=side, K=K, min_sep=min_sep)
    return _prior_on(Case("k%d" % K, _sliced(images), centers, sed, morph, iters=4), range(0, K, 2))


def psf_mixed(first=6300):
    """bands 0-2 observed through a PSF (difference kernel: G planes), bands 3-4 on the model's grid (inline)"""
    from oracle import pgm
    from scarlet_amd import synth
    model = synth.gaussian_psf((11, 11), 0.9)
    psfs = np.array([synth.gaussian_psf((11, 11), 1.2 + 0.15 * b) for b in range(3)])
    diff = pgm.match_psfs(psfs.astype(F32), model[None].astype(F32)).astype(F32)
    images, centers, sed, morph = _scenes(first, 2, H=32, W=32)
    obs = [dict(images=images[:, :3], band0=0, diff=diff), dict(images=images[:, 3:], band0=3)]
    return _prior_on(Case("psf_mixed", obs, centers, sed, morph, cw=model.astype(F32)), (0, 2))


def ragged(first=6400):
    """counts 4, 2, 3, 4; fixed factors; scene 3 is a two-layer source (components 0, 1) and two single ones"""
    S, K = 4, 4
    images, centers, sed, morph = _scenes(first, S, H=32, W=32, K=K)
    counts = np.array([4, 2, 3, 4], np.int32)
    group = np.full((S, K), -1, np.int32)
    group[3, :2] = 0
    centers[3, 1] = centers[3, 0]
    morph[3, 1] = morph[3, 0] ** 2
    sed[3, 1] = 0.5 * sed[3, 0]
    s, k = np.mgrid[:S, :K]
    fix_sed, fix_morph = (s + k) % 4 == 1, (s + k) % 4 == 2
    fix_sed[3, :2] = fix_morph[3, :2] = False
    present = k < counts[:, None]
    sed[~present] = 0
    morph[~present] = 0
    case = Case("ragged", _sliced(images), centers, sed, morph, counts=counts, fix_sed=fix_sed, fix_morph=fix_morph,
                group=group, iters=6)
    return _prior_on(case, range(K))                               # every component, the fixed ones included


def lowres(S=2):
    """geometry "a" of tests/golden/lowres.npz (32 x 32 model, 16 x 16 observation of bands 3-4) beside a model-grid
    observation of bands 0-2 with a difference kernel; scene 0 is the fixture's, scene 1 other noise and another start"""
    import lowres_common as lc
    obs, (sed0, morph0, cen0), cw, lo = lc.fit_inputs(lc.fixture(), "a")
    rng = np.random.default_rng(23)
    hr = np.stack([obs[0]["images"] + (0.02 * rng.standard_normal(obs[0]["images"].shape) if s else 0) for s in range(S)])
    lr = np.stack([obs[1]["images"] + (0.02 * rng.standard_normal(obs[1]["images"].shape) if s else 0) for s in range(S)])
    wl = np.stack([obs[1]["weights"] * (1 + 0.2 * s) for s in range(S)])
    sed = np.stack([sed0 * (1 + 0.1 * s) for s in range(S)])
    data = [dict(images=hr.astype(F32), band0=0, diff=obs[0]["diff_kernel"]),
            dict(images=lr.astype(F32), band0=3, weights=wl.astype(F32), lowres=lo)]
    case = Case("lowres", data, np.stack([cen0] * S), sed, np.stack([morph0] * S), cw=np.asarray(cw, F32), iters=6)
    return _prior_on(case, range(case.K))


def stopping():
    """scenes that reach e_rel after different numbers of iterations, all within 10"""
    return two_obs("sliced", first=6500, S=6, name="stopping", iters=10, e_rel=STOP_E_REL)


STOP_E_REL = 0.05

CASES = {
    "sliced_30x34": lambda: two_obs("sliced"),
    "epochs_30x34": lambda: two_obs("epochs", first=6050),
    "two_tiles_72x60": lambda: two_obs("sliced", first=6100, H=72, W=60, S=2),
    "k9": lambda: many_components(9, 32, 6200, 3),
    "k33": lambda: many_components(33, 48, 6250, 2),
    "approximate_L": lambda: two_obs("sliced", first=6020, name="approximate_L", approximate_L=True),
    "psf_mixed": psf_mixed,
    "ragged": ragged,
    "l0": lambda: two_obs("sliced", first=6600, name="l0", l0=0.05, iters=10),
    "l1": lambda: two_obs("sliced", first=6650, name="l1", l1=0.05, iters=10),
    "lowres": lowres,
    "forms": lambda: two_obs("sliced", first=6700, name="forms", l0=0.05, iters=10),
    "stopping": stopping,
}
