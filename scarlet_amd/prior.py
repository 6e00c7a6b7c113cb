"""Priors of a batch (reference Prior / Component.backward_prior, component.py:39-67, 177-187).

A prior adds a gradient and a Lipschitz constant to the step of ONE component.  `BlendBatch.fit(prior=...)` and
`BlendBatch.step(prior=...)` take

  - a `QuadraticPrior`: w/2 |x - target|^2 per component and factor, evaluated by the library (gradient w (x - target),
    constant w) -- the whole fit is one call of scarlet_fit_constrained (scarlet_fit_observations_prior for a batch made
    by `from_observations`, whose SEDs are (S, K, C) over the model frame's channels);
  - a dict of given device tensors, any subset of `GIVEN_KEYS`: constant gradients (a linear prior) and constants;
  - a callable `fn(sed, morph) -> dict` of the same keys, called once per iteration with the current factors
    ((S, K, B) and (S, K, H, W) device tensors) on the current stream;
  - a list of these (at most one QuadraticPrior); given values add up.

The functions of this module that do not take a batch run without a device.
"""
import numpy as np

GIVEN_KEYS = ("grad_sed", "grad_morph", "L_sed", "L_morph")


def expand_weights(w, S, K, name="weight"):
    """A weight per component from a scalar, (K,) or (S, K) host value -> (S, K) float32 array.

    Raises ValueError for another shape, for a negative or a non-finite weight (the weight is the prior's Lipschitz
    constant: the step 1 / (L + w) needs w >= 0)."""
    a = np.asarray(w, dtype=np.float64)
    if a.shape not in ((), (K,), (S, K)):
        raise ValueError("%s must be a scalar, (K,) = (%d,) or (S, K) = (%d, %d), not %s" % (name, K, S, K, a.shape))
    if not np.isfinite(a).all():
        raise ValueError("%s must be finite" % name)
    if (a < 0).any():
        raise ValueError("%s must be >= 0 (it is added to the Lipschitz constant), min is %g" % (name, a.min()))
    return np.ascontiguousarray(np.broadcast_to(a, (S, K)), dtype=np.float32)


def check_target(shape, full, name):
    """A target must broadcast to the factor's shape (S, K, B) / (S, K, H, W)."""
    try:
        ok = np.broadcast_shapes(tuple(shape), tuple(full)) == tuple(full)
    except ValueError:
        ok = False
    if not ok:
        raise ValueError("%s of shape %s does not broadcast to %s" % (name, tuple(shape), tuple(full)))


class QuadraticPrior(object):
    """w/2 |x - target|^2 on the SEDs and / or the morphologies of a batch's components.

    sed_weight, morph_weight : None, a scalar, (K,) or (S, K): the weight of every component (0 = no prior there);
        host values are checked here (>= 0), device tensors are taken as they are
    sed_target, morph_target : None (= 0), or an array / tensor that broadcasts to (S, K, B) / (S, K, H, W); a target
        needs its weight
    """

    def __init__(self, sed_weight=None, sed_target=None, morph_weight=None, morph_target=None):
        if sed_target is not None and sed_weight is None:
            raise ValueError("QuadraticPrior: sed_target without sed_weight")
        if morph_target is not None and morph_weight is None:
            raise ValueError("QuadraticPrior: morph_target without morph_weight")
        for name, w in (("sed_weight", sed_weight), ("morph_weight", morph_weight)):
            if w is not None and not _is_tensor(w):
                a = np.asarray(w, dtype=np.float64)
                if a.ndim > 2:
                    raise ValueError("QuadraticPrior: %s must be a scalar, (K,) or (S, K), not %s" % (name, a.shape))
                if not np.isfinite(a).all() or (a < 0).any():
                    raise ValueError("QuadraticPrior: %s must be finite and >= 0" % name)
        self.sed_weight, self.sed_target = sed_weight, sed_target
        self.morph_weight, self.morph_target = morph_weight, morph_target

    def host_weights(self, S, K):
        """The (S, K) float32 weights of a batch of S scenes x K components, (None where there is no prior); runs
        without a device when the weights were given as host values."""
        out = []
        for name, w in (("sed_weight", self.sed_weight), ("morph_weight", self.morph_weight)):
            if w is None:
                out.append(None)
            else:
                out.append(expand_weights(w.detach().cpu().numpy() if _is_tensor(w) else w, S, K, name))
        return tuple(out)

    def bind(self, batch):
        """Device tensors for `batch`: dict of quad_sed_weight, quad_sed_target, quad_morph_weight, quad_morph_target
        (None where absent), float32, contiguous, full shape."""
        t, S, K = batch.torch, batch.S, batch.K
        f32 = dict(dtype=t.float32, device=batch.device)
        out = {}
        full = dict(sed=(S, K, batch.B), morph=(S, K, batch.H, batch.W))
        for fac, w, tgt in (("sed", self.sed_weight, self.sed_target), ("morph", self.morph_weight, self.morph_target)):
            wt = tt = None
            if w is not None:
                if _is_tensor(w):
                    if tuple(w.shape) not in ((), (K,), (S, K)):
                        raise ValueError("%s_weight must be a scalar, (K,) or (S, K), not %s" % (fac, tuple(w.shape)))
                    wt = w.to(**f32).expand(S, K).contiguous()
                else:
                    wt = t.as_tensor(expand_weights(w, S, K, fac + "_weight")).to(**f32)
            if tgt is not None:
                tt = (tgt if _is_tensor(tgt) else t.as_tensor(np.asarray(tgt, dtype=np.float32))).to(**f32)
                check_target(tt.shape, full[fac], fac + "_target")
                tt = tt.expand(full[fac]).contiguous()
            out["quad_%s_weight" % fac], out["quad_%s_target" % fac] = wt, tt
        return out


def _is_tensor(x):
    return hasattr(x, "data_ptr") and hasattr(x, "device")


def split_priors(prior):
    """prior argument of fit() / step() -> (QuadraticPrior or None, [dicts of given values], [callables])."""
    items = list(prior) if isinstance(prior, (list, tuple)) else [prior]
    quad, given, fns = None, [], []
    for p in items:
        if isinstance(p, QuadraticPrior):
            if quad is not None:
                raise ValueError("prior: at most one QuadraticPrior (add the weights up instead)")
            quad = p
        elif isinstance(p, dict):
            check_given_keys(p)
            given.append(p)
        elif callable(p):
            fns.append(p)
        else:
            raise ValueError("prior: a QuadraticPrior, a dict of %s, a callable or a list of these, not %r"
                             % (", ".join(GIVEN_KEYS), type(p).__name__))
    return quad, given, fns


def check_given_keys(d):
    if not isinstance(d, dict):
        raise ValueError("a prior callable must return a dict of %s, not %r" % (", ".join(GIVEN_KEYS), type(d).__name__))
    unknown = set(d) - set(GIVEN_KEYS)
    if unknown:
        raise ValueError("prior: unknown key %r (one of %s)" % (sorted(unknown)[0], ", ".join(GIVEN_KEYS)))
