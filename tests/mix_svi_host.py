"""TEST INFRASTRUCTURE for stochastic variational inference on the count-mixture blocks.

* ``restate_dirichlet_step`` / ``restate_gamma_step``: NumPy restatements of the two table kinds of
  ``vmp_mix_natural_step`` in a dtype of the caller's choice, with the bound terms in the
  reference's own form (cgf of the prior - cgf of q + sum (phi_p - phi_q) u).  float64 is the
  reference's arithmetic (SciPy), long double the yardstick (``special_ld``: digamma and ln Gamma by
  the recurrence up to x >= 24 and the asymptotic series, vectorised).
* ``StepDouble``: ``natural_step`` / ``natural_step_workspace`` for the kernel doubles of the five
  blocks (tests/*_host.py), and ``svi_double(tag)``: the double of a case of tests/mix_svi_models.py
  with them.
It lives under tests/ and is never imported by the product."""
import numpy as np


# -- special functions in long double ----------------------------------------------------------------
_B = (1.0 / 6, -1.0 / 30, 1.0 / 42, -1.0 / 30, 5.0 / 66, -691.0 / 2730, 7.0 / 6, -3617.0 / 510,
      43867.0 / 798)


def _shift(x):
    """(y >= 24, sum of 1 / (x + i), sum of log(x + i)) over the steps of the recurrence."""
    ld = np.longdouble
    y = np.array(x, dtype=ld)
    rec, logs = np.zeros_like(y), np.zeros_like(y)
    for _ in range(24):
        low = y < 24
        if not low.any():
            break
        rec = rec + np.where(low, 1 / np.where(low, y, 1), 0)
        logs = logs + np.where(low, np.log(np.where(low, y, 1)), 0)
        y = np.where(low, y + 1, y)
    return y, rec, logs


def digamma_ld(x):
    ld = np.longdouble
    y, rec, _ = _shift(x)
    inv2 = 1 / (y * y)
    s, p = np.zeros_like(y), inv2.copy()
    for k, b in enumerate(_B, 1):
        s = s + ld(b) / (2 * k) * p
        p = p * inv2
    return np.log(y) - 1 / (2 * y) - s - rec


def gammaln_ld(x):
    ld = np.longdouble
    y, _, logs = _shift(x)
    inv2 = 1 / (y * y)
    s, p = np.zeros_like(y), 1 / y
    for k, b in enumerate(_B, 1):
        s = s + ld(b) / (2 * k * (2 * k - 1)) * p
        p = p * inv2
    half_log_2pi = ld('0.918938533204672741780329736405617639861')
    return (y - ld(0.5)) * np.log(y) - y + half_log_2pi + s - logs


def special(dtype):
    if dtype == np.float64:
        from scipy.special import digamma, gammaln
        return digamma, gammaln
    return digamma_ld, gammaln_ld


# -- restatements ------------------------------------------------------------------------------------
def restate_dirichlet_step(prior, counts, alpha, mult, scale, dtype=np.longdouble):
    """rows x cols arrays -> dict(q, par, mom, bound): alpha <- alpha + scale (prior + mult counts -
    alpha); scale == 1 does not look at ``alpha``."""
    psi, lgam = special(dtype)
    prior = np.asarray(prior, dtype=dtype)
    q = prior + (0 if counts is None else dtype(mult) * np.asarray(counts, dtype=dtype))
    new = q if scale == 1 else np.asarray(alpha, dtype=dtype) \
        + dtype(scale) * (q - np.asarray(alpha, dtype=dtype))
    elog = psi(new) - psi(new.sum(-1, keepdims=True))

    def g(a):
        return lgam(a.sum(-1)) - lgam(a).sum(-1)
    bound = np.sum((prior - new) * elog) + np.sum(g(prior) - g(new))
    return dict(q=q, par=new, mom=elog, bound=bound)


def restate_gamma_step(a0, b0, S, cnt, par, mult, scale, dtype=np.longdouble):
    """(n,) priors and statistics (``cnt`` broadcast by the caller), par (n, 2) -> dict(q, par (n, 2),
    mom (n, 2), bound): a <- a + scale (a0 + mult S - a), b likewise."""
    psi, lgam = special(dtype)
    a0, b0 = np.asarray(a0, dtype=dtype).reshape(-1), np.asarray(b0, dtype=dtype).reshape(-1)
    zero = np.zeros_like(a0)
    S = zero if S is None else np.asarray(S, dtype=dtype).reshape(-1)
    cnt = zero if cnt is None else np.asarray(cnt, dtype=dtype).reshape(-1)
    q = np.stack([a0 + dtype(mult) * S, b0 + dtype(mult) * cnt], -1)
    if scale == 1:
        new = q
    else:
        old = np.asarray(par, dtype=dtype).reshape(-1, 2)
        new = old + dtype(scale) * (q - old)
    a, b = new[:, 0], new[:, 1]
    mom = np.stack([a / b, psi(a) - np.log(b)], -1)
    L = (a0 * np.log(b0) - lgam(a0)) - (a * np.log(b) - lgam(a)) + (-b0 + b) * mom[:, 0] \
        + (a0 - a) * mom[:, 1]
    return dict(q=q, par=new, mom=mom, bound=L.sum())


# -- the kernel doubles ------------------------------------------------------------------------------
class StepDouble:
    """Mixin of a kernels double that has ``calls``: the step in float64 NumPy / SciPy."""

    def natural_step_workspace(self, kind, rows, cols, K):
        return max(rows, 1)

    def natural_step(self, kind, nodes, rows, cols, rs, cs, prior, prior_b, stat, cnt, per_element,
                     par, mom, K, prior_r, Nk, alpha_r, elog_r, mult, scale, ws, bound):
        self.calls.append('natural_step_%d' % nodes)
        assert mult > 0 and K <= 64
        n = lambda t: None if t is None else t.numpy()       # noqa: E731
        out = {}
        if nodes & 1:
            if kind == 0:
                def view(t):
                    return np.lib.stride_tricks.as_strided(t.numpy().reshape(-1),
                                                           shape=(rows, cols),
                                                           strides=(8 * rs, 8 * cs))
                o = restate_dirichlet_step(view(prior), None if stat is None else view(stat),
                                           view(par).copy(), mult, scale, np.float64)
                out['table'] = (view(par), view(mom), o)
            else:
                c = None if cnt is None else \
                    (n(cnt).reshape(-1) if per_element
                     else np.broadcast_to(n(cnt).reshape(-1), (rows // K, K)).reshape(-1))
                o = restate_gamma_step(n(prior), n(prior_b), n(stat), c, n(par).copy(), mult, scale,
                                       np.float64)
                out['table'] = (n(par).reshape(-1, 2), n(mom).reshape(-1, 2), o)
        if nodes & 2:
            o = restate_dirichlet_step(n(prior_r).reshape(1, K),
                                       None if Nk is None else n(Nk).reshape(1, K),
                                       n(alpha_r).reshape(1, K).copy(), mult, scale, np.float64)
            out['weights'] = (n(alpha_r).reshape(1, K), n(elog_r).reshape(1, K), o)
        # every optimum was formed before anything is written
        for slot, key in ((0, 'table'), (1, 'weights')):
            if key in out:
                p, m, o = out[key]
                p[...] = o['par']
                m[...] = o['mom']
                bound.numpy()[slot] = float(o['bound'])


def _double_class(tag):
    if tag.startswith('bmm'):
        from bmm_masked_host import CPUBMMMaskedKernels as Base
    elif tag.startswith('pmm'):
        from pmm_host import CPUPMMKernels as Base
    elif tag == 'binm':
        from binm_host import CPUBINMKernels as Base
    elif tag == 'cmm':
        from cmm_host import CPUCMMKernels as Base
    else:
        from mmm_host import CPUMMMKernels as Base
    return type('SVI' + Base.__name__, (StepDouble, Base), {})


PLAN = dict(bmm='BernoulliMixtureSVIPlan', bmm_mask='BernoulliMixtureSVIPlan',
            pmm='PoissonMixtureSVIPlan', pmm_value='PoissonMixtureSVIPlan',
            binm='BinomialMixtureSVIPlan', cmm='CategoricalMixtureSVIPlan',
            mmm='MultinomialMixtureSVIPlan')


def on_double(tag):
    """``after_vb`` of the model scripts: the plan of case ``tag`` on its kernel double."""
    def go(Q):
        from bayespy_amd.device import Runtime
        plan = Q.plans[0]
        assert type(plan).__name__ == PLAN[tag], type(plan).__name__
        rt = Runtime(device='cpu')
        plan._rt, plan._kernels = rt, _double_class(tag)(rt)
    return go
