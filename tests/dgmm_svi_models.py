"""TEST INFRASTRUCTURE: the diagonal-Gaussian mixture under stochastic variational inference
(bayespy/demos/stochastic_inference.py:93-133), shared by tools/make_golden_dgmm_svi.py -- which
runs the cases on the live reference -- and the tests, which run them on this package:
``mods = dict(nodes=<module with the node classes>, VB=<class>, vb_kwargs=..., after_vb=...)``.

400 rows, mini-batches of 70 (a batch crosses the tile of 64 rows), D = 5, K = 3, m = 400 / 70, six
steps of length (n + 2)^-0.7; priors mu (0.3, 0.1), tau (0.5, 0.2), weights 0.7.  ``make_inputs``
gives the inputs, ``run_case`` the recorded arrays: after every step the bound, the five per-node
bound terms (Y, Z, mu, tau, alpha) and the moments of mu, tau and the weights; at the end ``Z.u[0]``
of the last batch.

    par     ``mu`` and ``tau`` start from given parameters
    value   ``mu`` starts from a value (a point mass)
    mask    as ``par`` with a mask of the full shape that changes with every batch; batch 1 has a
            row with nothing observed, batch 2 hides column 1"""
import numpy as np

CASES = ('par', 'value', 'mask')
N, NB, STEPS, D, K = 400, 70, 6, 5, 3
TERMS = ('Y', 'Z', 'mu', 'tau', 'alpha')
MOMENTS = ('mu_u0', 'mu_u1', 'tau_u0', 'tau_u1', 'alpha_u0', 'Z_u0_last')
HIDDEN_BATCH, HIDDEN_COLUMN = 2, 1


def scale(n):
    return (n + 2) ** (-0.7)


def make_inputs(rs):
    g = {}
    centres = 2.5 * rs.normal(size=(K, D))
    widths = rs.gamma(4.0, 0.25, size=(K, D)) + 0.3
    z = rs.randint(K, size=N)
    g['y'] = centres[z] + widths[z] * rs.normal(size=(N, D))
    g['batches'] = np.stack([rs.choice(N, NB) for _ in range(STEPS)])
    g['init_m'] = centres.T + 0.8 * rs.normal(size=(D, K))
    g['init_lam'] = rs.gamma(3.0, 1.0, size=(D, K)) + 0.2
    g['init_a'] = rs.gamma(3.0, 1.0, size=(D, K)) + 0.5
    g['init_b'] = rs.gamma(3.0, 1.0, size=(D, K)) + 0.5
    g['value_mu0'] = centres.T + 0.8 * rs.normal(size=(D, K))
    g['mask_masks'] = rs.rand(STEPS, NB, D) < 0.8
    g['mask_masks'][1, 5] = False                               # a row of nothing
    g['mask_masks'][HIDDEN_BATCH, :, HIDDEN_COLUMN] = False     # a whole column hidden
    return g


def build(mods, g, tag, m=N / NB):
    """The nodes of case ``tag``: dict(Y, Z, mu, tau, alpha) -- nothing observed yet."""
    N_ = mods['nodes']
    alpha = N_.Dirichlet(K * [0.7], name='alpha')
    Z = N_.Categorical(alpha, plates=(NB, 1), plates_multiplier=(m, 1), name='Z')
    mu = N_.GaussianARD(0.3, 0.1, plates=(D, K), name='mu')
    tau = N_.Gamma(0.5, 0.2, plates=(D, K), name='tau')
    Y = N_.Mixture(Z, N_.GaussianARD, mu, tau, name='Y')
    if tag == 'value':
        mu.initialize_from_value(g['value_mu0'])
    else:
        mu.initialize_from_parameters(g['init_m'], g['init_lam'])
    tau.initialize_from_parameters(g['init_a'], g['init_b'])
    return dict(Y=Y, Z=Z, mu=mu, tau=tau, alpha=alpha)


def nodes_of(m):
    return [m[k] for k in ('Y', 'Z', 'mu', 'tau', 'alpha')]


def batch(g, tag, n):
    """(rows, mask or None) of step ``n`` of case ``tag``."""
    rows = g['y'][g['batches'][n]]
    mask = g['mask_masks'][n] if tag == 'mask' else None
    if mask is not None:
        rows = np.where(mask, rows, 0.0)
    return rows, mask


def observe(Y, rows, mask):
    if mask is None:
        Y.observe(rows)
    else:
        Y.observe(rows, mask=mask)


def run_case(mods, g, tag, observe=observe, on_step=None, first=0, before=None):
    """Run the mini-batch loop of case ``tag`` from step ``first``; ``observe(Y, rows, mask)`` may
    replace the host observation (device tensors), ``before(Q, m)`` runs once after the engine is
    built and the batch of step ``first`` observed (a checkpoint is loaded there), ``on_step(Q, m,
    n)`` after every step."""
    m = build(mods, g, tag)
    Y, Z, mu, tau, alpha = nodes_of(m)
    observe(Y, *batch(g, tag, first))
    Q = mods['VB'](Y, Z, mu, tau, alpha, **mods.get('vb_kwargs', {}))
    Q.ignore_bound_checks = True
    if 'after_vb' in mods:
        mods['after_vb'](Q)
    if before is not None:
        before(Q, m)
    out = {k: [] for k in ('L', 'terms') + MOMENTS[:-1]}
    for n in range(first, STEPS):
        if n > first:
            observe(Y, *batch(g, tag, n))
        Q.update(Z, verbose=False)
        Q.gradient_step(mu, tau, alpha, scale=scale(n))
        out['L'].append(float(Q.compute_lowerbound()))
        out['terms'].append([float(x.lower_bound_contribution()) for x in nodes_of(m)])
        for key, node in (('mu', mu), ('tau', tau)):
            u = node.get_moments()
            out[key + '_u0'].append(np.array(u[0]))
            out[key + '_u1'].append(np.array(u[1]))
        out['alpha_u0'].append(np.array(alpha.get_moments()[0]))
        if on_step is not None:
            on_step(Q, m, n)
    res = {tag + '_' + k: np.array(v) for k, v in out.items()}
    res[tag + '_Z_u0_last'] = np.array(Z.get_moments()[0])
    res[tag + '_plan'] = Q
    return res
