"""TEST INFRASTRUCTURE: the count-mixture models under stochastic variational inference
(bayespy/demos/stochastic_inference.py:93-133), shared by tools/make_golden_mix_svi.py -- which runs
them on the live reference -- and the tests, which run them on this package:
``mods = dict(nodes=<module with the node classes>, VB=<class>, vb_kwargs=..., after_vb=...)``.

One case per block and two more: 400 rows, mini-batches of 70 (a batch crosses the tile of 64 rows),
m = 400 / 70, six steps of length (n + 2)^-0.7.  ``make_inputs`` gives the inputs, ``run_case`` the
recorded arrays: after every step the bound, the per-node bound terms (X, Z, the parameter node, R)
and the moments of the parameter node and the weights; at the end ``Z.u[0]`` of the last batch.

    bmm        Bernoulli, D = 65 (a second bit word), K = 3
    bmm_mask   the same with a mask of the full shape that changes with every batch
    pmm        Poisson, D = 5, K = 3, a mask in every batch; that of batch 2 hides column 1
    pmm_value  Poisson without a mask, ``lam`` starts from a value (a point mass)
    binm       binomial, D = 3, K = 2, trials per row
    cmm        categorical, D = 3, M = 4, K = 3
    mmm        multinomial, M = 7, K = 3, trials per row

The trials of the binomial and multinomial cases are constants of the model and belong to the row
of the batch, not to the row of the data: row r of the data has the trials of position r mod 70, and
position j of a batch is drawn among the rows j, j + 70, ..."""
import numpy as np

CASES = ('bmm', 'bmm_mask', 'pmm', 'pmm_value', 'binm', 'cmm', 'mmm')
N, NB, STEPS = 400, 70, 6
PARAM = dict(bmm='P', bmm_mask='P', pmm='lam', pmm_value='lam', binm='P', cmm='P', mmm='P')
MOMENTS = ('par_u0', 'par_u1', 'R_u0', 'Z_u0_last')


def scale(n):
    return (n + 2) ** (-0.7)


def make_inputs(rs):
    g = {}

    def batches(tag, by_position):
        if by_position:
            idx = np.stack([np.arange(NB) + NB * rs.randint(0, N // NB, size=NB)
                            for _ in range(STEPS)])
        else:
            idx = np.stack([rs.choice(N, NB) for _ in range(STEPS)])
        g[tag + '_batches'] = idx

    # Bernoulli
    D, K = 65, 3
    p = rs.beta(0.7, 0.7, size=(K, D))
    g['bmm_x'] = (rs.rand(N, D) < p[rs.randint(K, size=N)]).astype(np.uint8)
    g['bmm_init'] = rs.gamma(2.0, 1.0, size=(D, K, 2)) + 0.2
    batches('bmm', False)
    g['bmm_mask_masks'] = rs.rand(STEPS, NB, D) < 0.75
    g['bmm_mask_masks'][1, 5] = False               # a row of nothing
    # Poisson
    D, K = 5, 3
    rates = rs.gamma(2.0, 3.0, size=(K, D))
    g['pmm_x'] = rs.poisson(rates[rs.randint(K, size=N)]).astype(np.int64)
    g['pmm_init_a'] = rs.gamma(3.0, 2.0, size=(D, K)) + 0.5
    g['pmm_init_b'] = rs.gamma(3.0, 0.5, size=(D, K)) + 0.2
    g['pmm_value_lam0'] = rs.gamma(4.0, 1.5, size=(D, K))
    batches('pmm', False)
    g['pmm_masks'] = rs.rand(STEPS, NB, D) < 0.8
    g['pmm_masks'][2, :, 1] = False                 # a whole column hidden in batch 2
    # binomial, trials per row
    D, K = 3, 2
    g['binm_n'] = rs.randint(1, 30, size=(NB, 1, 1)).astype(np.int64)
    p = rs.beta(1.0, 1.0, size=(K, D))
    nrow = np.tile(g['binm_n'][:, 0, :], (N // NB + 1, 1))[:N]
    g['binm_x'] = rs.binomial(nrow, p[rs.randint(K, size=N)]).astype(np.int64)
    g['binm_init'] = rs.gamma(2.0, 1.0, size=(D, K, 2)) + 0.2
    batches('binm', True)
    # categorical
    D, M, K = 3, 4, 3
    p = rs.dirichlet(0.6 * np.ones(M), size=(K, D))
    z = rs.randint(K, size=N)
    g['cmm_x'] = np.array([[rs.choice(M, p=p[z[i], d]) for d in range(D)]
                           for i in range(N)]).astype(np.int64)
    g['cmm_init'] = rs.gamma(2.0, 1.0, size=(D, K, M)) + 0.2
    batches('cmm', False)
    # multinomial, trials per row
    M, K = 7, 3
    g['mmm_n'] = rs.randint(1, 40, size=(NB, 1)).astype(np.int64)
    p = rs.dirichlet(0.6 * np.ones(M), size=K)
    z = rs.randint(K, size=N)
    g['mmm_x'] = np.array([rs.multinomial(int(g['mmm_n'][i % NB, 0]), p[z[i]])
                           for i in range(N)]).astype(np.int64)
    g['mmm_init'] = rs.gamma(2.0, 1.0, size=(K, M)) + 0.2
    batches('mmm', True)
    return g


def source(tag):
    """The case whose data, batches and initial parameters ``tag`` runs on."""
    return dict(bmm_mask='bmm', pmm_value='pmm').get(tag, tag)


def build(mods, g, tag, m=N / NB):
    """The nodes of case ``tag``: dict(X, Z, par, R) -- nothing observed yet."""
    N_ = mods['nodes']
    src = source(tag)
    if src == 'mmm':
        K, M = g['mmm_init'].shape
        R = N_.Dirichlet(np.ones(K), name='R')
        Z = N_.Categorical(R, plates=(NB,), plates_multiplier=(m,), name='Z')
        P = N_.Dirichlet(0.5 * np.ones(M), plates=(K,), name='P')
        X = N_.Mixture(Z, N_.Multinomial, g['mmm_n'], P, name='X')
        P.initialize_from_parameters(g['mmm_init'])
        return dict(X=X, Z=Z, par=P, R=R)
    D, K = g[src + ('_init_a' if src == 'pmm' else '_init')].shape[:2]
    R = N_.Dirichlet(K * [0.7], name='R')
    Z = N_.Categorical(R, plates=(NB, 1), plates_multiplier=(m, 1), name='Z')
    if src == 'pmm':
        P = N_.Gamma(0.5, 0.1, plates=(D, K), name='lam')
        X = N_.Mixture(Z, N_.Poisson, P, name='X')
        if tag == 'pmm_value':
            P.initialize_from_value(g['pmm_value_lam0'])
        else:
            P.initialize_from_parameters(g['pmm_init_a'], g['pmm_init_b'])
        return dict(X=X, Z=Z, par=P, R=R)
    if src == 'cmm':
        P = N_.Dirichlet(g['cmm_init'].shape[2] * [0.5], plates=(D, K), name='P')
        X = N_.Mixture(Z, N_.Categorical, P, name='X')
    elif src == 'binm':
        P = N_.Beta([0.5, 0.8], plates=(D, K), name='P')
        X = N_.Mixture(Z, N_.Binomial, g['binm_n'], P, name='X')
    else:
        P = N_.Beta([0.5, 0.8], plates=(D, K), name='P')
        X = N_.Mixture(Z, N_.Bernoulli, P, name='X')
    P.initialize_from_parameters(g[src + '_init'])
    return dict(X=X, Z=Z, par=P, R=R)


def batch(g, tag, n):
    """(rows, mask or None) of step ``n`` of case ``tag``."""
    src = source(tag)
    rows = g[src + '_x'][g[src + '_batches'][n]]
    mask = g[tag + '_masks'][n] if tag + '_masks' in g else None
    if mask is not None:
        rows = np.where(mask, rows, 0)          # observe checks every value, hidden ones included
    return rows, mask


def observe(X, rows, mask):
    if mask is None:
        X.observe(rows)
    else:
        X.observe(rows, mask=mask)


def run_case(mods, g, tag, observe=observe, on_step=None, first=0, before=None):
    """Run the mini-batch loop of case ``tag`` from step ``first``; ``observe(X, rows, mask)`` may
    replace the host observation (device tensors), ``before(Q, m)`` runs once after the engine is
    built and the batch of step ``first`` observed (a checkpoint is loaded there), ``on_step(Q, m,
    n)`` after every step."""
    m = build(mods, g, tag)
    X, Z, P, R = m['X'], m['Z'], m['par'], m['R']
    observe(X, *batch(g, tag, first))
    Q = mods['VB'](X, Z, P, R, **mods.get('vb_kwargs', {}))
    Q.ignore_bound_checks = True
    if 'after_vb' in mods:
        mods['after_vb'](Q)
    if before is not None:
        before(Q, m)
    out = {k: [] for k in ('L', 'terms', 'par_u0', 'par_u1', 'R_u0')}
    for n in range(first, STEPS):
        if n > first:
            observe(X, *batch(g, tag, n))
        Q.update(Z, verbose=False)
        Q.gradient_step(P, R, scale=scale(n))
        out['L'].append(float(Q.compute_lowerbound()))
        out['terms'].append([float(x.lower_bound_contribution()) for x in (X, Z, P, R)])
        u = P.get_moments()
        out['par_u0'].append(np.array(u[0]))
        if len(u) > 1:
            out['par_u1'].append(np.array(u[1]))
        out['R_u0'].append(np.array(R.get_moments()[0]))
        if on_step is not None:
            on_step(Q, m, n)
    res = {tag + '_' + k: np.array(v) for k, v in out.items() if len(v)}
    res[tag + '_Z_u0_last'] = np.array(Z.get_moments()[0])
    res[tag + '_plan'] = Q
    return res
