"""CPU: what the plate-mixture blocks share (bayespy_amd/inference/plans/_mixture.py) and no test
of a single block pins -- the layout of a checkpoint of every block, the three errors of an
initial value of ``Z`` in every block, and that a reason of a shared check of the matcher comes
from the block of the model's family alone, in the same words from ``match`` and from
``compile_model``.  Every plan runs on its kernel double (tests/*_host.py) at the sizes of its
fixture (tests/golden/*.npz)."""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

# block -> (plan module, plan class, fixture, model scripts, their run function, case, module and
# class of the kernel double)
BLOCKS = dict(
    bmm=('bmm', 'BernoulliMixturePlan', 'bmm_fused.npz', 'bmm_models', 'run_bmm_cases', 'e',
         'bmm_host', 'CPUBMMKernels'),
    bmm_masked=('bmm', 'BernoulliMixturePlan', 'bmm_masked.npz', 'bmm_masked_models',
                'run_masked_cases', 'e', 'bmm_masked_host', 'CPUBMMMaskedKernels'),
    dgmm=('dgmm', 'DiagGaussianMixturePlan', 'dgmm.npz', 'dgmm_models', 'run_cases', 'f',
          'dgmm_host', 'CPUDGMMKernels'),
    dgmm_masked=('dgmm_masked', 'MaskedDiagGaussianMixturePlan', 'dgmm_masked.npz',
                 'dgmm_masked_models', 'run_masked_cases', 'f', 'dgmm_masked_host',
                 'CPUDGMMMaskedKernels'),
    cmm=('cmm', 'CategoricalMixturePlan', 'cmm.npz', 'cmm_models', 'run_cmm_cases', 'f',
         'cmm_host', 'CPUCMMKernels'),
    pmm=('pmm', 'PoissonMixturePlan', 'pmm.npz', 'pmm_models', 'run_pmm_cases', 'f', 'pmm_host',
         'CPUPMMKernels'),
)
LABELS = dict(bmm='fused Bernoulli-mixture block', dgmm='fused diagonal-Gaussian-mixture block',
              cmm='fused categorical-mixture block', pmm='fused Poisson-mixture block')


def _plan_class(block):
    mod = importlib.import_module('bayespy_amd.inference.plans.' + BLOCKS[block][0])
    return getattr(mod, BLOCKS[block][1])


def _inputs(block):
    g = np.load(os.path.join(GOLDEN, BLOCKS[block][2]))
    ints = block in ('cmm', 'pmm')
    return {k[3:]: (g[k].astype(np.int64) if ints and k.endswith('_x') else g[k])
            for k in g.files if k.startswith('in_')}


def _on_double(block):
    def install(Q):
        from bayespy_amd.device import Runtime
        plan = Q.plans[0]
        assert type(plan) is _plan_class(block)
        rt = Runtime(device='cpu')
        plan._rt = rt
        plan._kernels = getattr(importlib.import_module(BLOCKS[block][6]), BLOCKS[block][7])(rt)
    return install


def _mods(block):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    return dict(nodes=nodes, VB=VB, vb_kwargs=dict(engine='fused'), after_vb=_on_double(block))


# -- the layout of a checkpoint --------------------------------------------------------------------
# sorted (key, dtype, shape) of what ``save_state`` puts after two updates of every node, as the
# blocks wrote it before they had a common base
F8, I8, U1 = 'float64', 'int64', 'uint8'
LAYOUT = dict(
    bmm=[('Nk', F8, (2,)), ('S', F8, (9, 2)), ('alpha_p', F8, (18, 2)), ('alpha_r', F8, (2,)),
         ('c', F8, (2,)), ('counts', F8, (18, 2)), ('delta_roles', U1, (0,)), ('dims', I8, (3,)),
         ('elog_p', F8, (18, 2)), ('elog_r', F8, (2,)), ('flags', I8, (1,)), ('kind', U1, (3,)),
         ('scal', F8, (8,)), ('w', F8, (9, 2))],
    bmm_masked=[('M', F8, (5, 1)), ('Nk', F8, (1,)), ('S', F8, (5, 1)), ('alpha_p', F8, (5, 2)),
                ('alpha_r', F8, (1,)), ('c', F8, (1,)), ('counts', F8, (5, 2)),
                ('delta_roles', U1, (0,)), ('dims', I8, (3,)), ('elog_p', F8, (5, 2)),
                ('elog_r', F8, (1,)), ('flags', I8, (1,)), ('kind', U1, (3,)), ('l0', F8, (5, 1)),
                ('mask', U1, (50, 5)), ('scal', F8, (8,)), ('w', F8, (5, 1))],
    cmm=[('L', F8, (5, 21)), ('Nk', F8, (3,)), ('S', F8, (5, 21)), ('alpha_p', F8, (5, 21)),
         ('alpha_r', F8, (3,)), ('c', F8, (3,)), ('delta_roles', U1, (0,)), ('dims', I8, (4,)),
         ('elog_p', F8, (5, 21)), ('elog_r', F8, (3,)), ('flags', I8, (1,)), ('kind', U1, (3,)),
         ('mask', U1, (300, 7)), ('scal', F8, (8,))],
    dgmm=[('Nk', F8, (3,)), ('S1', F8, (3, 3)), ('S2', F8, (3, 3)), ('alpha_r', F8, (3,)),
          ('c', F8, (3,)), ('delta_roles', U1, (0,)), ('dims', I8, (3,)), ('elog_r', F8, (3,)),
          ('flags', I8, (1,)), ('h', F8, (3, 3)), ('kind', U1, (4,)), ('mu_mom', F8, (9, 2)),
          ('mu_par', F8, (9, 2)), ('q', F8, (3, 3)), ('scal', F8, (12,)), ('tau_mom', F8, (9, 2)),
          ('tau_par', F8, (9, 2))],
    dgmm_masked=[('M', F8, (3, 3)), ('Nk', F8, (3,)), ('S1', F8, (3, 3)), ('S2', F8, (3, 3)),
                 ('alpha_r', F8, (3,)), ('c', F8, (3,)), ('delta_roles', U1, (0,)),
                 ('dims', I8, (3,)), ('elog_r', F8, (3,)), ('flags', I8, (1,)), ('g', F8, (3, 3)),
                 ('h', F8, (3, 3)), ('kind', U1, (4,)), ('mask', U1, (70, 3)),
                 ('mu_mom', F8, (9, 2)), ('mu_par', F8, (9, 2)), ('q', F8, (3, 3)),
                 ('scal', F8, (12,)), ('tau_mom', F8, (9, 2)), ('tau_par', F8, (9, 2))],
    pmm=[('M', F8, (7, 3)), ('Nk', F8, (3,)), ('S', F8, (7, 3)), ('alpha_r', F8, (3,)),
         ('c', F8, (3,)), ('delta_roles', U1, (0,)), ('dims', I8, (3,)), ('elog_r', F8, (3,)),
         ('elog_r_used', F8, (3,)), ('flags', I8, (2,)), ('kind', U1, (3,)), ('l', F8, (7, 3)),
         ('lam_mom', F8, (21, 2)), ('lam_mom_used', F8, (21, 2)), ('lam_par', F8, (21, 2)),
         ('lb', F8, (7, 3)), ('mask', U1, (300, 7)), ('scal', F8, (8,))],
)


def _layout(block):
    _, _, _, models, run, case, _, _ = BLOCKS[block]
    run = getattr(importlib.import_module(models), run)
    Q = run(_mods(block), _inputs(block), only=(case,), n_iter=2)[case + '_plan']
    got = []
    Q.plans[0].save_state(lambda key, a: got.append((key, a.dtype.name, a.shape)), None, 0)
    assert all(key.startswith('plans/0/') for key, _, _ in got)
    return sorted((key[len('plans/0/'):], dt, shape) for key, dt, shape in got)


@pytest.mark.parametrize('block', sorted(BLOCKS))
def test_checkpoint_layout(block):
    assert _layout(block) == LAYOUT[block]


# -- the initial value of Z ------------------------------------------------------------------------
def _model(block, **zkw):
    """The model of the block at the size of its fixture, observed; ``zkw`` goes to ``Z``."""
    from bayespy_amd import nodes
    g = _inputs(block)
    family = block.split('_')[0]
    case = BLOCKS[block][5]
    key = '_y' if family == 'dgmm' else '_x'
    data = g.get(case + key, g['a' + key])          # a case without data of its own runs on (a)'s
    mask = g[case + '_mask'] if case + '_mask' in g else None
    N, D = data.shape
    K = 2
    W = nodes.Dirichlet(K * [1.0], name='alpha' if family == 'dgmm' else 'R')
    Z = nodes.Categorical(W, plates=(N, 1), name='Z', **zkw)
    if family == 'bmm':
        params = [nodes.Beta([0.5, 0.5], plates=(D, K), name='P')]
        X = nodes.Mixture(Z, nodes.Bernoulli, *params, name='X')
    elif family == 'dgmm':
        params = [nodes.GaussianARD(0.0, 1e-3, plates=(D, K), name='mu'),
                  nodes.Gamma(1e-2, 1e-2, plates=(D, K), name='tau')]
        X = nodes.Mixture(Z, nodes.GaussianARD, *params, name='Y')
    elif family == 'cmm':
        params = [nodes.Dirichlet((int(data.max()) + 1) * [0.5], plates=(D, K), name='P')]
        X = nodes.Mixture(Z, nodes.Categorical, *params, name='X')
    else:
        params = [nodes.Gamma(1e-2, 1e-3, plates=(D, K), name='lam')]
        X = nodes.Mixture(Z, nodes.Poisson, *params, name='X')
    if mask is None:
        X.observe(data)
    else:
        X.observe(np.where(mask, data, 0).astype(data.dtype), mask=mask)
    return Z, [X, Z] + params + [W]


def _bad_labels(which, N, K):
    if which == 'fraction':
        z = np.zeros((N, 1))
        z[N // 2] = 0.5
        return z, 'Values must be integers'
    if which == 'dtype':
        return np.zeros((N, 1), dtype=complex), 'Values must be integers'
    z = np.zeros((N, 1), dtype=np.int64)
    z[N - 1] = K
    return z, 'Invalid category index'


@pytest.mark.parametrize('which', ('fraction', 'dtype', 'index'))
@pytest.mark.parametrize('block', sorted(BLOCKS))
def test_labels_errors(block, which):
    from bayespy_amd.inference import VB
    Z, nodes = _model(block)
    z, text = _bad_labels(which, Z.plates[0], 2)
    Z.initialize_from_value(z)
    Q = VB(*nodes, engine='fused')
    _on_double(block)(Q)
    with pytest.raises(ValueError) as err:
        Q.plans[0]._materialize()
    assert str(err.value) == text


# -- a reason of a shared check --------------------------------------------------------------------
@pytest.mark.parametrize('block', sorted(BLOCKS))
def test_reason_of_a_shared_check_comes_from_the_family_alone(block):
    from bayespy_amd.inference.plans import compile_model
    family = block.split('_')[0]
    _, nodes = _model(block, plates_multiplier=(2.5, 1))
    why = []
    assert _plan_class(block).match(nodes, why) is None
    assert why == ['%s, observed node %s: plates_multiplier (mini-batches) goes through the '
                   'generic engine' % (LABELS[family], 'Y' if family == 'dgmm' else 'X')]
    with pytest.raises(NotImplementedError) as err:
        compile_model(nodes, engine='fused')
    said = str(err.value)
    assert said.count(why[0]) == 1
    assert [f for f in LABELS if LABELS[f] in said] == [family]
    assert all(n._plan is None for n in nodes)
