"""CPU: the fused latent-Dirichlet-allocation block with learnt concentrations without a device --
the g++ build of csrc/vmp_lda_hyper_dev.h against a long-double restatement of S and qterm, the
matcher of ``HyperLDAPlan`` / ``WideHyperLDAPlan`` and every declining reason, the engine values
(every old value keeps its answer), plan reuse, the plans' host logic on the kernel doubles of
tests/lda_hyper_host.py against the traces of tests/golden/lda_hyper.npz (live reference,
tools/make_golden_lda_hyper.py), checkpoints across the four LDA forms and the argument checks of
the host-only entry point."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

# what tests/test_hyperparameters_gpu.py holds the Concentration node to on the generic engine
BOUND_TOL = dict(rtol=1e-9, atol=0)
MOM_TOL = dict(rtol=1e-7, atol=1e-9)

CASES = ['topic', 'word', 'both', 'pair', 'first', 'k70']


def _on_double(Q):
    from bayespy_amd.device import Runtime
    from lda_hyper_host import CPUHyperLDAKernels, CPUWideHyperLDAKernels
    plan = Q.plans[0]
    rt = Runtime(device='cpu')
    kinds = {'HyperLDAPlan': CPUHyperLDAKernels, 'WideHyperLDAPlan': CPUWideHyperLDAKernels}
    plan._rt, plan._kernels = rt, kinds[type(plan).__name__](rt)


def _mods(after=_on_double, **kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments
    from lda_hyper_models import plan_params
    kw.setdefault('engine', 'fused+topics+hyper')
    m = dict(nodes=nodes, VB=VB, CategoricalMoments=CategoricalMoments, vb_kwargs=kw,
             params=plan_params)
    if after is not None:
        m['after_vb'] = after
    return m


def _golden():
    g = np.load(os.path.join(GOLDEN, 'lda_hyper.npz'))
    return g, {k[3:]: g[k] for k in g.files if k.startswith('in_')}


def _model(K=5, reg_topic=True, reg_word=False):
    from lda_hyper_models import build_hyper
    return build_hyper(_mods(), _golden()[1], K, reg_topic, reg_word)


def _nodes(m):
    from lda_hyper_models import model_nodes
    return model_nodes(m)


# -- the device header on the host ---------------------------------------------------------------------
def test_layout_functions():
    from lda_hyper_host import lda_hyper_host
    lib = lda_hyper_host()
    for W, R in ((1, 1), (64, 1), (65, 2), (128, 2), (129, 4), (256, 4), (257, 8), (513, 16),
                 (1024, 16)):
        assert lib.lda_hyper_regs(W) == R
    assert lib.lda_hyper_chunk_rows(1000) == 16 and lib.lda_hyper_chunk_rows(10 ** 9) == 256
    assert lib.lda_hyper_ws_doubles(33, 70) == 2 * (3 + 70) + 2 * 3 * 70


@pytest.mark.parametrize('cols', [1, 2, 63, 64, 65, 130, 1024])
def test_host_build_against_long_double_row_major(cols):
    """The rule of DESIGN.md 4.14 (8 x the float64 deviation from long double, floor 4 ulp) on S
    and qterm at every shape; the three figures are printed per shape (the worst ratios of error
    to allowance are recorded in DESIGN.md 4.13b)."""
    from lda_hyper_host import lda_hyper_host, host_stats, compare, make_tables
    T = lda_hyper_host().lda_hyper_chunk_rows(100)
    assert T == 16
    rs = np.random.RandomState(500 + cols)
    for rows in (0, 1, T - 1, T, T + 1, 3 * T + 5):
        for kind in ('plain', 'spread'):
            alpha, elog = make_tables(rs, rows, cols, kind)
            S, q = host_stats(alpha, elog, False)
            bad = compare(S, q, alpha, elog, label='rows %d cols %d %s' % (rows, cols, kind))
            assert not bad, (rows, cols, kind, bad)
            if rows == 0:
                assert not S.any() and q == 0.0


@pytest.mark.parametrize('rows', [1, 64, 65, 1024])
def test_host_build_against_long_double_transposed(rows):
    """The rule of DESIGN.md 4.14 (8 x the float64 deviation from long double, floor 4 ulp) on S
    and qterm at every shape; the three figures are printed per shape (the worst ratios of error
    to allowance are recorded in DESIGN.md 4.13b)."""
    from lda_hyper_host import host_stats, compare, make_tables
    rs = np.random.RandomState(600 + rows)
    for cols in (2, 15, 16, 17, 53):     # (one category is the exact zero of the row-major test)
        for kind in ('plain', 'spread'):
            alpha, elog = make_tables(rs, rows, cols, kind)
            S, q = host_stats(alpha, elog, True)
            bad = compare(S, q, alpha, elog, label='T rows %d cols %d %s' % (rows, cols, kind))
            assert not bad, (rows, cols, kind, bad)


def test_host_build_nan_and_repeat():
    from lda_hyper_host import host_stats, make_tables
    rs = np.random.RandomState(7)
    alpha, elog = make_tables(rs, 40, 70)
    for tr in (False, True):
        S, q = host_stats(alpha, elog, tr)
        S2, q2 = host_stats(alpha, elog, tr)
        assert np.array_equal(S, S2) and q == q2
        a = alpha.copy()
        a[17, 66] = np.nan
        S3, q3 = host_stats(a, elog, tr)
        assert np.isnan(q3) and np.array_equal(S3, S)
        e = elog.copy()
        e[17, 66] = np.nan
        S4, q4 = host_stats(alpha, e, tr)
        assert np.isnan(q4) and np.isnan(S4[66]) and np.isnan(S4).sum() == 1


# -- the matcher ------------------------------------------------------------------------------------
def _match(m, cls='HyperLDAPlan', nodes=None):
    from bayespy_amd.inference.plans import lda_hyper
    why = []
    return getattr(lda_hyper, cls).match(_nodes(m) if nodes is None else nodes, why), why


def test_matcher_accepts():
    for rt, rw in ((True, None), (None, False), (True, False), ((-6.0, 3.0), (-8.0, 2.0))):
        m = _model(5, rt, rw)
        r, why = _match(m)
        assert r is not None and why == []
        assert ('conc_topic' in r) == (rt is not None) and ('conc_word' in r) == (rw is not None)
    r, why = _match(_model(70, True, True), 'WideHyperLDAPlan')
    assert r is not None and why == [] and r['conc_word'].D == 30
    r, why = _match(_model(64), 'HyperLDAPlan')
    assert r is not None


def test_matcher_declines_with_reasons():
    from bayespy_amd import nodes
    from lda_hyper_models import D, V, N
    _, gin = _golden()
    docs, words = gin['docs'], gin['words']

    def reason(m, cls='HyperLDAPlan', nodes=None):
        r, why = _match(m, cls, nodes)
        assert r is None and len(why) == 1, why
        assert why[0].startswith('fused LDA block (concentrations)'), why
        return why[0]

    def build(a, b, K=5, plates=(N,), mult=None, idx=docs, data=words):
        p_topic = nodes.Dirichlet(a, plates=(D,), name='p_topic')
        p_word = nodes.Dirichlet(b, plates=(K,), name='p_word')
        kw = {} if mult is None else dict(plates_multiplier=mult)
        topics = nodes.Categorical(nodes.Gate(idx, p_topic), plates=plates, name='topics', **kw)
        w = nodes.Categorical(nodes.Gate(topics, p_word), name='words', **kw)
        w.observe(data)
        m = dict(words=w, topics=topics, p_word=p_word, p_topic=p_topic)
        for key, c in (('conc_topic', a), ('conc_word', b)):
            if isinstance(c, nodes.Concentration):
                m[key] = c
        return m
    assert 'use the LDA block' in reason(_model(5, None, None))
    assert 'exceeds the limit' in reason(_model(70))
    assert 'use the LDA block' in reason(_model(5), 'WideHyperLDAPlan')
    assert 'exceeds the limit' in reason(_model(1025, True, None), 'WideHyperLDAPlan')
    # a plated concentration
    c = nodes.Concentration(5, plates=(D,), name='c')
    assert 'has plates (12,)' in reason(build(c, np.ones(V)))
    # stochastic VI
    c = nodes.Concentration(5, name='c')
    assert 'stochastic VI with learnt concentrations is not built' in reason(
        build(c, np.ones(V), mult=(2.5,)))
    # a mask
    m = build(nodes.Concentration(5, name='c'), np.ones(V))
    m['words'].observe(words, mask=np.arange(N) % 2 == 0)
    assert 'mask' in reason(m)
    # sharded plates
    m = build(nodes.Concentration(5, name='c'), np.ones(V))
    m['topics'].shard(-1)
    assert 'sharded' in reason(m)
    # a concentration with another child
    c = nodes.Concentration(5, name='c')
    m = build(c, np.ones(V))
    other = nodes.Dirichlet(c, name='other')
    assert 'other children' in reason(m) and other is not None
    # an observed concentration (the node's own observe() refuses; the matcher reads the flag)
    m = build(nodes.Concentration(5, name='c'), np.ones(V))
    m['conc_topic'].observed = True
    assert 'is observed' in reason(m)
    # a concentration that is not among the nodes, one with an initial value
    m = build(nodes.Concentration(5, name='c'), np.ones(V))
    four = [m['words'], m['topics'], m['p_word'], m['p_topic']]
    assert 'not among the nodes' in reason(m, nodes=four)
    m = build(nodes.Concentration(5, name='c'), np.ones(V))
    m['conc_topic'].initialize_from_value(np.full(5, 2.0))
    assert 'initialised by value' in reason(m)
    # what the block itself declines keeps its reason under this label
    m = build(nodes.Concentration(5, name='c'), np.ones(V), plates=(20, 20),
              idx=docs.reshape(20, 20), data=words.reshape(20, 20))
    assert 'one token plate axis' in reason(m)
    m = build(nodes.Concentration(5, name='c'), np.ones(V))
    m['words'].unobserve()
    assert 'not observed' in reason(m)
    from bayespy_amd.inference import VB
    Q = VB(*_nodes(_model(5)), engine='fused+hyper')
    with pytest.raises(NotImplementedError, match=r'fused LDA block \(concentrations\).*gradient'):
        Q.gradient_step('p_topic', 'p_word', scale=0.5)


# -- engine values ------------------------------------------------------------------------------------
def test_engine_values(monkeypatch):
    from bayespy_amd.inference import VB, plans
    from bayespy_amd.inference.plans.generic import GenericPlan
    from bayespy_amd.inference.plans.lda import LDAPlan, LDASVIPlan
    from bayespy_amd.inference.plans.lda_wide import WideLDAPlan
    from bayespy_amd.inference.plans.lda_hyper import HyperLDAPlan, WideHyperLDAPlan
    assert plans.OPT_IN_HYPER == {LDAPlan: [HyperLDAPlan], WideLDAPlan: [WideHyperLDAPlan]}
    assert issubclass(HyperLDAPlan, LDAPlan) and issubclass(WideHyperLDAPlan, WideLDAPlan)
    assert HyperLDAPlan not in plans.PLAN_TYPES and WideHyperLDAPlan not in plans.PLAN_TYPES
    monkeypatch.delenv('BAYESPY_AMD_ENGINE', raising=False)

    def plan_of(K, engine, **kw):
        m = _model(K, **kw)
        return type(VB(*_nodes(m), engine=engine).plans[0])
    # the new values
    assert plan_of(5, 'fused+hyper') is HyperLDAPlan
    assert plan_of(5, 'fused+topics+hyper') is HyperLDAPlan
    assert plan_of(70, 'fused+topics+hyper') is WideHyperLDAPlan
    with pytest.raises(NotImplementedError, match=r'fused LDA block \(concentrations\), observed '
                                                  r'node words: n_topics = 70 exceeds') as ei:
        plan_of(70, 'fused+hyper')
    assert 'wide topics' not in str(ei.value)
    # constant concentrations stay with the existing forms under the new values
    const = dict(reg_topic=None, reg_word=None)
    assert plan_of(5, 'fused+hyper', **const) is LDASVIPlan
    assert plan_of(5, 'fused+topics+hyper', **const) is LDASVIPlan
    assert plan_of(70, 'fused+topics+hyper', **const) is WideLDAPlan
    # every old value keeps its answer for a model with a Concentration parent
    for K in (5, 70):
        for engine in ('fused', 'fused+batches', 'fused+batches+gaussian', 'fused+topics'):
            with pytest.raises(NotImplementedError, match=r'fused LDA block, observed node words: '
                                                          r'the concentration of p_topic is a node '
                                                          r'\(Concentration\), not a constant') as ei:
                plan_of(K, engine)
            assert '(concentrations)' not in str(ei.value)
        with pytest.warns(UserWarning, match='generic message-passing engine.*fused LDA block, '
                                             'observed node words: the concentration of p_topic'):
            assert issubclass(plan_of(K, None), GenericPlan)
        assert issubclass(plan_of(K, 'generic'), GenericPlan)
    # through the environment
    for value, K, want in (('fused+hyper', 5, HyperLDAPlan),
                           ('fused+topics+hyper', 70, WideHyperLDAPlan)):
        monkeypatch.setenv('BAYESPY_AMD_ENGINE', value)
        assert plan_of(K, None) is want
    monkeypatch.delenv('BAYESPY_AMD_ENGINE')


def test_plan_reuse_only_for_the_new_values(monkeypatch):
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.plans.generic import GenericPlan
    from bayespy_amd.inference.plans.lda_hyper import HyperLDAPlan
    monkeypatch.delenv('BAYESPY_AMD_ENGINE', raising=False)
    m = _model(5)
    plan = VB(*_nodes(m), engine='fused+hyper').plans[0]
    assert type(plan) is HyperLDAPlan
    assert VB(*_nodes(m), engine='fused+hyper').plans[0] is plan
    assert VB(*_nodes(m), engine='fused+topics+hyper').plans[0] is plan
    for engine in ('fused', 'fused+topics', 'fused+batches'):
        with pytest.raises(NotImplementedError, match='not a constant'):
            VB(*_nodes(m), engine=engine)
    m = _model(5)
    VB(*_nodes(m), engine='fused+hyper')
    with pytest.warns(UserWarning, match='generic message-passing engine'):
        Q2 = VB(*_nodes(m))
    assert isinstance(Q2.plans[0], GenericPlan)


# -- the plans on the kernel doubles --------------------------------------------------------------------
def _check_trace(res, g, tag, bound_tol=BOUND_TOL, mom_tol=MOM_TOL, out=print):
    from lda_hyper_models import SWEEPS
    checked = 0
    for k, v in res.items():
        if k.endswith(('_plan', '_model')):
            continue
        want = g[k]
        assert np.shape(v) == want.shape, k
        tol = bound_tol if (k.endswith('_L') or '_l_' in k) else mom_tol
        with np.errstate(all='ignore'):
            dev = np.max(np.abs(v - want) / np.maximum(np.abs(want), 1e-300)) if want.size else 0.0
        out('%-28s largest relative deviation %.3e' % (k, dev))
        if k.endswith('_L') or '_l_' in k:
            assert want.shape[0] == SWEEPS
        np.testing.assert_allclose(v, want, err_msg=k, **tol)
        checked += 1
    return checked


def test_fixture_holds_the_initial_value_of_the_reference():
    g, _ = _golden()
    for tag in CASES:
        for key, cols in (('conc_topic', None), ('conc_word', 30)):
            k0 = '%s_%s_init_u0' % (tag, key)
            if k0 in g.files:
                a = g[k0]
                assert np.all(a == 1.0)
                from scipy import special
                np.testing.assert_allclose(g[k0[:-1] + '1'], special.gammaln(a.size), rtol=1e-15)


@pytest.mark.parametrize('tag', CASES)
def test_plan_reproduces_the_fixture_trace_on_the_kernel_double(tag):
    from lda_hyper_models import run_hyper_case, HYPER_CASES, SWEEPS
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_hyper_case(_mods(), gin, tag)
    n_conc = sum(r is not None for r in HYPER_CASES[tag][1:3])
    assert _check_trace(res, g, tag) == 1 + 4 + 2 + 5 * n_conc
    plan = res[tag + '_plan'].plans[0]
    calls = plan.kernels.calls
    assert type(plan).__name__ == ('WideHyperLDAPlan' if HYPER_CASES[tag][0] > 64
                                   else 'HyperLDAPlan')
    # per sweep and concentration: one update, one fill, and ONE pass per state of the table (after
    # the Dirichlet's update; the concentration's update and the bound share it)
    assert calls.count('ml_concentration') == SWEEPS * n_conc
    assert calls.count('prior_fill') == SWEEPS * n_conc
    first = HYPER_CASES[tag][3]
    assert calls.count('stats') == SWEEPS * n_conc + (n_conc if first else 0)
    # asking again runs nothing
    before = len(calls)
    res[tag + '_plan'].compute_lowerbound()
    assert len(calls) == before


def test_bound_is_right_after_either_update_and_regularization_setter():
    """The Dirichlet's term under the present prior, after a Dirichlet update and after a
    concentration update, against the NumPy evaluation from the plan's tables; the regularization
    setter changes the concentration's term only and keeps every table."""
    from scipy import special
    from lda_hyper_models import run_hyper_case
    _, gin = _golden()
    res = run_hyper_case(_mods(), gin, 'both', sweeps=2)
    Q, m = res['both_plan'], res['both_model']
    plan = Q.plans[0]

    def z(a):
        return special.gammaln(a.sum(-1)) - special.gammaln(a).sum(-1)

    def terms():
        out = {}
        for key, al, el in (('conc_topic', plan.alpha_theta.numpy(), plan.elog_theta.numpy()),
                            ('conc_word', plan.alpha_beta_t.numpy().T, plan.elog_beta_t.numpy().T)):
            a = m[key].get_moments()[0]
            out[key] = float(np.sum(z(a) - z(al) + ((a - al) * el).sum(-1)))
        return out
    for node in ('conc_topic', 'p_topic', 'p_word', 'conc_word', 'topics', 'p_topic'):
        Q.update(node, verbose=False)
        want = terms()
        np.testing.assert_allclose(m['p_topic'].lower_bound_contribution(), want['conc_topic'],
                                   rtol=1e-10, atol=1e-9)
        np.testing.assert_allclose(m['p_word'].lower_bound_contribution(), want['conc_word'],
                                   rtol=1e-10, atol=1e-9)
    calls = plan.kernels.calls
    n = len(calls)
    t_before = m['p_topic'].lower_bound_contribution()
    a_before = m['conc_topic'].get_moments()[0].copy()
    m['conc_topic'].regularization = (-7.0, 4.0)
    a, zz = m['conc_topic'].get_moments()
    assert np.array_equal(a, a_before)
    np.testing.assert_allclose(m['conc_topic'].lower_bound_contribution(),
                               float(np.sum(a * -7.0) + zz * 4.0), rtol=1e-13)
    assert m['p_topic'].lower_bound_contribution() == t_before
    assert [c for c in calls[n:] if c != 'dot'] == []       # no pass, no update, no fill
    Q.update('conc_topic', verbose=False)
    assert not np.array_equal(m['conc_topic'].get_moments()[0], a_before)
    assert [c for c in calls[n:] if c != 'dot'] == ['ml_concentration', 'prior_fill']
    with pytest.raises(NotImplementedError, match='maximum-likelihood node has no distribution'):
        m['conc_topic'].get_parameters()
    np.testing.assert_array_equal(m['p_word'].get_parameters()[0], plan.alpha_beta_t.numpy().T)


def test_random_initialisation_draws_from_the_prior_at_set_up():
    from bayespy_amd.inference import VB
    m = _model(5, True, True)
    np.random.seed(3)
    m['p_topic'].initialize_from_random()
    m['p_word'].initialize_from_random()
    Q = VB(*_nodes(m), engine='fused+hyper')
    _on_double(Q)
    Q.ignore_bound_checks = True
    plan = Q.plans[0]
    assert m['p_topic'].lower_bound_contribution() == -np.inf      # (builds the state)
    np.random.seed(3)
    x = np.random.gamma(np.ones((12, 5)))
    np.testing.assert_allclose(plan.elog_theta.numpy(), np.log(x / x.sum(-1, keepdims=True)))
    Q.update(repeat=3, verbose=False)
    L = Q.L[:3]
    assert np.all(np.isfinite(L)) and np.all(np.diff(L) > -1e-8), L


def test_checkpoints_across_the_four_forms(tmp_path):
    from lda_hyper_models import run_hyper_case
    from lda_host import CPULDAKernels
    from lda_wide_host import CPUWideLDAKernels
    from bayespy_amd.device import Runtime
    from bayespy_amd.inference import VB
    _, gin = _golden()
    res = run_hyper_case(_mods(), gin, 'both')
    Q = res['both_plan']
    fn = str(tmp_path / 'lda_hyper.ckpt')
    Q.save(filename=fn)
    L4 = Q.L[:4].copy()
    Q.update(repeat=2, verbose=False)
    L6 = Q.L[:6].copy()
    a6 = res['both_model']['conc_topic'].get_moments()[0].copy()
    Q.load(filename=fn)
    assert Q.iter == 4
    np.testing.assert_array_equal(Q.L[:4], L4)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:6], L6)
    np.testing.assert_array_equal(res['both_model']['conc_topic'].get_moments()[0], a6)
    # the other three forms
    Qw = run_hyper_case(_mods(), gin, 'k70', sweeps=1)['k70_plan']
    fnw = str(tmp_path / 'lda_wide_hyper.ckpt')
    Qw.save(filename=fnw)
    with pytest.raises(Exception, match=r"holds the state of the fused LDA block with learnt "
                                        r"concentrations \(engine='fused\+hyper'"):
        Qw.load(filename=fn)
    with pytest.raises(Exception, match=r"holds the state of the wide-topic form of the fused LDA "
                                        r"block with learnt concentrations"):
        Q.load(filename=fnw)
    rt = Runtime(device='cpu')
    Qn = VB(*_nodes(_model(5, None, None)))
    Qn.plans[0]._rt, Qn.plans[0]._kernels = rt, CPULDAKernels(rt)
    assert type(Qn.plans[0]).__name__ == 'LDAPlan'
    with pytest.raises(Exception, match=r"holds the state of the fused LDA block with learnt"):
        Qn.load(filename=fn)
    Qn.update(repeat=1, verbose=False)
    fnn = str(tmp_path / 'lda.ckpt')
    Qn.save(filename=fnn)
    with pytest.raises(Exception, match=r"holds the state of the fused LDA block \(K <= 64\)"):
        Q.load(filename=fnn)
    Qt = VB(*_nodes(_model(70, None, None)), engine='fused+topics')
    Qt.plans[0]._rt, Qt.plans[0]._kernels = rt, CPUWideLDAKernels(rt)
    with pytest.raises(Exception, match=r"holds the state of the wide-topic form of the fused LDA "
                                        r"block with learnt"):
        Qt.load(filename=fnw)
    Qt.update(repeat=1, verbose=False)
    fnt = str(tmp_path / 'lda_wide.ckpt')
    Qt.save(filename=fnt)
    with pytest.raises(Exception, match=r"holds the state of the wide-topic form of the fused LDA "
                                        r"block \(engine='fused\+topics'"):
        Qw.load(filename=fnt)
    # a file of the same form that learns another concentration
    Q1 = run_hyper_case(_mods(), gin, 'topic', sweeps=1)['topic_plan']
    fn1 = str(tmp_path / 'lda_hyper_topic.ckpt')
    Q1.save(filename=fn1)
    tables = [Q.plans[0].alpha_theta.numpy().copy(), Q.plans[0].elog_beta_t.numpy().copy()]
    with pytest.raises(Exception, match='holds the learnt concentrations of p_topic, this model '
                                        'learns p_topic, p_word'):
        Q.load(filename=fn1)
    # ... and the other way round; a refused load leaves the state as it was
    with pytest.raises(Exception, match='holds the learnt concentrations of p_topic, p_word, this '
                                        'model learns p_topic'):
        Q1.load(filename=fn)
    np.testing.assert_array_equal(Q.plans[0].alpha_theta.numpy(), tables[0])
    np.testing.assert_array_equal(Q.plans[0].elog_beta_t.numpy(), tables[1])


# -- the C ABI where the library loads without a device --------------------------------------------------
def test_cabi_declares_the_entry_points():
    from bayespy_amd import _lib
    from lda_hyper_host import lda_hyper_host
    lib = _lib.load()
    for name in ('vmp_lda_concentration_stats', 'vmp_lda_concentration_stats_workspace',
                 'vmp_lda_prior_fill'):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    host = lda_hyper_host()
    w = ctypes.c_int64()
    for rows, cols in ((1, 1), (1000, 70), (10 ** 6, 1024), (33, 5)):
        assert lib.vmp_lda_concentration_stats_workspace(rows, cols, cols, 1,
                                                         ctypes.byref(w)) == _lib.VMP_OK
        assert w.value == host.lda_hyper_ws_doubles(rows, cols)
    for rows, cols in ((5, 20000), (1024, 30), (64, 1)):
        assert lib.vmp_lda_concentration_stats_workspace(rows, cols, 1, rows,
                                                         ctypes.byref(w)) == _lib.VMP_OK
        assert w.value == host.lda_hyper_ws_doubles(cols, rows)
    assert lib.vmp_lda_concentration_stats_workspace(0, 7, 7, 1, ctypes.byref(w)) == _lib.VMP_OK
    for args in ((10, 1025, 1025, 1), (1025, 30, 1, 1025), (10, 7, 8, 1), (10, 7, 2, 20)):
        assert lib.vmp_lda_concentration_stats_workspace(*args, ctypes.byref(w)) \
            == _lib.VMP_ERR_UNSUPPORTED, args
    for args in ((-1, 7, 7, 1), (10, 0, 1, 1), (10, 7, 0, 1), (10, 7, 7, -1)):
        assert lib.vmp_lda_concentration_stats_workspace(*args, ctypes.byref(w)) \
            == _lib.VMP_ERR_INVALID, args
    assert lib.vmp_lda_concentration_stats_workspace(10, 7, 7, 1, None) == _lib.VMP_ERR_INVALID
