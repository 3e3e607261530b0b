"""CPU: the wide-topic form of the fused latent-Dirichlet-allocation block (65 <= K <= 1024) without
a device -- the g++ build of csrc/vmp_lda_wide_dev.h against a long-double restatement, the matcher
of ``WideLDAPlan`` and its declining reasons, the engine values, plan reuse, the plan's host logic
on the kernel double tests/lda_wide_host.py (CPUWideLDAKernels) against both traces of
tests/golden/lda_wide.npz (live reference, tools/make_golden_lda_wide.py), a save / load round trip
and the argument checks of the host-only entry points."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

TRACE_TOL = dict(rtol=1e-8, atol=1e-8)       # bounds: the scalar rule of the golden comparisons
MOM_TOL = dict(rtol=1e-7, atol=1e-9)         # parameters: the moment rule of tests/test_lda_host.py
U = 2.0 ** -53


def _on_double(Q):
    from bayespy_amd.device import Runtime
    from lda_wide_host import CPUWideLDAKernels
    plan = Q.plans[0]
    assert type(plan).__name__ == 'WideLDAPlan'
    rt = Runtime(device='cpu')
    plan._rt, plan._kernels = rt, CPUWideLDAKernels(rt)


def _mods(after=_on_double, **kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments
    from lda_wide_models import plan_params
    kw.setdefault('engine', 'fused+topics')
    m = dict(nodes=nodes, VB=VB, CategoricalMoments=CategoricalMoments, vb_kwargs=kw,
             params=plan_params)
    if after is not None:
        m['after_vb'] = after
    return m


def _golden():
    g = np.load(os.path.join(GOLDEN, 'lda_wide.npz'))
    return g, {k[3:]: g[k] for k in g.files if k.startswith('in_')}


def _model(K=70, **kw):
    from lda_models import build_lda
    _, gin = _golden()
    return build_lda(_mods(), gin['docs'], gin['words'], 7, 30, K, **kw)


def _four(m):
    return [m['words'], m['topics'], m['p_word'], m['p_topic']]


# -- the device header on the host ---------------------------------------------------------------------
def test_layout_functions():
    from lda_wide_host import lda_wide_host
    from lda_host import lda_host
    lib = lda_wide_host()
    for K, R in ((65, 2), (128, 2), (129, 4), (256, 4), (257, 8), (512, 8), (513, 16),
                 (1000, 16), (1024, 16)):
        assert lib.lda_wide_regs(K) == R and 64 * R >= K and (R == 2 or 32 * R < K)
    for n in (0, 1, 1000, 10 ** 5, 10 ** 6, 2 * 10 ** 6, 10 ** 7, 2 ** 31 - 1):
        T = lib.lda_wide_chunk_tokens(n)
        assert T == lda_host().lda_chunk_tokens(n, 64) and T in (16, 32, 64, 128, 256)
    assert lib.lda_wide_chunk_tokens(1000) == 16 and lib.lda_wide_chunk_tokens(10 ** 9) == 256


def _tables(rs, K, D, V, kind):
    et = np.log(rs.dirichlet(np.ones(K), size=D))
    ebt = np.log(rs.dirichlet(np.ones(V), size=K)).T
    if kind == 'inf':                   # columns of -inf in both tables, one in the last register
        et[:, [1, 64, K - 1]] = -np.inf
        ebt[:, [0, 66 % K, K - 2]] = -np.inf
    if kind == 'far':                   # rows hundreds of nats apart, and far apart inside a row
        et += rs.uniform(-150.0, 150.0, size=(D, 1))
        ebt += rs.uniform(-150.0, 150.0, size=(V, 1))
        et[:, ::7] -= 120.0
    return et, ebt


@pytest.mark.parametrize('K', [65, 127, 128, 129, 1000, 1024])
def test_host_build_of_the_device_header_against_long_double(K):
    """The bound of tests/test_lda_host.py, u = 2^-53: a responsibility exp(l - lse) is
    relative-exact to c u, c = 4 + 4 (lmax + log K), a count adds `len` positive terms in order:
    |error| <= (len + c) u * count; lse within 4 u (lmax + log K + 1).  That derivation allows 2 u
    for the log and the sum under it; the wide sum adds K positive terms in at most (R - 1) + 6 <= 21
    additions per path (in lane, then six butterfly levels), 21 u relative in s and so absolute in
    log s.  The rule covers it: these tables are logs of normalised rows, so lmax >= log K and
    4 (lmax + log K) >= 8 log 65 > 33."""
    from lda_wide_host import lda_wide_host, host_token_pass
    from lda_host import make_layouts, restate
    rs = np.random.RandomState(100 + K)
    D, V = 6, 11
    T = lda_wide_host().lda_wide_chunk_tokens(1000)
    assert T == 16
    for kind in ('plain', 'inf', 'far'):
        for n in (0, 1, T - 1, T, T + 1, 5 * T + 3):
            doc = np.sort(rs.randint(D, size=n)) if n != 5 * T + 3 else np.zeros(n, dtype=np.int64)
            word = rs.randint(V, size=n)
            et, ebt = _tables(rs, K, D, V, kind)
            lay, orig = make_layouts(doc, word, D, V)
            Ndk, Nvk, scal, lse, phi = host_token_pass(n, D, V, K, lay, None, et, ebt, orig=orig,
                                                       want_phi=True)
            rphi, rlse, rN, rM = restate(doc, word, D, V, K, et, ebt)
            lmax = float(np.abs(et[np.isfinite(et)]).max() + np.abs(ebt[np.isfinite(ebt)]).max())
            assert lmax >= np.log(K)
            c = 4 + 4 * (lmax + np.log(K))
            bound = (max(n, 1) + c) * U
            assert np.all(np.isfinite(Ndk)) and np.all(np.isfinite(Nvk)), (K, n, kind)
            assert np.all(np.abs(Ndk - rN) <= bound * np.maximum(rN, 0)), (K, n, kind)
            assert np.all(np.abs(Nvk - rM) <= bound * np.maximum(rM, 0)), (K, n, kind)
            if kind == 'inf':
                assert not Ndk[:, [1, 64, K - 1]].any() and not Nvk[:, [0, 66 % K, K - 2]].any()
            if n:
                np.testing.assert_allclose(phi, rphi.astype(np.float64), rtol=c * U, atol=0)
                np.testing.assert_allclose(lse, rlse.astype(np.float64)[orig], rtol=0,
                                           atol=4 * U * (lmax + np.log(K) + 1))
            adds = T + n / T + 1
            np.testing.assert_allclose(scal[0], float(rlse.sum()), rtol=0,
                                       atol=n * 4 * U * (lmax + np.log(K) + 1)
                                       + adds * U * float(np.abs(rlse).sum()))
            np.testing.assert_allclose(Ndk.sum(0), Nvk.sum(0), rtol=1e-12, atol=1e-300)


def test_host_build_edge_cases():
    from lda_wide_host import host_token_pass
    from lda_host import make_layouts
    K, D, V = 130, 4, 5
    et = np.log(np.full((D, K), 1.0 / K))
    ebt = np.log(np.full((V, K), 1.0 / V))
    lay, _ = make_layouts([], [], D, V)
    Ndk, Nvk, scal, _, _ = host_token_pass(0, D, V, K, lay, None, et, ebt)
    assert not Ndk.any() and not Nvk.any() and scal[0] == 0
    # empty documents and unused words are exact zeros; one document holds every token
    doc, word = np.full(100, 2), np.arange(100) % 2
    lay, orig = make_layouts(doc, word, D, V)
    Ndk, Nvk, _, _, _ = host_token_pass(100, D, V, K, lay, None, et, ebt)
    assert not Ndk[[0, 1, 3]].any() and not Nvk[2:].any()
    np.testing.assert_allclose(Ndk[2], 100.0 / K, rtol=1e-13)
    # fixed labels, some of them >= 64: one-hot counts, lse = 0
    lab = ((np.arange(100) * 37) % K).astype(np.int32)
    assert (lab >= 64).any() and (lab < 64).any()
    Ndk, Nvk, scal, lse, phi = host_token_pass(100, D, V, K, lay, lab, et, ebt, orig=orig,
                                               want_phi=True)
    np.testing.assert_array_equal(Ndk[2], np.bincount(lab, minlength=K))
    np.testing.assert_array_equal(phi[orig], np.eye(K)[lab])
    assert scal[0] == 0 and not lse.any()
    # prior only
    Ndk, Nvk, scal, lse, phi = host_token_pass(100, D, V, K, lay, None, et, None, orig=orig,
                                               want_phi=True)
    np.testing.assert_allclose(phi, 1.0 / K, rtol=1e-14)
    assert scal[2] == 0
    # a token whose logits are all -inf: NaN in its outputs and in nothing else
    ebt2 = ebt.copy()
    ebt2[1] = -np.inf
    doc, word = np.array([0, 0, 1, 3]), np.array([0, 1, 0, 2])
    lay, orig = make_layouts(doc, word, D, V)
    Ndk, Nvk, scal, lse, phi = host_token_pass(4, D, V, K, lay, None, et, ebt2, orig=orig,
                                               want_phi=True)
    assert np.isnan(phi[1]).all() and np.isfinite(phi[[0, 2, 3]]).all()
    assert np.isnan(lse[list(orig).index(1)]) and np.isnan(lse).sum() == 1
    assert np.isnan(Ndk[0]).all() and np.isfinite(Ndk[[1, 2, 3]]).all()
    assert np.isnan(Nvk[1]).all() and np.isfinite(Nvk[[0, 2, 3, 4]]).all()


# -- the matcher ------------------------------------------------------------------------------------
def _match(m, extra=()):
    from bayespy_amd.inference.plans.lda_wide import WideLDAPlan
    why = []
    return WideLDAPlan.match(_four(m) + list(extra), why), why


def test_matcher_accepts_65_to_1024_topics():
    for K in (65, 70, 1024):
        r, why = _match(_model(K))
        assert r is not None and why == []
    m = _model(130, index_constant=True)
    r, why = _match(m, [m['idx']])
    assert r is not None and why == [] and r['document_indices'] is m['idx']


def test_matcher_declines_with_reasons():
    from bayespy_amd import nodes
    _, gin = _golden()
    docs, words = gin['docs'], gin['words']
    n, K = len(words), 70

    def reason(m):
        r, why = _match(m)
        assert r is None and len(why) == 1, why
        assert why[0].startswith('fused LDA block (wide topics)'), why
        return why[0]
    assert 'use the LDA block' in reason(_model(64))
    assert 'use the LDA block' in reason(_model(4))
    assert 'exceeds the limit' in reason(_model(1025))
    m = _model(K)
    m['words'].observe(words, mask=np.arange(n) % 2 == 0)
    assert 'mask' in reason(m)
    c = nodes.Concentration(K, name='c')
    p_topic = nodes.Dirichlet(c, plates=(7,), name='p_topic')
    p_word = nodes.Dirichlet(np.ones(30), plates=(K,), name='p_word')
    topics = nodes.Categorical(nodes.Gate(docs, p_topic), plates=(n,), name='topics')
    w = nodes.Categorical(nodes.Gate(topics, p_word), name='words')
    w.observe(words)
    assert 'Concentration' in reason(dict(words=w, topics=topics, p_word=p_word, p_topic=p_topic))
    p_topic = nodes.Dirichlet(np.ones(K), plates=(7,), name='p_topic')
    p_word = nodes.Dirichlet(np.ones(30), plates=(K,), name='p_word')
    topics = nodes.Categorical(nodes.Gate(docs.reshape(20, 20), p_topic), plates=(20, 20),
                               name='topics')
    w = nodes.Categorical(nodes.Gate(topics, p_word), name='words')
    w.observe(words.reshape(20, 20))
    assert 'one token plate axis' in reason(dict(words=w, topics=topics, p_word=p_word,
                                                 p_topic=p_topic))
    m = _model(K)
    m['topics'].shard(-1)
    assert 'sharded' in reason(m)
    # mini-batches: declined, and gradient_step on a plan of this class says why
    p_topic = nodes.Dirichlet(np.ones(K), plates=(7,), name='p_topic')
    p_word = nodes.Dirichlet(np.ones(30), plates=(K,), name='p_word')
    topics = nodes.Categorical(nodes.Gate(docs, p_topic), plates=(n,), plates_multiplier=(2.5,),
                               name='topics')
    w = nodes.Categorical(nodes.Gate(topics, p_word), plates_multiplier=(2.5,), name='words')
    w.observe(words)
    assert 'plates_multiplier' in reason(dict(words=w, topics=topics, p_word=p_word,
                                              p_topic=p_topic))
    from bayespy_amd.inference import VB
    Q = VB(*_four(_model(K)), engine='fused+topics')
    with pytest.raises(NotImplementedError, match=r'fused LDA block \(wide topics\).*gradient'):
        Q.gradient_step('p_topic', 'p_word', scale=0.5)


# -- engine values ------------------------------------------------------------------------------------
def test_engine_values(monkeypatch):
    from bayespy_amd import inference, nodes
    from bayespy_amd.inference import VB, plans
    from bayespy_amd.inference.plans.generic import GenericPlan
    from bayespy_amd.inference.plans.lda import LDAPlan, LDASVIPlan
    from bayespy_amd.inference.plans.lda_wide import WideLDAPlan
    assert plans.OPT_IN_TOPICS == {LDAPlan: [WideLDAPlan]}
    assert issubclass(WideLDAPlan, LDAPlan) and WideLDAPlan not in plans.PLAN_TYPES
    monkeypatch.delenv('BAYESPY_AMD_ENGINE', raising=False)
    # the new value: K = 65 goes to the wide form, K = 64 stays with the LDA block
    assert type(VB(*_four(_model(65)), engine='fused+topics').plans[0]) is WideLDAPlan
    assert type(VB(*_four(_model(64)), engine='fused+topics').plans[0]) is LDASVIPlan
    assert type(VB(*_four(_model(64)), engine='fused').plans[0]) is LDASVIPlan
    assert type(VB(*_four(_model(64))).plans[0]) is LDAPlan
    # every other value keeps its answer for K = 65
    for engine in ('fused', 'fused+batches', 'fused+batches+gaussian'):
        with pytest.raises(NotImplementedError, match=r'fused LDA block, observed node words: '
                                                      r'n_topics = 65 exceeds the limit') as ei:
            VB(*_four(_model(65)), engine=engine)
        assert 'wide topics' not in str(ei.value)
    with pytest.warns(UserWarning, match='generic message-passing engine.*fused LDA block, '
                                         'observed node words: n_topics = 65 exceeds the limit'):
        Q = VB(*_four(_model(65)))
    assert isinstance(Q.plans[0], GenericPlan)
    assert isinstance(VB(*_four(_model(65)), engine='generic').plans[0], GenericPlan)
    # through the environment
    monkeypatch.setenv('BAYESPY_AMD_ENGINE', 'fused+topics')
    assert type(VB(*_four(_model(65))).plans[0]) is WideLDAPlan
    monkeypatch.delenv('BAYESPY_AMD_ENGINE')
    # what no form takes is declined by both, each with its own label
    with pytest.raises(NotImplementedError) as ei:
        VB(*_four(_model(1025)), engine='fused+topics')
    assert 'fused LDA block (wide topics), observed node words: n_topics = 1025 exceeds' \
        in str(ei.value) and 'fused LDA block, observed node words' in str(ei.value)
    assert inference is not None and nodes is not None


def test_plan_reuse_only_for_the_new_value(monkeypatch):
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.plans.generic import GenericPlan
    from bayespy_amd.inference.plans.lda_wide import WideLDAPlan
    monkeypatch.delenv('BAYESPY_AMD_ENGINE', raising=False)
    m = _model(70)
    Q = VB(*_four(m), engine='fused+topics')
    plan = Q.plans[0]
    assert type(plan) is WideLDAPlan
    assert VB(*_four(m), engine='fused+topics').plans[0] is plan
    for engine in ('fused', 'fused+batches'):
        with pytest.raises(NotImplementedError, match='exceeds the limit'):
            VB(*_four(m), engine=engine)
    m = _model(70)
    Q = VB(*_four(m), engine='fused+topics')
    with pytest.warns(UserWarning, match='generic message-passing engine'):
        Q2 = VB(*_four(m))
    assert isinstance(Q2.plans[0], GenericPlan)


# -- the plan on the kernel double ---------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['k70', 'k130'])
def test_plan_reproduces_the_fixture_trace_on_the_kernel_double(tag):
    from lda_wide_models import run_wide_case, SWEEPS
    from lda_host import restate
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_wide_case(_mods(), gin, tag)
    checked = 0
    for k, v in res.items():
        if k.endswith(('_plan', '_model')):
            continue
        assert v.shape == g[k].shape and v.shape[0] == SWEEPS
        np.testing.assert_allclose(v, g[k], err_msg=k,
                                   **(MOM_TOL if '_alpha_' in k else TRACE_TOL))
        checked += 1
    assert checked == 1 + 4 + 2
    Q, m = res[tag + '_plan'], res[tag + '_model']
    plan = Q.plans[0]
    calls = plan.kernels.calls
    assert 'token_pass_phi' not in calls and calls.count('token_pass') == 1 + SWEEPS
    # topics.get_moments(): formed on request from the tables of the last topics update
    K = plan.K
    phi = m['topics'].get_moments()[0]
    assert phi.shape == (400, K) and calls.count('token_pass_phi') == 1
    rphi = restate(gin['docs'], gin['words'], 7, 30, K, plan.used_theta.numpy(),
                   plan.used_beta_t.numpy())[0]
    np.testing.assert_allclose(phi, rphi.astype(np.float64), rtol=1e-12)
    with pytest.raises(NotImplementedError, match='never forms'):
        m['words'].get_moments()
    # the empty document and the unused words keep their prior
    from lda_wide_models import EMPTY_DOC, EMPTY_WORDS
    assert np.all(res[tag + '_alpha_topic'][:, EMPTY_DOC] == 1.0)
    assert np.all(res[tag + '_alpha_word'][:, :, list(EMPTY_WORDS)] == 1.0)


def test_initialisations_on_the_double():
    """Random and prior initialisation of the Dirichlets and fixed labels (some >= 64): the bound
    is finite and rises, the first counts under fixed labels are the label counts."""
    from bayespy_amd.inference import VB
    _, gin = _golden()
    K = 70
    for how in ('random', 'prior', 'labels'):
        m = _model(K)
        if how == 'random':
            np.random.seed(5)
            m['p_topic'].initialize_from_random()
            m['p_word'].initialize_from_random()
        lab = (np.arange(400) * 13) % K
        if how == 'labels':
            m['topics'].initialize_from_value(lab)
        Q = VB(*_four(m), engine='fused+topics')
        _on_double(Q)
        Q.ignore_bound_checks = True
        if how == 'labels':
            Q.update('p_topic', 'p_word', verbose=False)
            plan = Q.plans[0]
            want = np.zeros((7, K))
            np.add.at(want, (gin['docs'], lab), 1.0)
            np.testing.assert_array_equal(plan.Ndk.numpy(), want)
            np.testing.assert_array_equal(m['topics'].get_moments()[0], np.eye(K)[lab])
        Q.update(repeat=4, verbose=False)
        L = Q.L[:Q.iter]
        assert np.all(np.isfinite(L[-3:])) and np.all(np.diff(L[-3:]) > -1e-8), (how, L)


def test_save_load_round_trip_on_the_double(tmp_path):
    from lda_wide_models import run_wide_case
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.plans.lda import LDAPlan
    _, gin = _golden()
    res = run_wide_case(_mods(), gin, 'k70')
    Q = res['k70_plan']
    fn = str(tmp_path / 'lda_wide.ckpt')
    Q.save(filename=fn)
    L5 = Q.L[:5].copy()
    Q.update(repeat=2, verbose=False)
    L7 = Q.L[:7].copy()
    Q.load(filename=fn)
    assert Q.iter == 5
    np.testing.assert_array_equal(Q.L[:5], L5)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:7], L7)
    # the checkpoint names the wide form: a narrow plan does not take it, and the other way round
    from lda_host import CPULDAKernels
    from bayespy_amd.device import Runtime
    Qn = VB(*_four(_model(4)))
    assert type(Qn.plans[0]) is LDAPlan
    rt = Runtime(device='cpu')
    Qn.plans[0]._rt, Qn.plans[0]._kernels = rt, CPULDAKernels(rt)
    with pytest.raises(Exception, match=r"holds the state of the wide-topic form.*fused\+topics"):
        Qn.load(filename=fn)
    fn2 = str(tmp_path / 'lda.ckpt')
    Qn.update(repeat=1, verbose=False)
    Qn.save(filename=fn2)
    with pytest.raises(Exception, match=r"holds the state of the fused LDA block \(K <= 64\)"):
        Q.load(filename=fn2)
    # another K of the same form is told apart by the sizes
    Q130 = VB(*_four(_model(130)), engine='fused+topics')
    _on_double(Q130)
    with pytest.raises(ValueError, match='checkpoint is for'):
        Q130.load(filename=fn)


# -- the C ABI where the library loads without a device --------------------------------------------------
def test_cabi_declares_the_wide_entry_points():
    from bayespy_amd import _lib
    from bayespy_amd.inference.plans import lda_wide
    from lda_wide_host import lda_wide_host
    lib = _lib.load()
    for name in ('vmp_lda_wide_limits', 'vmp_lda_wide_plan', 'vmp_lda_wide_token_pass'):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES['vmp_lda_wide_token_pass'] == _lib.SIGNATURES['vmp_lda_token_pass']
    lo, hi, mc = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert lib.vmp_lda_wide_limits(ctypes.byref(lo), ctypes.byref(hi),
                                   ctypes.byref(mc)) == _lib.VMP_OK
    assert (lo.value, hi.value, mc.value) == (65, 1024, 256)
    assert (lda_wide.LDA_WIDE_MIN_K, lda_wide.LDA_WIDE_MAX_K) == (65, 1024)
    assert lib.vmp_lda_wide_limits(None, ctypes.byref(hi), ctypes.byref(mc)) == _lib.VMP_ERR_INVALID
    # the narrow limits are what they were
    mk = ctypes.c_int32()
    assert lib.vmp_lda_limits(ctypes.byref(mk), ctypes.byref(mc)) == _lib.VMP_OK and mk.value == 64
    r, c, w = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    refs = (ctypes.byref(r), ctypes.byref(c), ctypes.byref(w))
    host = lda_wide_host()
    for n, K in ((0, 65), (1000, 70), (10 ** 7, 128), (2 * 10 ** 6, 1024), (3 * 10 ** 5, 513),
                 (2 ** 31 - 1, 65)):
        assert lib.vmp_lda_wide_plan(n, K, *refs) == _lib.VMP_OK
        assert (r.value, c.value) == (host.lda_wide_regs(K), host.lda_wide_chunk_tokens(n))
        assert w.value == -(-n // c.value) * (2 * K + 1) + 1024
    for n, K in ((10, 64), (10, 1), (10, 0), (10, 1025), (2 ** 31, 70)):
        assert lib.vmp_lda_wide_plan(n, K, *refs) == _lib.VMP_ERR_UNSUPPORTED, (n, K)
    assert lib.vmp_lda_wide_plan(-1, 70, *refs) == _lib.VMP_ERR_INVALID
    assert lib.vmp_lda_wide_plan(10, 70, None, None, None) == _lib.VMP_ERR_INVALID
    assert lib.vmp_lda_wide_plan(10, 70, refs[0], refs[1], None) == _lib.VMP_ERR_INVALID
