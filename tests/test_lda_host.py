"""CPU: the latent-Dirichlet-allocation feature without a device -- the ``Constant(moments, value)``
form and ``CategoricalMoments``, the matcher of the fused block and its declining reasons, the
plan's host logic on the kernel double tests/lda_host.py (CPULDAKernels) against every fixture of
tests/golden/lda.npz (live reference, tools/make_golden_lda.py), the g++ build of the device header
csrc/vmp_lda_dev.h against a long-double restatement, and a save / load round trip."""
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
MOM_TOL = dict(rtol=1e-7, atol=1e-9)         # moments: MOM_RTOL of tests/test_generic_engine_gpu.py


def _mods(after=None, **kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments
    m = dict(nodes=nodes, VB=VB, CategoricalMoments=CategoricalMoments, vb_kwargs=kw)
    if after is not None:
        m['after_vb'] = after
    return m


def _on_double(Q):
    from bayespy_amd.device import Runtime
    from lda_host import CPULDAKernels
    plan = Q.plans[0]
    assert type(plan).__name__ == 'LDAPlan'
    rt = Runtime(device='cpu')
    plan._rt, plan._kernels = rt, CPULDAKernels(rt)


def _golden():
    g = np.load(os.path.join(GOLDEN, 'lda.npz'))
    return g, {k[3:]: g[k] for k in g.files if k.startswith('in_')}


def _doc_model(**kw):
    from lda_models import build_lda
    _, gin = _golden()
    return build_lda(_mods(), gin['doc_docs'], gin['doc_words'], 7, 30, 4, **kw)


# -- public interface -------------------------------------------------------------------------------
def test_constant_with_categorical_moments():
    from bayespy_amd import nodes
    from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments
    idx = np.array([0, 2, 1, 2])
    c = nodes.Constant(CategoricalMoments(3), idx, name='document_indices')
    assert c.name == 'document_indices' and c.plates == (4,)
    assert c.moments.categories == 3
    np.testing.assert_array_equal(c.indices, idx)
    np.testing.assert_array_equal(c.get_moments()[0], idx)
    c.set_value([2, 2, 0, 1])
    np.testing.assert_array_equal(c.indices, [2, 2, 0, 1])
    with pytest.raises(ValueError, match='Incorrect shape'):
        c.set_value([0, 1])
    with pytest.raises(ValueError, match='Invalid category index'):
        c.set_value([0, 1, 2, 3])
    with pytest.raises(ValueError, match='Values must be integers'):
        c.set_value([0.5, 1, 2, 0])
    with pytest.raises(ValueError, match='Invalid category index'):
        nodes.Constant(CategoricalMoments(3), [0, -1])
    with pytest.raises(ValueError, match='Values must be integers'):
        nodes.Constant(CategoricalMoments(3), [0.0, 1.5])
    with pytest.raises(ValueError, match='instance instead of a class'):
        nodes.Constant(CategoricalMoments, [0, 1])

    class OtherMoments:
        pass
    with pytest.raises(NotImplementedError, match='CategoricalMoments'):
        nodes.Constant(OtherMoments(), [0, 1])
    # the one-argument form is what it was
    c1 = nodes.Constant([[1.0, 2.0]], name='c1')
    assert c1.plates == (1, 2) and c1.moments is None and c1.name == 'c1'
    assert nodes.Constant(3.0, 'named').name == 'named'


def test_index_constant_is_an_index_parent_of_gate_and_mixture():
    from bayespy_amd import nodes
    from bayespy_amd.nodes.categorical import CategoricalMoments
    idx = np.array([0, 2, 1, 2, 0])
    c = nodes.Constant(CategoricalMoments(3), idx)
    p = nodes.Dirichlet(np.ones(4), plates=(3,))
    g = nodes.Gate(c, p)
    g0 = nodes.Gate(idx, nodes.Dirichlet(np.ones(4), plates=(3,)))
    assert g.plates == g0.plates == (5,) and g.K == g0.K == 3
    mu = nodes.GaussianARD(0, 1, plates=(3,))
    y = nodes.Mixture(c, nodes.GaussianARD, mu, 1.0)
    assert y.plates == (5,)
    with pytest.raises(ValueError, match='Invalid category index'):
        nodes.Gate(nodes.Constant(CategoricalMoments(4), [3]), p)


# -- the matcher ------------------------------------------------------------------------------------
def _match(m, extra=()):
    from bayespy_amd.inference.plans.lda import LDAPlan
    why = []
    nodes = [m['words'], m['topics'], m['p_word'], m['p_topic']] + list(extra)
    return LDAPlan.match(nodes, why), why


def test_matcher_accepts_the_doc_graph():
    for const in (False, True):
        m = _doc_model(index_constant=const)
        r, why = _match(m, [m['idx']] if const else [])
        assert r is not None and why == []
        assert r['words'] is m['words'] and r['p_topic'] is m['p_topic']


def test_matcher_declines_with_reasons():
    from bayespy_amd import nodes
    from lda_models import build_lda
    _, gin = _golden()
    docs, words = gin['doc_docs'], gin['doc_words']
    n = len(words)

    def reason(m):
        r, why = _match(m)
        assert r is None and len(why) == 1, why
        return why[0]
    # plates_multiplier on topics
    p_topic = nodes.Dirichlet(np.ones(4), plates=(7,), name='p_topic')
    p_word = nodes.Dirichlet(np.ones(30), plates=(4,), name='p_word')
    topics = nodes.Categorical(nodes.Gate(docs, p_topic), plates=(n,), plates_multiplier=(2.5,),
                               name='topics')
    w = nodes.Categorical(nodes.Gate(topics, p_word), name='words')
    w.observe(words)
    assert 'plates_multiplier' in reason(dict(words=w, topics=topics, p_word=p_word,
                                              p_topic=p_topic))
    # a mask
    m = _doc_model()
    m['words'].observe(words, mask=np.arange(n) % 2 == 0)
    assert 'mask' in reason(m)
    # a Concentration parent
    c = nodes.Concentration(4, name='c')
    p_topic = nodes.Dirichlet(c, plates=(7,), name='p_topic')
    p_word = nodes.Dirichlet(np.ones(30), plates=(4,), name='p_word')
    topics = nodes.Categorical(nodes.Gate(docs, p_topic), plates=(n,), name='topics')
    w = nodes.Categorical(nodes.Gate(topics, p_word), name='words')
    w.observe(words)
    assert 'Concentration' in reason(dict(words=w, topics=topics, p_word=p_word, p_topic=p_topic))
    # an extra child of one of the four nodes
    m = _doc_model()
    nodes.Categorical(m['p_topic'], name='another')
    assert 'other children' in reason(m)
    # more than one token axis
    p_topic = nodes.Dirichlet(np.ones(4), plates=(7,), name='p_topic')
    p_word = nodes.Dirichlet(np.ones(30), plates=(4,), name='p_word')
    topics = nodes.Categorical(nodes.Gate(docs.reshape(20, 20), p_topic), plates=(20, 20),
                               name='topics')
    w = nodes.Categorical(nodes.Gate(topics, p_word), name='words')
    w.observe(words.reshape(20, 20))
    assert 'one token plate axis' in reason(dict(words=w, topics=topics, p_word=p_word,
                                                 p_topic=p_topic))
    # too many topics
    m = build_lda(_mods(), docs, words, 7, 30, 65)
    assert 'exceeds the limit' in reason(m)
    # a sharded plate
    m = _doc_model()
    m['topics'].shard(-1)
    assert 'sharded' in reason(m)


def test_declined_model_runs_on_the_generic_engine_with_the_reason():
    from bayespy_amd.inference.plans import compile_model
    from bayespy_amd.inference.plans.generic import GenericPlan
    m = _doc_model()
    m['words'].observe(_golden()[1]['doc_words'], mask=np.arange(400) % 2 == 0)
    with pytest.warns(UserWarning, match='fused LDA block.*mask'):
        plans = compile_model([m['words'], m['topics'], m['p_word'], m['p_topic']])
    assert isinstance(plans[0], GenericPlan)


def test_matcher_is_silent_without_the_two_level_structure():
    """Gate / Categorical / Dirichlet models of another shape get no reason from this matcher."""
    from bayespy_amd import nodes
    from bayespy_amd.inference.plans.lda import LDAPlan
    p = nodes.Dirichlet(np.ones(3), plates=(4,), name='p')
    z = nodes.Categorical(nodes.Gate(np.array([0, 1, 2, 3, 0]), p), name='z')
    z.observe([0, 1, 2, 0, 1])
    a = nodes.Dirichlet(np.ones(3), name='a')
    zz = nodes.Categorical(a, plates=(5,), name='zz')
    x = nodes.Categorical(nodes.Gate(zz, nodes.Dirichlet(np.ones(2), plates=(3,), name='b')),
                          name='x')
    x.observe([0, 1, 0, 1, 1])
    for model in ([z, p], [x, zz, a] + [x.parents[0].parents[1]]):
        why = []
        assert LDAPlan.match(model, why) is None and why == []


# -- the plan on the kernel double ---------------------------------------------------------------------
def test_plan_reproduces_every_fixture_on_the_kernel_double():
    from lda_models import run_lda_cases
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_lda_cases(_mods(_on_double), gin, moments_of=('topics', 'p_word', 'p_topic'))
    checked = 0
    for k, v in res.items():
        if k.endswith('_plan'):
            continue
        tol = MOM_TOL if k.endswith('_u0') else TRACE_TOL
        np.testing.assert_allclose(v, g[k], err_msg=k, **tol)
        checked += 1
    assert checked == 8 * (1 + 4 + 3)
    # the index constant and the raw array: identical results
    raw = _mods(_on_double)
    raw['raw_indices'] = True
    res_raw = run_lda_cases(raw, gin, only=('const',), moments_of=('topics', 'p_word', 'p_topic'))
    for k in res_raw:
        if not k.endswith('_plan'):
            np.testing.assert_array_equal(res[k], res_raw[k], err_msg=k)
    # moments of words are never formed
    Q = res['doc_plan']
    with pytest.raises(NotImplementedError, match='never forms'):
        Q['words'].get_moments()
    calls = Q.plans[0].kernels.calls
    assert 'token_pass_phi' in calls and calls.count('token_pass') == 1 + 5


def test_save_load_round_trip_on_the_double(tmp_path):
    from lda_models import run_lda_cases
    g, gin = _golden()
    res = run_lda_cases(_mods(_on_double), gin, only=('doc',), moments_of=())
    Q = res['doc_plan']
    fn = str(tmp_path / 'lda.ckpt')
    Q.save(filename=fn)
    L5 = Q.L[:5].copy()
    Q.update(repeat=2, verbose=False)
    L7 = Q.L[:7].copy()
    Q.load(filename=fn)
    assert Q.iter == 5
    np.testing.assert_array_equal(Q.L[:5], L5)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:7], L7)


def test_reobserve_and_set_value_rebuild_the_layouts():
    from lda_models import build_lda
    _, gin = _golden()
    m = build_lda(_mods(), gin['doc_docs'], gin['doc_words'], 7, 30, 4, index_constant=True)
    from bayespy_amd.inference import VB
    m['p_topic'].initialize_from_value(gin['doc_theta0'])
    m['p_word'].initialize_from_value(gin['doc_beta0'])
    Q = VB(m['words'], m['topics'], m['p_word'], m['p_topic'], m['idx'])
    _on_double(Q)
    Q.update(repeat=2, verbose=False)
    plan = Q.plans[0]
    theta = m['p_topic'].get_moments()[0]
    perm = np.random.RandomState(0).permutation(400)
    m['words'].observe(gin['doc_words'][perm])
    m['idx'].set_value(gin['doc_docs'][perm])
    assert Q.plans[0] is plan
    np.testing.assert_array_equal(m['p_topic'].get_moments()[0], theta)     # the posterior stayed
    Q.update('topics', verbose=False)
    # the same multiset of tokens: the same counts, bit for bit
    N1 = plan.Ndk.numpy().copy()
    m['words'].observe(gin['doc_words'])
    m['idx'].set_value(gin['doc_docs'])
    Q.update('topics', verbose=False)
    np.testing.assert_array_equal(plan.Ndk.numpy(), N1)
    with pytest.raises(ValueError, match='Invalid category index'):
        m['words'].observe(np.full(400, 30))
        Q.update('topics', verbose=False)


def test_generic_engine_api_raises_its_own_errors():
    from lda_models import run_lda_cases
    _, gin = _golden()
    Q = run_lda_cases(_mods(_on_double), gin, only=('k1',), moments_of=())['k1_plan']
    with pytest.raises(NotImplementedError, match='generic engine'):
        Q.gradient_step('p_topic', 'p_word', scale=0.5)
    with pytest.raises(NotImplementedError, match="engine='generic'"):
        Q.set_annealing(0.5)
    with pytest.raises(NotImplementedError, match="engine='generic'"):
        Q.get_parameters('p_topic')


def test_svi_half_on_the_generic_engine_double_matches_reference():
    """Mini-batches with ``plates_multiplier`` through the two gates, ``set_value`` on the index
    constant and ``gradient_step``: the generic engine on the NumPy double of its entry points
    (tests/host_generic.py) against the live reference."""
    import host_generic
    from lda_models import run_lda_svi
    from bayespy_amd.inference.plans.generic import GenericPlan
    g, gin = _golden()
    host_generic.install()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res = run_lda_svi(_mods(engine='generic'), gin)
    finally:
        host_generic.uninstall()
    assert isinstance(res['svi_plan'].plans[0], GenericPlan)
    np.testing.assert_allclose(res['svi_L'], g['svi_L'], **TRACE_TOL)
    for k in ('svi_p_word_u0', 'svi_p_topic_u0', 'svi_topics_u0'):
        np.testing.assert_allclose(res[k], g[k], err_msg=k, **MOM_TOL)


# -- the device header on the host ---------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 2, 3, 5, 8, 17, 32, 33, 64])
def test_host_build_of_the_device_header_against_long_double(K):
    """The bound of a count, u = 2^-53.  A responsibility is exp(l - lse): the argument carries the
    rounding of the logit (u |l|), the error of lse (u |lse| from m + log s, plus 2 u for the log
    and the sum under it, whose terms are exact to 1 u each and positive) and the rounding of the
    difference (u |l - lse|), with |l| <= lmax, |lse| <= lmax + log K, |l - lse| <= 2 lmax + log K:
    at most (4 (lmax + log K) + 3) u absolute in the argument = relative in phi, plus 1 u for the
    exp itself: c = 4 + 4 (lmax + log K).  A count adds `len` such terms one after the other
    (positive terms: (len - 1) u relative):  |error| <= (len + c) u * count."""
    from lda_host import lda_host, make_layouts, host_token_pass, restate
    rs = np.random.RandomState(100 + K)
    lib = lda_host()
    assert lib.lda_group(K) == 1 << max(0, (K - 1).bit_length())
    D, V = 6, 11
    T = lib.lda_chunk_tokens(1000, K)
    assert T == 16
    for n in (0, 1, T - 1, T, T + 1, 5 * T + 3):
        doc = np.sort(rs.randint(D, size=n)) if n != 5 * T + 3 else np.zeros(n, dtype=np.int64)
        word = rs.randint(V, size=n)
        et = np.log(rs.dirichlet(np.ones(K), size=D))
        ebt = np.log(rs.dirichlet(np.ones(V), size=K)).T
        lay, orig = make_layouts(doc, word, D, V)
        Ndk, Nvk, scal, lse, phi = host_token_pass(n, D, V, K, lay, None, et, ebt, orig=orig,
                                                   want_phi=True)
        rphi, rlse, rN, rM = restate(doc, word, D, V, K, et, ebt)
        u = 2.0 ** -53
        lmax = float(np.abs(et).max() + np.abs(ebt).max())
        seg = max(n, 1)
        c = 4 + 4 * (lmax + np.log(K))
        bound = (seg + c) * u
        assert np.all(np.abs(Ndk - rN) <= bound * np.maximum(rN, 0) + 0.0), (K, n)
        assert np.all(np.abs(Nvk - rM) <= bound * np.maximum(rM, 0) + 0.0), (K, n)
        if n:
            np.testing.assert_allclose(phi, rphi.astype(np.float64), rtol=c * u,
                                       atol=0)
            # lse comes in document order: token orig[i] of the caller stands at i
            np.testing.assert_allclose(lse, rlse.astype(np.float64)[orig], rtol=0,
                                       atol=4 * u * (lmax + np.log(K) + 1))
        # sum of lse: every term within its own bound, then at most T additions inside a chunk
        # and one more per chunk (NumPy adds the chunk sums pairwise: fewer)
        adds = T + n / T + 1
        np.testing.assert_allclose(scal[0], float(rlse.sum()), rtol=0,
                                   atol=n * 4 * u * (lmax + np.log(K) + 1)
                                   + adds * u * float(np.abs(rlse).sum()))
        # rows of both count tables add up to the same per-topic totals
        np.testing.assert_allclose(Ndk.sum(0), Nvk.sum(0), rtol=1e-12, atol=1e-300)


def test_host_build_edge_cases():
    from lda_host import make_layouts, host_token_pass
    K, D, V = 3, 4, 5
    et = np.log(np.full((D, K), 1.0 / K))
    ebt = np.log(np.full((V, K), 1.0 / V))
    # n = 0: zeros
    lay, _ = make_layouts([], [], D, V)
    Ndk, Nvk, scal, _, _ = host_token_pass(0, D, V, K, lay, None, et, ebt)
    assert not Ndk.any() and not Nvk.any() and scal[0] == 0
    # empty documents and unused words are exact zeros; one document holds every token
    doc, word = np.full(100, 2), np.arange(100) % 2
    lay, _ = make_layouts(doc, word, D, V)
    Ndk, Nvk, _, _, _ = host_token_pass(100, D, V, K, lay, None, et, ebt)
    assert not Ndk[[0, 1, 3]].any() and not Nvk[2:].any()
    np.testing.assert_allclose(Ndk[2], 100.0 / 3, rtol=1e-13)
    np.testing.assert_allclose(Nvk[:2], 50.0 / 3, rtol=1e-13)
    # a topic with a -inf logit gets exactly zero, nothing turns NaN
    et2 = et.copy()
    et2[:, 1] = -np.inf
    Ndk, Nvk, scal, lse, _ = host_token_pass(100, D, V, K, lay, None, et2, ebt)
    assert np.all(Ndk[:, 1] == 0) and np.all(np.isfinite(Ndk)) and np.all(np.isfinite(lse))
    # fixed labels: one-hot counts, lse = 0
    lab = (np.arange(100) % 3).astype(np.int32)
    Ndk, Nvk, scal, lse, _ = host_token_pass(100, D, V, K, lay, lab, et, ebt)
    np.testing.assert_array_equal(Ndk[2], [34, 33, 33])
    assert scal[0] == 0 and not lse.any()


def test_cabi_declares_the_lda_entry_points():
    from bayespy_amd import _lib
    lib = _lib.load()
    for name in ('vmp_lda_limits', 'vmp_lda_plan', 'vmp_lda_token_pass', 'vmp_lda_dirichlet',
                 'vmp_lda_dot'):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    mk, mc = ctypes.c_int32(), ctypes.c_int32()
    assert lib.vmp_lda_limits(ctypes.byref(mk), ctypes.byref(mc)) == _lib.VMP_OK
    from bayespy_amd.inference.plans.lda import LDA_MAX_K
    assert mk.value == LDA_MAX_K >= 64 and mc.value == 256
    assert lib.vmp_lda_limits(None, None) == _lib.VMP_ERR_INVALID
    g, c, w = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    from lda_host import lda_host
    host = lda_host()
    for n, K in ((0, 1), (1000, 5), (10 ** 7, 16), (10 ** 7, 64), (3 * 10 ** 5, 33)):
        assert lib.vmp_lda_plan(n, K, ctypes.byref(g), ctypes.byref(c), ctypes.byref(w)) == 0
        assert (g.value, c.value) == (host.lda_group(K), host.lda_chunk_tokens(n, K))
        nc = -(-n // c.value)
        assert w.value == nc * (2 * K + 1) + 1024
    assert lib.vmp_lda_plan(10, 65, ctypes.byref(g), ctypes.byref(c),
                            ctypes.byref(w)) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_lda_plan(-1, 4, ctypes.byref(g), ctypes.byref(c),
                            ctypes.byref(w)) == _lib.VMP_ERR_INVALID
    assert lib.vmp_lda_plan(10, 4, None, None, None) == _lib.VMP_ERR_INVALID
