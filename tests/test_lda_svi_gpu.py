"""GPU: stochastic variational inference on the fused latent-Dirichlet-allocation block
(inference/plans/lda.py LDASVIPlan, csrc/vmp_lda.hip vmp_lda_dirichlet_step) -- the SVI fixtures of
tests/golden/lda.npz (live reference) under ``engine='fused'``, the block against the generic engine
at batch sizes that cross the 256-token chunk and hit both Dirichlet forms, the step kernel through
the C ABI against a SciPy restatement, the equivalence of a full step to a VB update, checkpoints."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
from scipy import special

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from test_generic_engine_gpu import MOM_RTOL        # noqa: E402

TRACE_TOL = dict(rtol=1e-8, atol=1e-8)       # tests/test_lda_gpu.py
MOM_TOL = dict(rtol=MOM_RTOL, atol=1e-9)
U = 2.0 ** -53


def _mods(**kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments
    return dict(nodes=nodes, VB=VB, CategoricalMoments=CategoricalMoments, vb_kwargs=kw)


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'lda.npz'))
    return g, {k[3:]: g[k] for k in g.files if k.startswith('in_')}


def test_svi_half_matches_reference_on_the_fused_block(golden_dir):
    from lda_models import run_lda_svi
    from bayespy_amd.inference.plans.lda import LDASVIPlan
    g, gin = _golden(golden_dir)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        res = run_lda_svi(_mods(engine='fused'), gin)
    assert not [str(w.message) for w in rec
                if 'engine' in str(w.message) or 'block' in str(w.message)]
    assert [type(p) for p in res['svi_plan'].plans] == [LDASVIPlan]
    np.testing.assert_allclose(res['svi_L'], g['svi_L'], **TRACE_TOL)
    for k in ('svi_p_word_u0', 'svi_p_topic_u0', 'svi_topics_u0'):
        np.testing.assert_allclose(res[k], g[k], err_msg=k, **MOM_TOL)


# -- the block against the generic engine ------------------------------------------------------------
def _svi_run(engine, n, S, D, V, K, seed, steps=3, device_batches=False, stop_after=None,
             resume=None):
    """One sweep, then ``steps`` SVI steps on seeded inputs; {trace, moments, Q}."""
    import torch
    from bayespy_amd import nodes as N_
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments
    rs = np.random.RandomState(seed)
    docs, corpus = rs.randint(D, size=n), rs.randint(V, size=n)
    theta0, beta0 = rs.dirichlet(np.ones(K), size=D), rs.dirichlet(np.ones(V), size=K)
    p_topic = N_.Dirichlet(np.ones(K), plates=(D,), name='p_topic')
    p_word = N_.Dirichlet(np.ones(V), plates=(K,), name='p_word')
    idx = N_.Constant(CategoricalMoments(D), docs[:S], name='document_indices')
    topics = N_.Categorical(N_.Gate(idx, p_topic), plates=(S,), plates_multiplier=(n / S,),
                            name='topics')
    words = N_.Categorical(N_.Gate(topics, p_word), name='words')
    words.observe(corpus[:S])
    p_topic.initialize_from_value(theta0)
    p_word.initialize_from_value(beta0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        Q = VB(words, topics, p_word, p_topic, idx, engine=engine)
    Q.ignore_bound_checks = True
    Q.update(verbose=False)
    dev = (lambda a: torch.from_numpy(a).to('cuda')) if device_batches else (lambda a: a)
    for it in range(steps):
        subset = rs.choice(n, S)
        if resume is not None and it == resume[1]:
            Q.load(filename=resume[0])
        words.observe(dev(corpus[subset]))
        idx.set_value(dev(docs[subset]))
        Q.update('topics', verbose=False)
        # a run that will load a checkpoint takes other steps until then: the load restores all
        before_load = resume is not None and it < resume[1]
        Q.gradient_step('p_topic', 'p_word', scale=0.9 if before_load else (it + 1) ** (-0.7))
        if stop_after is not None and it + 1 == stop_after[1]:
            Q.save(filename=stop_after[0])
    return dict(L=np.array(Q.L[:Q.iter]), p_word=np.array(p_word.get_moments()[0]),
                p_topic=np.array(p_topic.get_moments()[0]),
                topics=np.array(topics.get_moments()[0]), Q=Q)


SVI_SHAPES = [(5000, 700, 23, 130, 5), (5000, 300, 9, 70, 64), (5000, 300, 6, 12, 1)]


@pytest.mark.parametrize('n,S,D,V,K', SVI_SHAPES)
def test_block_against_the_generic_engine(n, S, D, V, K):
    from bayespy_amd.inference.plans.lda import LDASVIPlan
    from bayespy_amd.inference.plans.generic import GenericPlan
    ref = _svi_run('generic', n, S, D, V, K, seed=40 + K)
    blk = _svi_run('fused', n, S, D, V, K, seed=40 + K)
    assert isinstance(ref['Q'].plans[0], GenericPlan)
    assert [type(p) for p in blk['Q'].plans] == [LDASVIPlan]
    assert len(blk['L']) == 4 and np.all(np.isfinite(blk['L'][1:]))
    np.testing.assert_allclose(blk['L'], ref['L'], **TRACE_TOL)
    for k in ('p_word', 'p_topic', 'topics'):
        np.testing.assert_allclose(blk[k], ref[k], err_msg=k, **MOM_TOL)


def test_device_batches_stay_on_the_device():
    """Integer tensors in HBM as batches: the same bits as host arrays, and the index constant keeps
    the tensor (no host copy is formed by the block)."""
    n, S, D, V, K = 5000, 700, 23, 130, 5
    a = _svi_run('fused', n, S, D, V, K, seed=3)
    b = _svi_run('fused', n, S, D, V, K, seed=3, device_batches=True)
    for k in ('L', 'p_word', 'p_topic', 'topics'):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    idx = b['Q']['document_indices']
    assert idx.device_value is not None and idx.device_value.is_cuda and idx._value is None
    assert b['Q']['words']._data.is_cuda
    # the checks of the reference, made on the device with the rebuild
    import torch
    b['Q']['words'].observe(torch.full((S,), V, dtype=torch.int64, device='cuda'))
    with pytest.raises(ValueError, match='Invalid category index'):
        b['Q'].update('topics', verbose=False)


# -- the step kernel through the C ABI ---------------------------------------------------------------
def _restate(prior, counts, mult, scale, alpha):
    """lda_host.dirichlet_rows with the step: rows x cols arrays -> (q, alpha, elog, bound)."""
    q = prior + (0.0 if counts is None else mult * counts)
    new = q if scale == 1 else alpha + scale * (q - alpha)
    elog = special.digamma(new) - special.digamma(new.sum(-1, keepdims=True))

    def g(a):
        return special.gammaln(a.sum(-1)) - special.gammaln(a).sum(-1)
    bound = float(np.sum((prior - new) * elog) + np.sum(g(prior) - g(new)))
    return q, new, elog, bound


class _Step:
    def __init__(self):
        from bayespy_amd.device import get_runtime
        from bayespy_amd.inference.plans.lda import LDAKernels
        self.rt = get_runtime()
        self.k = LDAKernels(self.rt)

    def run(self, rows, cols, transposed, prior, counts, mult, scale, alpha, entry='step'):
        """Device (alpha, elog, bound) for rows x cols host arrays in either storage order."""
        import torch
        rt, k = self.rt, self.k
        store = (lambda a: np.ascontiguousarray(a.T)) if transposed else np.ascontiguousarray
        back = (lambda t: t.cpu().numpy().T) if transposed else (lambda t: t.cpu().numpy())
        rs_, cs_ = (1, rows) if transposed else (cols, 1)
        up = lambda a: None if a is None else torch.from_numpy(store(a)).to(rt.device)  # noqa: E731
        dp, dc, al = up(prior), up(counts), up(alpha)
        el = torch.full_like(dp, float('nan'))
        out = torch.full((1,), float('nan'), dtype=torch.float64, device=rt.device)
        rt.sync_stream()
        if entry == 'step':
            ws = rt.empty(k.dirichlet_step_ws(rows, cols, rs_, cs_))
            k.dirichlet_step(rows, cols, rs_, cs_, dp, dc, mult, scale, al, el, ws, out)
        else:
            ws = rt.empty(max(rows, 1024))
            k.dirichlet(rows, cols, rs_, cs_, dp, dc, al, el, ws, out)
        rt.synchronize()
        return back(al), back(el), float(out.item())


STEP_SHAPES = [(7, 4, False), (300, 64, False), (3, 65, False), (2, 1000, False)] \
    + [(K, V, True) for K in (1, 3, 64) for V in (1, 63, 257, 5000)]


@pytest.mark.parametrize('rows,cols,transposed', STEP_SHAPES)
def test_step_kernel_against_scipy(rows, cols, transposed):
    st = _Step()
    rs = np.random.RandomState(rows * 7919 + cols)
    prior = rs.gamma(1.0, 1.0, size=(rows, cols)) + 0.01
    counts = rs.gamma(2.0, 3.0, size=(rows, cols)) * (rs.rand(rows, cols) < 0.7)
    old = rs.gamma(2.0, 2.0, size=(rows, cols)) + 0.01
    for mult in (1, 4.0, 2.5):
        for scale in (1, 0.37):
            for cnt in (counts, None):
                al, el, b = st.run(rows, cols, transposed, prior, cnt, mult, scale, old)
                q, ra, re, rb = _restate(prior, cnt, mult, scale, old)
                err = np.abs(al - ra)
                lim = 8 * U * np.maximum(np.abs(old), np.abs(q))
                print('%s mult=%s scale=%s counts=%s: alpha error / bound %.3g, elog %.3g, '
                      'bound %.3g' % ((rows, cols, transposed), mult, scale, cnt is not None,
                                      float((err / lim).max()), float(np.abs(el - re).max()),
                                      abs(b - rb)))
                assert np.all(err <= lim)
                np.testing.assert_allclose(el, re, rtol=1e-11, atol=1e-12)
                np.testing.assert_allclose(b, rb, rtol=1e-10, atol=1e-9)
    # scale = 1 never reads the old alpha: NaN there, a finite result, the bits of vmp_lda_dirichlet
    nan = np.full((rows, cols), np.nan)
    al, el, b = st.run(rows, cols, transposed, prior, counts, 1, 1, nan)
    al0, el0, b0 = st.run(rows, cols, transposed, prior, counts, 1, 1, nan, entry='dirichlet')
    assert np.all(np.isfinite(al)) and np.all(np.isfinite(el)) and np.isfinite(b)
    np.testing.assert_array_equal(al, al0)
    np.testing.assert_allclose(el, el0, rtol=1e-11, atol=1e-12)
    # two calls: identical bits of every output
    x = st.run(rows, cols, transposed, prior, counts, 2.5, 0.37, old)
    y = st.run(rows, cols, transposed, prior, counts, 2.5, 0.37, old)
    for u, v in zip(x, y):
        np.testing.assert_array_equal(u, v)


def test_step_kernel_argument_checks():
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    lib, ctx = rt.lib, rt.ctx
    z = rt.zeros(4096)
    out = rt.empty(1)
    out.fill_(float('nan'))
    p, o = ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(out.data_ptr())
    step = lib.vmp_lda_dirichlet_step
    rt.sync_stream()
    assert step(ctx, 0, 4, 4, 1, p, None, 1.0, 1.0, p, p, p, o) == _lib.VMP_OK
    rt.synchronize()
    assert float(out.item()) == 0.0                                      # rows = 0: bound 0
    assert step(ctx, 0, 4, 1, 0, p, None, 1.0, 0.5, p, p, p, o) == _lib.VMP_ERR_INVALID
    assert step(ctx, -1, 4, 4, 1, p, None, 1.0, 1.0, p, p, p, o) == _lib.VMP_ERR_INVALID
    assert step(ctx, 2, 0, 4, 1, p, None, 1.0, 1.0, p, p, p, o) == _lib.VMP_ERR_INVALID
    assert step(ctx, 2, 4, -4, 1, p, None, 1.0, 1.0, p, p, p, o) == _lib.VMP_ERR_INVALID
    assert step(ctx, 2, 4, 4, 1, p, None, 0.0, 1.0, p, p, p, o) == _lib.VMP_ERR_INVALID
    assert step(ctx, 2, 4, 4, 1, p, None, -2.0, 1.0, p, p, p, o) == _lib.VMP_ERR_INVALID
    assert step(ctx, 2, 4, 4, 1, p, None, float('nan'), 1.0, p, p, p, o) == _lib.VMP_ERR_INVALID
    assert step(ctx, 2, 4, 4, 1, p, None, 1.0, float('nan'), p, p, p, o) == _lib.VMP_ERR_INVALID
    assert step(ctx, 2, 4, 4, 1, None, None, 1.0, 1.0, p, p, p, o) == _lib.VMP_ERR_INVALID
    assert step(ctx, 2, 4, 4, 1, p, None, 1.0, 1.0, None, p, p, o) == _lib.VMP_ERR_INVALID
    assert step(ctx, 2, 4, 4, 1, p, None, 1.0, 1.0, p, None, p, o) == _lib.VMP_ERR_INVALID
    assert step(ctx, 2, 4, 4, 1, p, None, 1.0, 1.0, p, p, None, o) == _lib.VMP_ERR_INVALID
    assert step(ctx, 2, 4, 4, 1, p, None, 1.0, 1.0, p, p, p, None) == _lib.VMP_ERR_INVALID
    assert step(None, 2, 4, 4, 1, p, None, 1.0, 1.0, p, p, p, o) == _lib.VMP_ERR_INVALID
    w = ctypes.c_int64()
    q = lib.vmp_lda_dirichlet_step_workspace
    assert q(300, 64, 64, 1, ctypes.byref(w)) == _lib.VMP_OK and w.value == 300
    assert q(64, 100000, 1, 64, ctypes.byref(w)) == _lib.VMP_OK and 64 < w.value < 10 ** 6
    assert q(0, 4, 4, 1, ctypes.byref(w)) == _lib.VMP_OK and w.value >= 1
    assert q(-1, 4, 4, 1, ctypes.byref(w)) == _lib.VMP_ERR_INVALID
    assert q(2, 4, 4, 1, None) == _lib.VMP_ERR_INVALID
    rt.synchronize()


# -- the plan ------------------------------------------------------------------------------------------
def _doc_model(gin, engine):
    from lda_models import build_lda
    from bayespy_amd.inference import VB
    m = build_lda(_mods(), gin['doc_docs'], gin['doc_words'], 7, 30, 4, index_constant=True)
    m['p_topic'].initialize_from_value(gin['doc_theta0'])
    m['p_word'].initialize_from_value(gin['doc_beta0'])
    kw = {} if engine is None else dict(engine=engine)
    Q = VB(m['words'], m['topics'], m['p_word'], m['p_topic'], m['idx'], **kw)
    Q.ignore_bound_checks = True
    return m, Q


def test_full_gradient_step_is_a_vb_update(golden_dir):
    from bayespy_amd.inference.plans.lda import LDAPlan, LDASVIPlan
    _, gin = _golden(golden_dir)
    m0, Q0 = _doc_model(gin, None)
    m1, Q1 = _doc_model(gin, 'fused')
    assert type(Q0.plans[0]) is LDAPlan and type(Q1.plans[0]) is LDASVIPlan
    for Q in (Q0, Q1):
        Q.update(repeat=2, verbose=False)
        Q.update('topics', verbose=False)
    Q0.update('p_word', 'p_topic', verbose=False)
    Q1.gradient_step('p_word', 'p_topic', scale=1)
    for nm in ('p_word', 'p_topic', 'topics'):
        np.testing.assert_allclose(m1[nm].get_moments()[0], m0[nm].get_moments()[0], err_msg=nm,
                                   **MOM_TOL)
    np.testing.assert_array_equal(Q1.plans[0].alpha_beta_t.cpu().numpy(),
                                  Q0.plans[0].alpha_beta_t.cpu().numpy())
    np.testing.assert_allclose(Q1.compute_lowerbound(), Q0.compute_lowerbound(), **TRACE_TOL)
    # a point mass under a partial step: the generic engine's result, never a NaN table
    m2, Q2 = _doc_model(gin, 'fused')
    m3, Q3 = _doc_model(gin, 'generic')
    for Q in (Q2, Q3):
        Q.gradient_step('p_word', 'p_topic', scale=0.3)
    for nm in ('p_word', 'p_topic'):
        got = m2[nm].get_moments()[0]
        assert np.all(np.isfinite(got))
        np.testing.assert_allclose(got, m3[nm].get_moments()[0], err_msg=nm, **MOM_TOL)


def test_checkpoints_in_the_middle_of_an_svi_run(golden_dir, tmp_path):
    n, S, D, V, K = 5000, 300, 9, 70, 8
    fn = str(tmp_path / 'svi.ckpt')
    whole = _svi_run('fused', n, S, D, V, K, seed=11, steps=4, stop_after=(fn, 2))
    # a second run loads the state after step 2 in place of its own and continues to the same trace
    again = _svi_run('fused', n, S, D, V, K, seed=11, steps=4, resume=(fn, 2))
    np.testing.assert_array_equal(again['L'][3:], whole['L'][3:])
    for k in ('p_word', 'p_topic', 'topics'):
        np.testing.assert_array_equal(again[k], whole[k], err_msg=k)
    # a checkpoint of the default plan loads into the mini-batch form
    _, gin = _golden(golden_dir)
    m0, Q0 = _doc_model(gin, None)
    Q0.update(repeat=3, verbose=False)
    fn0 = str(tmp_path / 'lda.ckpt')
    Q0.save(filename=fn0)
    m1, Q1 = _doc_model(gin, 'fused')
    Q1.load(filename=fn0)
    assert Q1.iter == 3
    for nm in ('p_word', 'p_topic', 'topics'):
        np.testing.assert_array_equal(m1[nm].get_moments()[0], m0[nm].get_moments()[0])
    Q0.update(verbose=False)
    Q1.update(verbose=False)
    np.testing.assert_allclose(Q1.L[3], Q0.L[3], **TRACE_TOL)
    # and the other way round
    fn1 = str(tmp_path / 'svi_plan.ckpt')
    Q1.save(filename=fn1)
    Q0.load(filename=fn1)
    np.testing.assert_array_equal(m0['p_word'].get_moments()[0], m1['p_word'].get_moments()[0])
