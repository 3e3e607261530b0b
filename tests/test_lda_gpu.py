"""GPU: the fused latent-Dirichlet-allocation block (inference/plans/lda.py, csrc/vmp_lda.hip) --
every fixture of tests/golden/lda.npz (live reference) through ``VB`` on the block and on the
generic engine, the token pass through the C ABI against a long-double restatement at sizes that
cross chunk and lane-group boundaries, bit-identity, the memory peak, save / load, the
responsibilities on request and the argument checks."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from test_generic_engine_gpu import MOM_RTOL        # noqa: E402

TRACE_TOL = dict(rtol=1e-8, atol=1e-8)       # _compare_shared: scalars and traces
MOM_TOL = dict(rtol=MOM_RTOL, atol=1e-9)     # _compare_shared: moments
U = 2.0 ** -53


def _mods(**kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments
    return dict(nodes=nodes, VB=VB, CategoricalMoments=CategoricalMoments, vb_kwargs=kw)


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'lda.npz'))
    return g, {k[3:]: g[k] for k in g.files if k.startswith('in_')}


def _compare(res, g, skip_words=False):
    n = 0
    for k, v in res.items():
        if k.endswith('_plan'):
            continue
        if k.endswith('_words_u0'):
            if skip_words:
                continue
            assert np.all((v == 0) | (v == 1))
            np.testing.assert_array_equal(np.argmax(v, axis=-1), g[k], err_msg=k)
        else:
            np.testing.assert_allclose(v, g[k], err_msg=k,
                                       **(MOM_TOL if k.endswith('_u0') else TRACE_TOL))
        n += 1
    return n


def test_every_fixture_on_the_fused_block(golden_dir):
    from lda_models import run_lda_cases, CASES
    from bayespy_amd.inference.plans.lda import LDAPlan
    g, gin = _golden(golden_dir)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        res = run_lda_cases(_mods(), gin, moments_of=('topics', 'p_word', 'p_topic'))
    # neither "runs on the generic engine" nor "the block restarts": nothing about engines or blocks
    assert not [str(w.message) for w in rec
                if 'engine' in str(w.message) or 'block' in str(w.message)]
    for tag in CASES:
        plans = res[tag + '_plan'].plans
        assert len(plans) == 1 and isinstance(plans[0], LDAPlan), tag
    assert _compare(res, g) == len(CASES) * 8
    raw = _mods()
    raw['raw_indices'] = True
    res_raw = run_lda_cases(raw, gin, only=('const',), moments_of=('topics', 'p_word', 'p_topic'))
    for k in res_raw:
        if not k.endswith('_plan'):
            np.testing.assert_array_equal(res[k], res_raw[k], err_msg=k)
    with pytest.raises(NotImplementedError, match='never forms'):
        res['doc_plan']['words'].get_moments()


def test_every_fixture_on_the_generic_engine(golden_dir):
    from lda_models import run_lda_cases, CASES
    from bayespy_amd.inference.plans.generic import GenericPlan
    g, gin = _golden(golden_dir)
    res = run_lda_cases(_mods(engine='generic'), gin)
    for tag in CASES:
        assert isinstance(res[tag + '_plan'].plans[0], GenericPlan)
    assert _compare(res, g) == len(CASES) * 9
    # and the block agrees with the generic engine to the same tolerance
    blk = run_lda_cases(_mods(), gin, moments_of=('topics', 'p_word', 'p_topic'))
    for k, v in blk.items():
        if not k.endswith('_plan'):
            np.testing.assert_allclose(v, res[k], err_msg=k,
                                       **(MOM_TOL if k.endswith('_u0') else TRACE_TOL))


def test_svi_half_matches_reference_on_the_generic_engine(golden_dir):
    from lda_models import run_lda_svi
    from bayespy_amd.inference.plans.generic import GenericPlan
    g, gin = _golden(golden_dir)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = run_lda_svi(_mods(engine='generic'), gin)
    assert isinstance(res['svi_plan'].plans[0], GenericPlan)
    np.testing.assert_allclose(res['svi_L'], g['svi_L'], **TRACE_TOL)
    for k in ('svi_p_word_u0', 'svi_p_topic_u0', 'svi_topics_u0'):
        np.testing.assert_allclose(res[k], g[k], err_msg=k, **MOM_TOL)


def test_svi_half_of_the_doc_example_runs_on_the_generic_engine():
    """doc/source/examples/lda.rst, second half, at its size: mini-batches with
    ``plates_multiplier``, ``set_value`` on the index constant, ``gradient_step``."""
    from bayespy_amd import nodes
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.plans.generic import GenericPlan
    from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments
    rs = np.random.RandomState(3)
    n_documents, n_words, n_vocabulary, n_topics, subset_size = 10, 10000, 100, 5, 1000
    word_documents = rs.randint(n_documents, size=n_words)
    corpus = rs.randint(n_vocabulary, size=n_words)
    p_topic = nodes.Dirichlet(np.ones(n_topics), plates=(n_documents,), name='p_topic')
    p_word = nodes.Dirichlet(np.ones(n_vocabulary), plates=(n_topics,), name='p_word')
    document_indices = nodes.Constant(CategoricalMoments(n_documents),
                                      word_documents[:subset_size], name='document_indices')
    topics = nodes.Categorical(nodes.Gate(document_indices, p_topic), plates=(subset_size,),
                               plates_multiplier=(n_words / subset_size,), name='topics')
    words = nodes.Categorical(nodes.Gate(topics, p_word), name='words')
    words.observe(corpus[:subset_size])
    p_topic.initialize_from_random()
    p_word.initialize_from_random()
    Q = VB(words, topics, p_word, p_topic, document_indices, engine='generic')
    assert isinstance(Q.plans[0], GenericPlan)
    Q.ignore_bound_checks = True
    seen = []
    for it in range(4):
        subset = rs.choice(n_words, subset_size)
        Q['words'].observe(corpus[subset])
        Q['document_indices'].set_value(word_documents[subset])
        Q.update('topics', verbose=False)
        # the responsibilities follow the new indices: rows gather the new documents' tables
        seen.append(Q['topics'].get_moments()[0].copy())
        Q.gradient_step('p_topic', 'p_word', scale=(it + 1) ** (-0.7))
    assert Q.iter == 4 and np.all(np.isfinite(Q.L[1:4]))
    assert not np.allclose(seen[0], seen[1])
    # without engine='generic' the same model declines the block and says why
    with pytest.warns(UserWarning, match='fused LDA block.*plates_multiplier'):
        Q2 = VB(words, topics, p_word, p_topic, document_indices)
    assert isinstance(Q2.plans[0], GenericPlan)


# -- the token pass through the C ABI -------------------------------------------------------------------
def _device_pass(doc, word, D, V, K, et, ebt, want_phi=False, labels=None):
    import torch
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.lda import LDAKernels
    from lda_host import make_layouts
    rt = get_runtime()
    k = LDAKernels(rt)
    n = len(doc)
    lay, orig = make_layouts(doc, word, D, V)
    dev = {key: torch.from_numpy(v).to(rt.device) for key, v in lay.items()}
    _, _, wsd = k.plan(n, K)
    up = lambda a: None if a is None else torch.from_numpy(          # noqa: E731
        np.ascontiguousarray(a, dtype=np.float64)).to(rt.device)
    lse, ws = rt.empty(max(n, 1)), rt.empty(wsd)
    Ndk = torch.full((D, K), float('nan'), dtype=torch.float64, device=rt.device)
    Nvk = torch.full((V, K), float('nan'), dtype=torch.float64, device=rt.device)
    scal = torch.full((8,), float('nan'), dtype=torch.float64, device=rt.device)
    phi = torch.full((n, K), float('nan'), dtype=torch.float64, device=rt.device) \
        if want_phi else None
    lab = None
    if labels is not None:
        lab = torch.from_numpy(np.asarray(labels)[orig].astype(np.int32)).to(rt.device)
    rt.sync_stream()
    k.token_pass(n, D, V, K, dev, lab, up(et), up(ebt), 7, lse, ws, Ndk, Nvk, scal,
                 torch.from_numpy(orig).to(rt.device) if want_phi else None, phi)
    rt.synchronize()
    return (Ndk.cpu().numpy(), Nvk.cpu().numpy(), scal.cpu().numpy()[:3], lse.cpu().numpy()[:n],
            None if phi is None else phi.cpu().numpy(), orig)


def _check_against_restatement(doc, word, D, V, K, rs):
    """Count bound (u = 2^-53), derived in tests/test_lda_host.py: a responsibility exp(l - lse)
    is relative-exact to c u with c = 4 + 4 (lmax + log K) (roundings of the logit, of lse, of
    their difference, and of the three library calls at 1 u each), and a count adds at most
    `len` positive terms in order, (len - 1) u:  |error| <= (len + c) u * count, with len = the
    longest segment.  The device's exp / log are taken as 1 u like the host's."""
    from lda_host import restate, lda_host
    et = np.log(rs.dirichlet(np.ones(K), size=D))
    ebt = np.log(rs.dirichlet(np.ones(V), size=K)).T
    Ndk, Nvk, scal, lse, phi, orig = _device_pass(doc, word, D, V, K, et, ebt, want_phi=True)
    rphi, rlse, rN, rM = restate(doc, word, D, V, K, et, ebt)
    n = len(doc)
    lmax = float(np.abs(et).max() + np.abs(ebt).max())
    c = 4 + 4 * (lmax + np.log(K))
    seg = max(1, int(np.bincount(doc, minlength=D).max()) if n else 1,
              int(np.bincount(word, minlength=V).max()) if n else 1)
    errN = np.abs(Ndk - rN) / np.maximum(rN, 1e-300)
    errM = np.abs(Nvk - rM) / np.maximum(rM, 1e-300)
    print('K=%d n=%d: max count error %.3g u (Ndk), %.3g u (Nvk), bound %.3g u'
          % (K, n, float(errN.max() / U) if errN.size else 0,
             float(errM.max() / U) if errM.size else 0, seg + c))
    assert np.all(np.abs(Ndk - rN) <= (seg + c) * U * rN), (K, n)
    assert np.all(np.abs(Nvk - rM) <= (seg + c) * U * rM), (K, n)
    if n:
        np.testing.assert_allclose(phi, rphi.astype(np.float64), rtol=c * U, atol=0)
        np.testing.assert_allclose(lse, rlse.astype(np.float64)[orig], rtol=0,
                                   atol=4 * U * (lmax + np.log(K) + 1))
    # sum of lse: every term within its own bound above, then at most T additions inside a chunk,
    # chunks / 1024 per lane of the final workgroup and 4 + 6 levels of its tree
    T = lda_host().lda_chunk_tokens(n, K)
    adds = T + n / (T * 1024.0) + 10
    np.testing.assert_allclose(scal[0], float(rlse.sum()), rtol=0,
                               atol=n * 4 * U * (lmax + np.log(K) + 1)
                               + adds * U * float(np.abs(rlse).sum()))
    np.testing.assert_allclose(scal[1], float((rN * et).sum()), rtol=1e-12)
    np.testing.assert_allclose(scal[2], float((rM * ebt).sum()), rtol=1e-12)
    return Ndk, Nvk


@pytest.mark.parametrize('K', [1, 2, 3, 5, 8, 17, 32, 33, 64])
def test_token_pass_against_long_double(K):
    from lda_host import lda_host
    rs = np.random.RandomState(500 + K)
    D, V = 9, 13
    T = lda_host().lda_chunk_tokens(1000, K)
    for n in (T - 1, T, T + 1, 3 * T - 1, 3 * T, 3 * T + 1, 7 * T + 5):
        doc, word = rs.randint(D, size=n), rs.randint(V, size=n)
        _check_against_restatement(doc, word, D, V, K, rs)
    # one document holds every token (a segment over several chunks), one word most of them
    n = 9 * T + 2
    doc = np.full(n, 4)
    word = np.where(rs.rand(n) < 0.8, 7, rs.randint(V, size=n))
    Ndk, Nvk = _check_against_restatement(doc, word, D, V, K, rs)
    assert not Ndk[[0, 1, 2, 3, 5, 6, 7, 8]].any()          # empty documents: exact zeros
    unused = np.setdiff1d(np.arange(V), word)
    assert not Nvk[unused].any()


def test_token_pass_at_a_large_chunk_size():
    """n large enough for the 256-token chunk, K = 33 in a 64-lane group: chunk boundaries inside
    documents and words, a frequent word over hundreds of chunks."""
    from lda_host import lda_host
    rs = np.random.RandomState(9)
    K, D, V = 33, 300, 1000
    n = (1 << 18) + 1077
    assert lda_host().lda_chunk_tokens(n, K) == 256
    doc = rs.randint(D, size=n)
    word = rs.zipf(1.3, size=n) % V
    _check_against_restatement(doc, word, D, V, K, rs)


def test_bit_identity_and_permutation_invariance():
    rs = np.random.RandomState(77)
    K, D, V, n = 17, 40, 90, 5000
    doc, word = rs.randint(D, size=n), rs.randint(V, size=n)
    et = np.log(rs.dirichlet(np.ones(K), size=D))
    ebt = np.log(rs.dirichlet(np.ones(V), size=K)).T
    a = _device_pass(doc, word, D, V, K, et, ebt)
    b = _device_pass(doc, word, D, V, K, et, ebt)
    for x, y in zip(a[:4], b[:4]):
        np.testing.assert_array_equal(x, y)
    # the layouts are sorted by (document, word) and (word, document): ANY order of the input
    # tokens gives the same layouts, hence the same bits of both count tables and of sum lse
    perm = rs.permutation(n)
    c = _device_pass(doc[perm], word[perm], D, V, K, et, ebt)
    for x, y in zip(a[:4], c[:4]):
        np.testing.assert_array_equal(x, y)
    # the host build of the device header walks the same order: equal up to the library exp / log
    from lda_host import make_layouts, host_token_pass
    lay, _ = make_layouts(doc, word, D, V)
    h = host_token_pass(n, D, V, K, lay, None, et, ebt)
    np.testing.assert_allclose(a[0], h[0], rtol=1e-13)
    np.testing.assert_allclose(a[1], h[1], rtol=1e-13)


def test_edge_cases_on_the_device():
    K, D, V = 3, 4, 5
    et = np.log(np.full((D, K), 1.0 / K))
    ebt = np.log(np.full((V, K), 1.0 / V))
    Ndk, Nvk, scal, _, _, _ = _device_pass(np.zeros(0, dtype=np.int64),
                                           np.zeros(0, dtype=np.int64), D, V, K, et, ebt)
    assert not Ndk.any() and not Nvk.any() and not scal.any()
    doc, word = np.full(100, 2), np.arange(100) % 2
    et2 = et.copy()
    et2[:, 1] = -np.inf
    Ndk, Nvk, scal, lse, _, _ = _device_pass(doc, word, D, V, K, et2, ebt)
    assert np.all(Ndk[:, 1] == 0) and np.all(np.isfinite(Ndk)) and np.all(np.isfinite(lse))
    lab = np.arange(100) % 3
    Ndk, Nvk, scal, lse, phi, _ = _device_pass(doc, word, D, V, K, et, ebt, want_phi=True,
                                               labels=lab)
    np.testing.assert_array_equal(Ndk[2], [34, 33, 33])
    np.testing.assert_array_equal(phi, np.eye(3)[lab])
    assert scal[0] == 0 and not lse.any()
    # prior only: no word term
    Ndk, Nvk, scal, lse, phi, _ = _device_pass(doc, word, D, V, K, et, None, want_phi=True)
    np.testing.assert_allclose(phi, 1.0 / 3, rtol=1e-15)
    np.testing.assert_allclose(Nvk[:2], 50.0 / 3, rtol=1e-13)
    assert scal[2] == 0


def test_argument_checks():
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    lib, ctx = rt.lib, rt.ctx
    z = rt.zeros(4096)
    p = ctypes.c_void_p(z.data_ptr())
    args = [p] * 7 + [None, p, p, 7, p, p, p, p, p, None, None]
    assert lib.vmp_lda_token_pass(ctx, 0, 1, 1, 4, *args) == _lib.VMP_OK
    assert lib.vmp_lda_token_pass(ctx, -1, 1, 1, 4, *args) == _lib.VMP_ERR_INVALID
    assert lib.vmp_lda_token_pass(ctx, 0, 1, 1, 0, *args) == _lib.VMP_ERR_INVALID
    assert lib.vmp_lda_token_pass(ctx, 0, 1, 1, 65, *args) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_lda_token_pass(None, 0, 1, 1, 4, *args) == _lib.VMP_ERR_INVALID
    bad = list(args)
    bad[13] = None                                       # Ndk
    assert lib.vmp_lda_token_pass(ctx, 0, 1, 1, 4, *bad) == _lib.VMP_ERR_INVALID
    bad = list(args)
    bad[10] = 8                                          # phases
    assert lib.vmp_lda_token_pass(ctx, 0, 1, 1, 4, *bad) == _lib.VMP_ERR_INVALID
    bad = list(args)
    bad[17] = p                                          # phi without orig
    assert lib.vmp_lda_token_pass(ctx, 0, 1, 1, 4, *bad) == _lib.VMP_ERR_INVALID
    assert lib.vmp_lda_dirichlet(ctx, -1, 4, 4, 1, p, None, p, p, p, p) == _lib.VMP_ERR_INVALID
    assert lib.vmp_lda_dirichlet(ctx, 2, 4, 4, 1, None, None, p, p, p, p) == _lib.VMP_ERR_INVALID
    assert lib.vmp_lda_dot(ctx, -1, p, p, p, p) == _lib.VMP_ERR_INVALID
    assert lib.vmp_lda_dot(ctx, 4, None, p, p, p) == _lib.VMP_ERR_INVALID
    rt.synchronize()
    # the host validates the indices with the reference's errors
    from lda_models import build_lda
    m = build_lda(_mods(), np.array([0, 1, 1]), np.array([0, 5, 2]), 2, 5, 2)
    with pytest.raises(ValueError, match='Invalid category index'):
        m['topics'].update()


def test_dirichlet_rows_against_scipy():
    import torch
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.lda import LDAKernels
    from lda_host import dirichlet_rows
    rt = get_runtime()
    k = LDAKernels(rt)
    rs = np.random.RandomState(4)
    for rows, cols, transposed in ((300, 7, False), (5, 64, False), (6, 1000, True),
                                   (3, 65, True), (1, 1, False)):
        prior = rs.gamma(1.0, 1.0, size=(rows, cols)) + 0.01
        counts = rs.gamma(2.0, 3.0, size=(rows, cols)) * (rs.rand(rows, cols) < 0.7)
        store = (lambda a: np.ascontiguousarray(a.T)) if transposed else np.ascontiguousarray
        rs_, cs_ = (1, rows) if transposed else (cols, 1)
        dp, dc = [torch.from_numpy(store(a)).to(rt.device) for a in (prior, counts)]
        al, el = torch.empty_like(dp), torch.empty_like(dp)
        ws, out = rt.empty(max(rows, 1024)), rt.zeros(1)
        for cnt, ref_c in ((dc, counts), (None, None)):
            rt.sync_stream()
            k.dirichlet(rows, cols, rs_, cs_, dp, cnt, al, el, ws, out)
            ra, re, rb = dirichlet_rows(prior, ref_c)
            back = (lambda t: t.cpu().numpy().T) if transposed else (lambda t: t.cpu().numpy())
            np.testing.assert_allclose(back(al), ra, rtol=1e-15)
            np.testing.assert_allclose(back(el), re, rtol=1e-11, atol=1e-12)
            np.testing.assert_allclose(float(out.item()), rb, rtol=1e-10, atol=1e-9)


# -- the block at scale ---------------------------------------------------------------------------------
def test_memory_peak_is_linear_in_tokens():
    """2e6 tokens, V = 2e4: a tokens x V fp64 array would be 320 GB.  What the block may hold: the
    int64 indices and sort keys while the layouts are built (at most 12 token-sized int64 arrays
    alive at once: 96 B per token), the scratch of two device sorts (32 B per token), then the
    steady state of five int32 arrays, lse and the chunk partials (< 40 B per token) -- 256 B per
    token bounds all of it -- plus ten (D + V) x K tables of doubles."""
    import torch
    from bayespy_amd import nodes
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.plans.lda import LDAPlan
    n, D, V, K = 2000000, 20000, 20000, 16
    rs = np.random.RandomState(0)
    docs, corpus = rs.randint(D, size=n), rs.randint(V, size=n)
    p_topic = nodes.Dirichlet(np.ones(K), plates=(D,), name='p_topic')
    p_word = nodes.Dirichlet(np.ones(V), plates=(K,), name='p_word')
    topics = nodes.Categorical(nodes.Gate(docs, p_topic), plates=(n,), name='topics')
    words = nodes.Categorical(nodes.Gate(topics, p_word), name='words')
    words.observe(corpus)
    p_topic.initialize_from_random()
    p_word.initialize_from_random()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    Q = VB(words, topics, p_word, p_topic)
    assert isinstance(Q.plans[0], LDAPlan)
    Q.update(repeat=3, verbose=False)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    limit = 256 * n + 10 * 8 * (D + V) * K
    print('peak %.1f MB, limit %.1f MB, tokens x V fp64 = %.0f GB'
          % (peak / 1e6, limit / 1e6, 8.0 * n * V / 1e9))
    assert peak <= limit
    assert 8.0 * n * V > 100 * peak
    assert np.all(np.isfinite(Q.L[:3])) and Q.L[2] > Q.L[1] > Q.L[0]
    # the counts add up to the tokens
    plan = Q.plans[0]
    np.testing.assert_allclose(float(plan.Ndk.sum().item()), n, rtol=1e-12)
    np.testing.assert_allclose(float(plan.Nvk.sum().item()), n, rtol=1e-12)


def test_save_load_and_responsibilities(golden_dir, tmp_path):
    from lda_models import run_lda_cases
    from lda_host import restate
    g, gin = _golden(golden_dir)
    Q = run_lda_cases(_mods(), gin, only=('doc',), moments_of=())['doc_plan']
    plan = Q.plans[0]
    # topics.get_moments(): the tables of the last topics update, not the present ones
    et, ebt = plan.used_theta.cpu().numpy(), plan.used_beta_t.cpu().numpy()
    rphi = restate(gin['doc_docs'], gin['doc_words'], 7, 30, 4, et, ebt)[0]
    phi = Q['topics'].get_moments()[0]
    assert phi.shape == (400, 4)
    np.testing.assert_allclose(phi, rphi.astype(np.float64), rtol=1e-13)
    np.testing.assert_allclose(phi, g['doc_topics_u0'], **MOM_TOL)
    fn = str(tmp_path / 'lda.ckpt')
    Q.save(filename=fn)
    L5 = Q.L[:5].copy()
    Q.update(repeat=2, verbose=False)
    L7 = Q.L[:7].copy()
    Q.load(filename=fn)
    assert Q.iter == 5
    np.testing.assert_array_equal(Q.L[:5], L5)
    np.testing.assert_array_equal(Q['topics'].get_moments()[0], phi)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:7], L7)
    # autosave goes the same way
    Q.set_autosave(str(tmp_path / 'auto.ckpt'), iterations=1)
    Q.update(repeat=1, verbose=False)
    assert os.path.exists(str(tmp_path / 'auto.ckpt'))


def test_first_half_of_the_doc_example():
    """doc/source/examples/lda.rst through ``Q.update(repeat=...)`` with only the import lines
    changed (the data are drawn with NumPy: sampling is not part of the model)."""
    import numpy as np
    from bayespy_amd import nodes
    rs = np.random.RandomState(1)
    n_documents, n_words, n_vocabulary, n_topics = 10, 10000, 100, 5
    word_documents = rs.randint(n_documents, size=n_words)
    corpus = rs.randint(n_vocabulary, size=n_words)
    p_topic = nodes.Dirichlet(np.ones(n_topics),
                              plates=(n_documents,),
                              name='p_topic')
    p_word = nodes.Dirichlet(np.ones(n_vocabulary),
                             plates=(n_topics,),
                             name='p_word')
    from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments
    document_indices = nodes.Constant(CategoricalMoments(n_documents), word_documents,
                                      name='document_indices')
    topics = nodes.Categorical(nodes.Gate(document_indices, p_topic),
                               plates=(len(corpus),),
                               name='topics')
    words = nodes.Categorical(nodes.Gate(topics, p_word),
                              name='words')
    words.observe(corpus)
    p_topic.initialize_from_random()
    p_word.initialize_from_random()
    from bayespy_amd.inference import VB
    Q = VB(words, topics, p_word, p_topic, document_indices)
    Q.update(repeat=20, verbose=False)
    from bayespy_amd.inference.plans.lda import LDAPlan
    assert isinstance(Q.plans[0], LDAPlan)
    assert Q.iter >= 2 and np.all(np.diff(Q.L[:Q.iter]) > -1e-6)
    assert Q['p_word'].get_moments()[0].shape == (n_topics, n_vocabulary)
