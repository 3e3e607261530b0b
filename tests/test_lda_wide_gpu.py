"""GPU: the wide-topic form of the fused latent-Dirichlet-allocation block (inference/plans/
lda_wide.py, csrc/vmp_lda_wide.hip, 65 <= K <= 1024) -- ``vmp_lda_wide_token_pass`` through the C ABI
against the host build of its header and a long-double restatement at every register count, at
sizes around the chunk, with segments over several chunks, empty segments, fixed labels, the
prior-only forms, phi on request and an all -inf token; both traces of tests/golden/lda_wide.npz
(live reference) through ``VB(..., engine='fused+topics')``, the generic engine on the same model,
bit-identity, the memory peak and save / load."""
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

TRACE_TOL = dict(rtol=1e-8, atol=1e-8)       # tests/test_lda_gpu.py: scalars and traces
MOM_TOL = dict(rtol=MOM_RTOL, atol=1e-9)     # tests/test_lda_gpu.py: moments
HOST_RTOL = 1e-13                            # tests/test_lda_gpu.py: counts against the host build
U = 2.0 ** -53


def _mods(**kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments
    from lda_wide_models import plan_params
    kw.setdefault('engine', 'fused+topics')
    return dict(nodes=nodes, VB=VB, CategoricalMoments=CategoricalMoments, vb_kwargs=kw,
                params=plan_params)


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'lda_wide.npz'))
    return g, {k[3:]: g[k] for k in g.files if k.startswith('in_')}


# -- the token pass through the C ABI -------------------------------------------------------------------
def _device_pass(doc, word, D, V, K, et, ebt, want_phi=False, labels=None):
    import torch
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.lda_wide import WideLDAKernels
    from lda_host import make_layouts
    rt = get_runtime()
    k = WideLDAKernels(rt)
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


def _host_pass(doc, word, D, V, K, et, ebt, want_phi=False, labels=None):
    from lda_host import make_layouts
    from lda_wide_host import host_token_pass
    lay, orig = make_layouts(doc, word, D, V)
    lab = None if labels is None else np.asarray(labels)[orig].astype(np.int32)
    return host_token_pass(len(doc), D, V, K, lay, lab, et, ebt, orig=orig, want_phi=want_phi)


def _tables(rs, K, D, V):
    return (np.log(rs.dirichlet(np.ones(K), size=D)), np.log(rs.dirichlet(np.ones(V), size=K)).T)


def _check(doc, word, D, V, K, et, ebt):
    """The rule of tests/test_lda_gpu.py for the narrow pass, on the same quantities: against the
    long-double restatement a responsibility within c u, c = 4 + 4 (lmax + log K), a count within
    (len + c) u of itself with len = the longest segment, lse within 4 u (lmax + log K + 1), the
    sum of lse by its additions, the dot products to 1e-12; against the host build of the device
    header, which adds in the same order, the counts to 1e-13.  The sum of up to 1024 exponentials
    rounds at most (R - 1) + 6 <= 21 times per path, inside the 4 (lmax + log K) > 33 u of that rule
    (tests/test_lda_wide_host.py); every figure is printed before it is asserted."""
    from lda_host import restate
    from lda_wide_host import lda_wide_host
    Ndk, Nvk, scal, lse, phi, orig = _device_pass(doc, word, D, V, K, et, ebt, want_phi=True)
    rphi, rlse, rN, rM = restate(doc, word, D, V, K, et, ebt)
    h = _host_pass(doc, word, D, V, K, et, ebt, want_phi=True)
    n = len(doc)
    fin = lambda a: a[np.isfinite(a)]                                       # noqa: E731
    lmax = float(np.abs(fin(et)).max() + (np.abs(fin(ebt)).max() if ebt is not None else 0.0))
    c = 4 + 4 * (lmax + np.log(K))
    seg = max(1, int(np.bincount(doc, minlength=D).max()), int(np.bincount(word, minlength=V).max()))
    rN64, rM64 = rN.astype(np.float64), rM.astype(np.float64)
    errN = np.abs(Ndk - rN) / np.maximum(rN, 1e-300)
    errM = np.abs(Nvk - rM) / np.maximum(rM, 1e-300)
    errP = np.abs(phi - rphi) / np.maximum(rphi, 1e-300)
    errL = np.abs(lse - rlse[orig])
    hN = np.abs(Ndk - h[0]) / np.maximum(np.abs(h[0]), 1e-300)
    hM = np.abs(Nvk - h[1]) / np.maximum(np.abs(h[1]), 1e-300)
    print('K=%d n=%d: against long double: counts %.3g u (Ndk) %.3g u (Nvk), bound %.3g u; phi '
          '%.3g u, bound %.3g u; lse %.3g u, bound %.3g u; against the host build: counts %.3g u '
          '(Ndk) %.3g u (Nvk), bound %.3g u'
          % (K, n, float(errN.max() / U), float(errM.max() / U), seg + c, float(errP.max() / U), c,
             float(errL.max() / U), 4 * (lmax + np.log(K) + 1), float(hN.max() / U),
             float(hM.max() / U), HOST_RTOL / U))
    assert np.all(np.abs(Ndk - rN) <= (seg + c) * U * rN), (K, n)
    assert np.all(np.abs(Nvk - rM) <= (seg + c) * U * rM), (K, n)
    np.testing.assert_allclose(phi, rphi.astype(np.float64), rtol=c * U, atol=0)
    np.testing.assert_allclose(lse, rlse.astype(np.float64)[orig], rtol=0,
                               atol=4 * U * (lmax + np.log(K) + 1))
    T = lda_wide_host().lda_wide_chunk_tokens(n)
    adds = T + n / (T * 1024.0) + 10
    np.testing.assert_allclose(scal[0], float(rlse.sum()), rtol=0,
                               atol=n * 4 * U * (lmax + np.log(K) + 1)
                               + adds * U * float(np.abs(rlse).sum()))
    with np.errstate(invalid='ignore'):
        np.testing.assert_allclose(scal[1], float(np.nansum(rN64 * et)), rtol=1e-12)
        if ebt is None:
            assert scal[2] == 0
        else:
            np.testing.assert_allclose(scal[2], float(np.nansum(rM64 * ebt)), rtol=1e-12)
    np.testing.assert_allclose(Ndk, h[0], rtol=HOST_RTOL, atol=0)
    np.testing.assert_allclose(Nvk, h[1], rtol=HOST_RTOL, atol=0)
    np.testing.assert_allclose(phi, h[4], rtol=HOST_RTOL, atol=0)
    return Ndk, Nvk


@pytest.mark.parametrize('K', [65, 128, 129, 1000, 1024])
def test_token_pass_against_host_build_and_long_double(K):
    """Every register count (2, 2, 4, 16, 16), each with a partly filled last register or, at 128 and
    1024, a full one; n around the chunk; then one document and one word over seven chunks with
    empty segments first, in the middle and last."""
    from lda_wide_host import lda_wide_host
    rs = np.random.RandomState(500 + K)
    D, V = 9, 13
    T = lda_wide_host().lda_wide_chunk_tokens(1000)
    for n in (1, T - 1, T, T + 1, 5 * T + 3):
        doc, word = rs.randint(D, size=n), rs.randint(V, size=n)
        _check(doc, word, D, V, K, *_tables(rs, K, D, V))
    n = 9 * T + 2
    doc = np.where(rs.rand(n) < 0.8, 4, rs.choice([1, 6], size=n))
    word = np.where(rs.rand(n) < 0.8, 7, rs.choice([2, 11], size=n))
    assert (doc == 4).sum() > 3 * T and (word == 7).sum() > 3 * T
    Ndk, Nvk = _check(doc, word, D, V, K, *_tables(rs, K, D, V))
    assert not Ndk[[0, 2, 3, 5, 7, 8]].any()                # empty documents: exact zeros
    assert not Nvk[[0, 1, 3, 4, 5, 6, 8, 9, 10, 12]].any()
    assert Ndk[[1, 4, 6]].sum() > 0 and abs(Ndk.sum() - n) < 1e-9 * n


def test_token_pass_at_the_largest_chunk_size():
    """n large enough for the 256-token chunk (a function of n alone), not a multiple of it: chunk
    boundaries inside documents and words, a frequent word over hundreds of chunks.  Against the host
    build, which walks the same order."""
    from lda_wide_host import lda_wide_host
    rs = np.random.RandomState(9)
    K, D, V = 65, 300, 1000
    n = (1 << 18) + 1077
    assert lda_wide_host().lda_wide_chunk_tokens(n) == 256
    doc = rs.randint(D, size=n)
    word = rs.zipf(1.3, size=n) % V
    et, ebt = _tables(rs, K, D, V)
    Ndk, Nvk, scal, lse, _, _ = _device_pass(doc, word, D, V, K, et, ebt)
    h = _host_pass(doc, word, D, V, K, et, ebt)
    np.testing.assert_allclose(Ndk, h[0], rtol=HOST_RTOL, atol=0)
    np.testing.assert_allclose(Nvk, h[1], rtol=HOST_RTOL, atol=0)
    np.testing.assert_allclose(lse, h[3], rtol=HOST_RTOL, atol=0)
    np.testing.assert_allclose(scal, h[2], rtol=1e-12)
    np.testing.assert_allclose(float(Ndk.sum()), n, rtol=1e-12)


def test_fixed_labels_prior_only_and_phi_in_the_callers_order():
    rs = np.random.RandomState(21)
    K, D, V, n = 130, 5, 7, 83
    doc, word = rs.randint(D, size=n), rs.randint(V, size=n)
    et, ebt = _tables(rs, K, D, V)
    # fixed labels, on both sides of lane 63 and in the partly filled last register
    lab = rs.randint(K, size=n)
    lab[:4] = [0, 63, 64, K - 1]
    Ndk, Nvk, scal, lse, phi, _ = _device_pass(doc, word, D, V, K, et, ebt, want_phi=True,
                                               labels=lab)
    np.testing.assert_array_equal(phi, np.eye(K)[lab])
    wantD, wantV = np.zeros((D, K)), np.zeros((V, K))
    np.add.at(wantD, (doc, lab), 1.0)
    np.add.at(wantV, (word, lab), 1.0)
    np.testing.assert_array_equal(Ndk, wantD)
    np.testing.assert_array_equal(Nvk, wantV)
    assert scal[0] == 0 and not lse.any()
    # prior only: pass A without the gathered table, pass B without the kept one
    Ndk, Nvk = _check(doc, word, D, V, K, et, None)
    # phi in the caller's order: the tokens are not sorted, row i is token i
    from lda_host import restate
    phi = _device_pass(doc, word, D, V, K, et, ebt, want_phi=True)[4]
    rphi = restate(doc, word, D, V, K, et, ebt)[0]
    np.testing.assert_allclose(phi, rphi.astype(np.float64), rtol=HOST_RTOL)
    assert np.any(np.diff(doc) < 0)


def test_an_all_minus_inf_token_gives_nan_in_its_outputs_only():
    K, D, V = 129, 4, 5
    rs = np.random.RandomState(2)
    et, ebt = _tables(rs, K, D, V)
    ebt[1] = -np.inf
    et[:, [3, 70]] = -np.inf                     # topics with -inf logits: exact zeros, no NaN
    doc, word = np.array([0, 0, 1, 3, 3]), np.array([0, 1, 0, 2, 2])
    Ndk, Nvk, scal, lse, phi, orig = _device_pass(doc, word, D, V, K, et, ebt, want_phi=True)
    assert np.isnan(phi[1]).all() and np.isfinite(phi[[0, 2, 3, 4]]).all()
    assert not phi[[0, 2, 3, 4]][:, [3, 70]].any()
    assert np.isnan(lse[list(orig).index(1)]) and np.isnan(lse).sum() == 1
    assert np.isnan(Ndk[0]).all() and np.isfinite(Ndk[[1, 2, 3]]).all() and not Ndk[2].any()
    assert np.isnan(Nvk[1]).all() and np.isfinite(Nvk[[0, 2, 3, 4]]).all()
    assert np.isnan(scal[0])
    h = _host_pass(doc, word, D, V, K, et, ebt, want_phi=True)
    np.testing.assert_allclose(phi, h[4], rtol=HOST_RTOL, equal_nan=True)


def test_bit_identity_and_permutation_invariance():
    rs = np.random.RandomState(77)
    K, D, V, n = 257, 40, 90, 5000
    doc, word = rs.randint(D, size=n), rs.randint(V, size=n)
    et, ebt = _tables(rs, K, D, V)
    a = _device_pass(doc, word, D, V, K, et, ebt)
    b = _device_pass(doc, word, D, V, K, et, ebt)
    for x, y in zip(a[:4], b[:4]):
        np.testing.assert_array_equal(x, y)
    perm = rs.permutation(n)
    c = _device_pass(doc[perm], word[perm], D, V, K, et, ebt)
    for x, y in zip(a[:4], c[:4]):
        np.testing.assert_array_equal(x, y)
    h = _host_pass(doc, word, D, V, K, et, ebt)
    np.testing.assert_allclose(a[0], h[0], rtol=HOST_RTOL)
    np.testing.assert_allclose(a[1], h[1], rtol=HOST_RTOL)


def test_argument_checks_and_the_narrow_limit():
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    lib, ctx = rt.lib, rt.ctx
    z = rt.zeros(8192)
    p = ctypes.c_void_p(z.data_ptr())
    args = [p] * 7 + [None, p, p, 7, p, p, p, p, p, None, None]
    # the narrow pass stops where it stopped
    assert lib.vmp_lda_token_pass(ctx, 0, 1, 1, 64, *args) == _lib.VMP_OK
    assert lib.vmp_lda_token_pass(ctx, 0, 1, 1, 65, *args) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_lda_wide_token_pass(ctx, 0, 1, 1, 65, *args) == _lib.VMP_OK
    assert lib.vmp_lda_wide_token_pass(ctx, 0, 1, 1, 1024, *args) == _lib.VMP_OK
    assert lib.vmp_lda_wide_token_pass(ctx, 0, 1, 1, 64, *args) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_lda_wide_token_pass(ctx, 0, 1, 1, 1025, *args) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_lda_wide_token_pass(ctx, -1, 1, 1, 70, *args) == _lib.VMP_ERR_INVALID
    assert lib.vmp_lda_wide_token_pass(ctx, 0, 1, 1, 0, *args) == _lib.VMP_ERR_INVALID
    assert lib.vmp_lda_wide_token_pass(None, 0, 1, 1, 70, *args) == _lib.VMP_ERR_INVALID
    bad = list(args)
    bad[13] = None                                       # Ndk
    assert lib.vmp_lda_wide_token_pass(ctx, 0, 1, 1, 70, *bad) == _lib.VMP_ERR_INVALID
    bad = list(args)
    bad[10] = 8                                          # phases
    assert lib.vmp_lda_wide_token_pass(ctx, 0, 1, 1, 70, *bad) == _lib.VMP_ERR_INVALID
    bad = list(args)
    bad[17] = p                                          # phi without orig
    assert lib.vmp_lda_wide_token_pass(ctx, 0, 1, 1, 70, *bad) == _lib.VMP_ERR_INVALID
    rt.synchronize()
    # n = 0 leaves zeros
    Ndk, Nvk, scal, _, _, _ = _device_pass(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64),
                                           3, 4, 70, np.zeros((3, 70)), np.zeros((4, 70)))
    assert not Ndk.any() and not Nvk.any() and not scal.any()


# -- the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['k70', 'k130'])
def test_fixture_trace_on_the_wide_form(golden_dir, tag):
    from lda_wide_models import run_wide_case, SWEEPS
    from bayespy_amd.inference.plans.lda_wide import WideLDAPlan
    g, gin = _golden(golden_dir)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        res = run_wide_case(_mods(), gin, tag)
    assert not [str(w.message) for w in rec
                if 'engine' in str(w.message) or 'block' in str(w.message)]
    plans = res[tag + '_plan'].plans
    assert len(plans) == 1 and type(plans[0]) is WideLDAPlan
    checked = 0
    for k, v in res.items():
        if k.endswith(('_plan', '_model')):
            continue
        assert v.shape == g[k].shape and v.shape[0] == SWEEPS
        np.testing.assert_allclose(v, g[k], err_msg=k,
                                   **(MOM_TOL if '_alpha_' in k else TRACE_TOL))
        checked += 1
    assert checked == 1 + 4 + 2


def _random_model(engine, K=130, n=2000, D=20, V=50, seed=5):
    from lda_models import build_lda
    from lda_wide_models import plan_params
    rs = np.random.RandomState(seed)
    docs, words = rs.randint(D, size=n), rs.randint(V, size=n)
    theta0, beta0 = rs.dirichlet(np.ones(K), size=D), rs.dirichlet(np.ones(V), size=K)
    mods = _mods(engine=engine)
    m = build_lda(mods, docs, words, D, V, K)
    m['p_topic'].initialize_from_value(theta0)
    m['p_word'].initialize_from_value(beta0)
    Q = mods['VB'](m['words'], m['topics'], m['p_word'], m['p_topic'], engine=engine)
    Q.ignore_bound_checks = True
    return Q, m, plan_params


def test_against_the_generic_engine():
    from bayespy_amd.inference.plans.generic import GenericPlan
    from bayespy_amd.inference.plans.lda_wide import WideLDAPlan
    Qw, mw, _ = _random_model('fused+topics')
    Qg, mg, _ = _random_model('generic')
    assert type(Qw.plans[0]) is WideLDAPlan and isinstance(Qg.plans[0], GenericPlan)
    Qw.update(repeat=3, verbose=False)
    Qg.update(repeat=3, verbose=False)
    np.testing.assert_allclose(Qw.L[:3], Qg.L[:3], **TRACE_TOL)
    for nm in ('words', 'topics', 'p_word', 'p_topic'):
        np.testing.assert_allclose(Qw.l[mw[nm]][:3], Qg.l[mg[nm]][:3], err_msg=nm, **TRACE_TOL)
    for nm in ('topics', 'p_word', 'p_topic'):
        np.testing.assert_allclose(mw[nm].get_moments()[0], mg[nm].get_moments()[0], err_msg=nm,
                                   **MOM_TOL)


def test_two_runs_give_identical_bits():
    out = []
    for _ in range(2):
        Q, m, params = _random_model('fused+topics')
        Q.update(repeat=3, verbose=False)
        out.append((np.array(Q.L[:3]),) + tuple(np.array(a) for a in params(Q, m))
                   + (m['topics'].get_moments()[0],))
    for x, y in zip(*out):
        np.testing.assert_array_equal(x, y)


def test_save_load_mid_run(tmp_path):
    Q, m, params = _random_model('fused+topics')
    Q.update(repeat=2, verbose=False)
    fn = str(tmp_path / 'lda_wide.ckpt')
    Q.save(filename=fn)
    phi = m['topics'].get_moments()[0]
    Q.update(repeat=2, verbose=False)
    L4 = Q.L[:4].copy()
    a4 = [np.array(a) for a in params(Q, m)]
    Q.load(filename=fn)
    assert Q.iter == 2
    np.testing.assert_array_equal(m['topics'].get_moments()[0], phi)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:4], L4)
    for x, y in zip(a4, params(Q, m)):
        np.testing.assert_array_equal(x, y)
    # a fresh model of the same sizes continues from the file as well
    Q2, m2, _ = _random_model('fused+topics')
    Q2.load(filename=fn)
    Q2.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q2.L[:4], L4)


def test_no_tokens_by_topics_array_is_held():
    """2e5 tokens, K = 256: a tokens x K fp64 array is 410 MB.  What the plan may hold is the bound
    of tests/test_lda_gpu.py: 256 B per token for the indices, their sort and the chunk partials,
    plus ten (D + V) x K tables of doubles."""
    import torch
    from bayespy_amd.inference.plans.lda_wide import WideLDAPlan
    n, D, V, K = 200000, 2000, 2000, 256
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    Q, m, _ = _random_model('fused+topics', K=K, n=n, D=D, V=V)
    assert type(Q.plans[0]) is WideLDAPlan
    Q.update(repeat=3, verbose=False)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    limit = 256 * n + 10 * 8 * (D + V) * K
    print('peak %.1f MB, limit %.1f MB, tokens x K fp64 = %.0f MB'
          % (peak / 1e6, limit / 1e6, 8.0 * n * K / 1e6))
    assert peak <= limit < 8.0 * n * K
    assert np.all(np.isfinite(Q.L[:3])) and Q.L[2] > Q.L[1] > Q.L[0]
    plan = Q.plans[0]
    np.testing.assert_allclose(float(plan.Ndk.sum().item()), n, rtol=1e-12)
    np.testing.assert_allclose(float(plan.Nvk.sum().item()), n, rtol=1e-12)
