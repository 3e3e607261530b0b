"""GPU: the fused latent-Dirichlet-allocation block with learnt concentrations (inference/plans/
lda_hyper.py, csrc/vmp_lda_hyper.hip) -- ``vmp_lda_concentration_stats`` through the C ABI against a
long-double restatement under the rule of DESIGN.md 4.14 at sizes around the chunk, every register
count and both stride forms, a row whose alpha spans 1e-3 .. 1e6, a NaN entry and bit identity;
``vmp_lda_prior_fill`` in both forms; the traces of tests/golden/lda_hyper.npz (live reference)
through ``engine='fused+topics+hyper'``, the same models on the generic engine, save / load and the
memory peak against the constant-prior block."""
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

# what tests/test_hyperparameters_gpu.py holds the Concentration node to on the generic engine
BOUND_TOL = dict(rtol=1e-9, atol=0)
MOM_TOL = dict(rtol=1e-7, atol=1e-9)
CASES = ['topic', 'word', 'both', 'pair', 'first', 'k70']
T = 16                                  # memory rows per chunk at these sizes


def _mods(**kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments
    from lda_hyper_models import plan_params, generic_params
    kw.setdefault('engine', 'fused+topics+hyper')
    return dict(nodes=nodes, VB=VB, CategoricalMoments=CategoricalMoments, vb_kwargs=kw,
                params=generic_params if kw['engine'] == 'generic' else plan_params)


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'lda_hyper.npz'))
    return g, {k[3:]: g[k] for k in g.files if k.startswith('in_')}


# -- the raw entries through the C ABI ------------------------------------------------------------------
def _device_stats(alpha, elog, transposed):
    import torch
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.lda_hyper import HyperLDAKernels
    from lda_hyper_host import _memory
    rt = get_runtime()
    k = HyperLDAKernels(rt)
    rows, cols = alpha.shape
    rs, cs = (1, rows) if transposed else (cols, 1)
    up = lambda a: torch.from_numpy(_memory(a, transposed)).to(rt.device)     # noqa: E731
    a, e = (up(alpha), up(elog)) if rows else (rt.empty(1), rt.empty(1))
    ws = torch.full((max(k.stats_ws(rows, cols, max(rs, 1), max(cs, 1)), 1),), float('nan'),
                    dtype=torch.float64, device=rt.device)
    S = torch.full((cols,), float('nan'), dtype=torch.float64, device=rt.device)
    q = torch.full((1,), float('nan'), dtype=torch.float64, device=rt.device)
    rt.sync_stream()
    k.stats(rows, cols, max(rs, 1), max(cs, 1), a, e, ws, S, q)
    rt.synchronize()
    return S.cpu().numpy(), float(q.cpu().numpy()[0])


@pytest.mark.parametrize('cols', [1, 2, 63, 64, 65, 130, 1024])
def test_stats_row_major_against_long_double(cols):
    """The rule of DESIGN.md 4.14 (8 x the float64 deviation from long double, floor 4 ulp) on S
    and qterm at every shape; the three figures are printed per shape (the worst ratios of error
    to allowance are recorded in DESIGN.md 4.13b)."""
    from lda_hyper_host import lda_hyper_host, compare, make_tables
    assert lda_hyper_host().lda_hyper_chunk_rows(100) == T
    rs = np.random.RandomState(500 + cols)
    bad = []
    for rows in (0, 1, T - 1, T, T + 1, 3 * T + 5):
        for kind in ('plain', 'spread'):
            alpha, elog = make_tables(rs, rows, cols, kind)
            S, q = _device_stats(alpha, elog, False)
            bad += [(rows, kind) + b for b in
                    compare(S, q, alpha, elog, label='rows %d cols %d %s' % (rows, cols, kind))]
            if rows == 0:
                assert not S.any() and q == 0.0
    assert not bad, bad


@pytest.mark.parametrize('rows', [1, 64, 65, 1024])
def test_stats_transposed_against_long_double(rows):
    """The rule of DESIGN.md 4.14 (8 x the float64 deviation from long double, floor 4 ulp) on S
    and qterm at every shape; the three figures are printed per shape (the worst ratios of error
    to allowance are recorded in DESIGN.md 4.13b)."""
    from lda_hyper_host import compare, make_tables
    rs = np.random.RandomState(600 + rows)
    bad = []
    for cols in (2, T - 1, T, T + 1, 3 * T + 5):
        for kind in ('plain', 'spread'):
            alpha, elog = make_tables(rs, rows, cols, kind)
            S, q = _device_stats(alpha, elog, True)
            bad += [(cols, kind) + b for b in
                    compare(S, q, alpha, elog, label='T rows %d cols %d %s' % (rows, cols, kind))]
    assert not bad, bad


def test_stats_nan_propagates_and_two_calls_give_the_same_bits():
    from lda_hyper_host import make_tables
    rs = np.random.RandomState(7)
    alpha, elog = make_tables(rs, 40, 70)
    for tr in (False, True):
        S, q = _device_stats(alpha, elog, tr)
        S2, q2 = _device_stats(alpha, elog, tr)
        assert np.array_equal(S, S2) and q == q2 and np.isfinite(q) and np.all(np.isfinite(S))
        a = alpha.copy()
        a[17, 66] = np.nan
        S3, q3 = _device_stats(a, elog, tr)
        assert np.isnan(q3) and np.array_equal(S3, S)
        e = elog.copy()
        e[17, 66] = np.nan
        S4, q4 = _device_stats(alpha, e, tr)
        assert np.isnan(q4) and np.isnan(S4[66]) and np.isnan(S4).sum() == 1


def test_stats_argument_checks():
    import torch
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime, ptr
    rt = get_runtime()
    lib, ctx = rt.lib, rt.ctx
    x = rt.zeros(64)
    rt.sync_stream()
    ok = (ctx, 4, 5, 5, 1, ptr(x), ptr(x), ptr(x), ptr(x), ptr(x))
    assert lib.vmp_lda_concentration_stats(*ok) == _lib.VMP_OK
    for i in (5, 6, 7, 8, 9):
        bad = list(ok)
        bad[i] = None
        assert lib.vmp_lda_concentration_stats(*bad) == _lib.VMP_ERR_INVALID, i
    for i, v in ((1, -1), (2, 0), (3, 0), (4, -1)):
        bad = list(ok)
        bad[i] = v
        assert lib.vmp_lda_concentration_stats(*bad) == _lib.VMP_ERR_INVALID, (i, v)
    bad = list(ok)
    bad[3] = 6
    assert lib.vmp_lda_concentration_stats(*bad) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_lda_prior_fill(ctx, 4, 5, 5, 1, None, ptr(x)) == _lib.VMP_ERR_INVALID
    assert lib.vmp_lda_prior_fill(ctx, -1, 5, 5, 1, ptr(x), ptr(x)) == _lib.VMP_ERR_INVALID
    assert lib.vmp_lda_prior_fill(ctx, 0, 5, 5, 1, None, None) == _lib.VMP_OK
    torch.cuda.synchronize()


@pytest.mark.parametrize('rows,cols', [(1, 1), (7, 5), (300, 70), (70, 300)])
def test_prior_fill_in_both_forms(rows, cols):
    import torch
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.lda_hyper import HyperLDAKernels
    rt = get_runtime()
    k = HyperLDAKernels(rt)
    a = np.random.RandomState(rows).gamma(2.0, size=cols)
    for rs, cs, shape in ((cols, 1, (rows, cols)), (1, rows, (cols, rows))):
        pad = 3
        t = torch.full((rows * cols + pad,), -1.0, dtype=torch.float64, device=rt.device)
        rt.sync_stream()
        k.prior_fill(rows, cols, rs, cs, torch.from_numpy(a).to(rt.device), t)
        rt.synchronize()
        got = t.cpu().numpy()
        assert np.all(got[rows * cols:] == -1.0)
        table = got[:rows * cols].reshape(shape)
        np.testing.assert_array_equal(table if cs == 1 else table.T, np.broadcast_to(a, (rows, cols)))


# -- the model ----------------------------------------------------------------------------------------
def _check(res, g, bound_tol=BOUND_TOL, mom_tol=MOM_TOL):
    n = 0
    for k, v in res.items():
        if k.endswith(('_plan', '_model')):
            continue
        want = g[k]
        is_bound = k.endswith('_L') or '_l_' in k
        with np.errstate(all='ignore'):
            dev = float(np.max(np.abs(v - want) / np.maximum(np.abs(want), 1e-300)))
        print('%-28s largest relative deviation %.3e' % (k, dev))
        np.testing.assert_allclose(v, want, err_msg=k, **(bound_tol if is_bound else mom_tol))
        n += 1
    return n


@pytest.mark.parametrize('tag', CASES)
def test_fixture_trace_on_the_device(golden_dir, tag):
    from lda_hyper_models import run_hyper_case, HYPER_CASES
    g, gin = _golden(golden_dir)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_hyper_case(_mods(), gin, tag)
    want = 'WideHyperLDAPlan' if HYPER_CASES[tag][0] > 64 else 'HyperLDAPlan'
    assert type(res[tag + '_plan'].plans[0]).__name__ == want
    n_conc = sum(r is not None for r in HYPER_CASES[tag][1:3])
    assert _check(res, g) == 1 + 4 + 2 + 5 * n_conc


@pytest.mark.parametrize('tag', CASES)
def test_same_models_on_the_generic_engine(golden_dir, tag):
    from lda_hyper_models import run_hyper_case
    from bayespy_amd.inference.plans.generic import GenericPlan
    g, gin = _golden(golden_dir)
    res = run_hyper_case(_mods(engine='generic'), gin, tag)
    assert isinstance(res[tag + '_plan'].plans[0], GenericPlan)
    _check(res, g)


def test_save_load_mid_run(golden_dir, tmp_path):
    from lda_hyper_models import run_hyper_case
    _, gin = _golden(golden_dir)
    res = run_hyper_case(_mods(), gin, 'both', sweeps=2)
    Q, m = res['both_plan'], res['both_model']
    fn = str(tmp_path / 'lda_hyper.ckpt')
    Q.save(filename=fn)
    Q.update(repeat=2, verbose=False)
    L4 = Q.L[:4].copy()
    a4 = m['conc_word'].get_moments()[0].copy()
    Q.load(filename=fn)
    assert Q.iter == 2
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:4], L4)
    np.testing.assert_array_equal(m['conc_word'].get_moments()[0], a4)
    # a fresh model of the same sizes continues from the file as well
    res2 = run_hyper_case(_mods(), gin, 'both', sweeps=0)
    Q2 = res2['both_plan']
    Q2.load(filename=fn)
    Q2.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q2.L[:4], L4)


def test_peak_memory_against_the_constant_prior_block():
    """n = 2e4 tokens, D = V = 2000, K = 64.  What the learnt concentrations may add to the peak of the
    constant-prior block: per concentration five cols-vectors and the workspace of the pass (chunk
    partials), no table and nothing token-sized -- bounded here by one (D + V) x K table of doubles,
    a tenth of what the block holds."""
    import torch
    from bayespy_amd import nodes
    from bayespy_amd.inference import VB
    n, D, V, K = 20000, 2000, 2000, 64
    rs = np.random.RandomState(5)
    docs, words = rs.randint(D, size=n), rs.randint(V, size=n)
    th0, be0 = rs.dirichlet(np.ones(K), size=D), rs.dirichlet(np.ones(V), size=K)

    def run(learnt):
        a = nodes.DirichletConcentration(K, name='ca') if learnt else np.ones(K)
        b = nodes.DirichletConcentration(V, name='cb') if learnt else np.ones(V)
        p_topic = nodes.Dirichlet(a, plates=(D,), name='p_topic')
        p_word = nodes.Dirichlet(b, plates=(K,), name='p_word')
        topics = nodes.Categorical(nodes.Gate(docs, p_topic), plates=(n,), name='topics')
        w = nodes.Categorical(nodes.Gate(topics, p_word), name='words')
        w.observe(words)
        p_topic.initialize_from_value(th0)
        p_word.initialize_from_value(be0)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        extra = [a, b] if learnt else []
        Q = VB(w, topics, p_word, p_topic, *extra, engine='fused+hyper' if learnt else 'fused')
        Q.ignore_bound_checks = True
        Q.update(repeat=2, verbose=False)
        torch.cuda.synchronize()
        assert np.all(np.isfinite(Q.L[:2]))
        return torch.cuda.max_memory_allocated() - base, type(Q.plans[0]).__name__
    const, name0 = run(False)
    learnt, name1 = run(True)
    print('peak: constant %.2f MB, learnt %.2f MB, allowance %.2f MB'
          % (const / 1e6, learnt / 1e6, 8.0 * (D + V) * K / 1e6))
    assert (name0, name1) == ('LDASVIPlan', 'HyperLDAPlan')
    assert learnt <= const + 8 * (D + V) * K
