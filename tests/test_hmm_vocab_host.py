"""CPU: the large-vocabulary form of the fused discrete hidden-Markov-model block without a device
-- where engine='fused+words' routes a model and what the other engine values keep saying, and the
segment walk and combine rule of csrc/vmp_hmm_vocab_dev.h, built with g++, bit for bit against the
same additions in the documented order."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _nodes(M, T=60, K=3):
    """Case one of tests/hmm_vocab_models.py with M words: one chain, a0, A and P from priors."""
    from bayespy_amd import nodes as N_
    a0 = N_.Dirichlet(np.ones(K), name='a0')
    A = N_.Dirichlet(np.ones((K, K)), name='A')
    P = N_.Dirichlet(np.ones((K, M)), name='P')
    Z = N_.CategoricalMarkovChain(a0, A, states=T, name='Z')
    Y = N_.Mixture(Z, N_.Categorical, P, name='Y')
    Y.observe(np.arange(T) % M)
    return [Y, Z, P, A, a0]


def test_routing():
    """Fails without the feature: engine='fused+words' is the generic engine's business today."""
    from bayespy_amd.inference.plans import compile_model
    from bayespy_amd.inference.plans.hmm_vocab import VocabCategoricalHMMPlan
    names = lambda plans: [type(p).__name__ for p in plans]  # noqa: E731
    assert names(compile_model(_nodes(131), engine='fused+words')) == ['VocabCategoricalHMMPlan']
    small = _nodes(100)
    why = []
    assert VocabCategoricalHMMPlan.match(small, why) is None
    assert len(why) == 1 and 'use the discrete HMM block' in why[0]
    assert names(compile_model(small, engine='fused+words')) == ['CategoricalHMMPlan']
    for engine, label in (('fused', 'block with categorical emissions'),
                          ('fused+chains', 'block (long chains, categorical)')):
        with pytest.raises(NotImplementedError) as exc:
            compile_model(_nodes(131), engine=engine)
        assert label + ', observed node Y: M = 131, K = 3 exceed the limits' in str(exc.value)
        assert 'large vocabulary' not in str(exc.value)


def _host():
    from host_build import build_host_library
    lib = build_host_library('hmmv', ['tests/host/hmm_vocab_host.cpp',
                                      'bayespy_amd/csrc/vmp_hmm_vocab_dev.h',
                                      'bayespy_amd/csrc/vmp_hmm_fused_dev.h',
                                      'bayespy_amd/csrc/vmp_lda_dev.h'])
    lib.hmmv_chunk_entries.argtypes = [ctypes.c_int64, ctypes.c_int]
    lib.hmmv_count.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
    lib.hmmv_count.restype = None
    return lib


def _count(lib, order, off, gam, M):
    K = gam.shape[1]
    nc = -(-len(order) // lib.hmmv_chunk_entries(len(order), K))
    S, head, tail = np.full((M, K), np.nan), np.full((nc, K), np.nan), np.full((nc, K), np.nan)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib.hmmv_count(len(order), M, K, p(order), p(off), p(gam), p(S), p(head), p(tail))
    return S


@pytest.mark.parametrize('M', [1, 3, 129])
@pytest.mark.parametrize('n_obs', [1, 16, 37, 53, 96])
def test_segment_walk_and_combine_rule(n_obs, M):
    lib = _host()
    rs = np.random.RandomState(n_obs + M)
    K, N = 5, n_obs + 7
    CH = lib.hmmv_chunk_entries(n_obs, K)
    assert CH == 16
    pos = np.sort(rs.permutation(N)[:n_obs])
    words = rs.randint(M, size=n_obs)
    idx = np.argsort(words, kind='stable')
    order = np.ascontiguousarray(pos[idx], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(np.bincount(words, minlength=M))]).astype(np.int32)
    gam = rs.dirichlet(np.ones(K), size=N)
    # the documented order: per chunk the entries in order from zero, then the chunks in order
    want = np.zeros((M, K))
    for m in range(M):
        parts = []
        for c in range(off[m] // CH, (off[m + 1] - 1) // CH + 1 if off[m + 1] > off[m] else 0):
            acc = np.zeros(K)
            for i in range(max(off[m], c * CH), min(off[m + 1], (c + 1) * CH)):
                acc = acc + gam[order[i]]
            parts.append(acc)
        for part in parts[1:]:
            parts[0] = parts[0] + part
        if parts:
            want[m] = parts[0]
    np.testing.assert_array_equal(_count(lib, order, off, gam, M), want)
    onehot = np.eye(K)[rs.randint(K, size=N)]
    exact = np.zeros((M, K))
    np.add.at(exact, words[idx], onehot[order])
    np.testing.assert_array_equal(_count(lib, order, off, onehot, M), exact)
