#!/usr/bin/env python
"""
A hidden Markov model with many states over count vectors: B sequences of genomic bins, each with
the counts of M marks among n reads, K = 96 hidden chromatin states, with a0, A and P learned from
their Dirichlet priors.  ``engine='fused+states'`` adds the wide-state form of the
multinomial-emission block (inference/plans/hmm_states.py): for
65 <= K <= 128 the chain pass runs with scaled probabilities on the fp64 matrix cores.  An entry
of <log A> below about -745 acts as -inf there.

    python examples/hmm_many_states.py [--chains 64] [--steps 200] [--marks 12] [--states 96]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hmm_multinomial import simulate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=64)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--marks', type=int, default=12)
    ap.add_argument('--states', type=int, default=96)
    ap.add_argument('--reads', type=int, default=40)
    ap.add_argument('--sweeps', type=int, default=20)
    a = ap.parse_args()
    from bayespy_amd.nodes import CategoricalMarkovChain, Dirichlet, Mixture, Multinomial
    from bayespy_amd.inference import VB
    B, T, M, K, n = a.chains, a.steps, a.marks, a.states, a.reads
    rs = np.random.RandomState(1)
    x, z = simulate(B, T, M, K, n, rs)
    a0 = Dirichlet(np.ones(K), name='a0')
    A = Dirichlet(np.ones((K, K)) + 5 * np.identity(K), name='A')
    P = Dirichlet(0.5 + rs.gamma(1.0, size=(K, M)), name='P')       # asymmetric: tells states apart
    Z = CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z')
    Y = Mixture(Z, Multinomial, n, P, name='Y')
    Y.observe(x)
    Q = VB(Y, Z, P, A, a0, engine='fused+states')
    print(type(Q.plans[0]).__name__)
    t0 = time.perf_counter()
    Q.update(repeat=a.sweeps, verbose=False)
    print('%d sweeps over %d count vectors, %d states: %.1f ms, set-up included; bound %.2f -> %.2f'
          % (Q.iter, B * T, K, 1e3 * (time.perf_counter() - t0), Q.L[0], Q.L[Q.iter - 1]))


if __name__ == '__main__':
    main()
