#!/usr/bin/env python
"""
The first model of doc/source/examples/hmm.rst -- rainy / sunny days seen through walk / shop /
clean, with known a0, A and P -- on ONE sequence of T = 2e5 days.  The discrete HMM block walks a
sequence step by step on one lane group; ``engine='fused+chains'`` puts its long-chain form in the
block's place, which cuts the sequence into segments and runs the recursion inside all of them at
once (inference/plans/hmm_seg_cat.py).  a0, A and P are constants, so Y and
Z are the whole model and one update gives the exact posterior.

    python examples/hmm_discrete_long.py [--steps 200000] [--seg-len 0] [--engine fused+chains]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

A0 = np.array([0.6, 0.4])                   # p(rainy) = 0.6, p(sunny) = 0.4
A = np.array([[0.7, 0.3],                   # p(rainy -> rainy) = 0.7, p(rainy -> sunny) = 0.3
              [0.4, 0.6]])                  # p(sunny -> rainy) = 0.4, p(sunny -> sunny) = 0.6
P = np.array([[0.1, 0.4, 0.5],
              [0.6, 0.3, 0.1]])


def simulate(T, rs):
    u, weather = rs.rand(T), np.empty(T, dtype=np.int64)
    weather[0] = u[0] > A0[0]
    for t in range(1, T):
        weather[t] = u[t] > A[weather[t - 1], 0]
    activity = (rs.rand(T)[:, None] > np.cumsum(P, axis=1)[weather]).sum(-1).clip(0, 2)
    return weather, activity


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200000)
    ap.add_argument('--seg-len', type=int, default=0)
    ap.add_argument('--engine', default='fused+chains', choices=('fused+chains', 'fused'))
    a = ap.parse_args()
    from bayespy_amd.nodes import CategoricalMarkovChain, Categorical, Mixture
    from bayespy_amd.inference import VB
    weather, activity = simulate(a.steps, np.random.RandomState(1))
    Z = CategoricalMarkovChain(A0, A, states=a.steps)
    Y = Mixture(Z, Categorical, P)
    Y.observe(activity)
    Q = VB(Y, Z, engine=a.engine)
    plan = Q.plans[0]
    print(type(plan).__name__)
    if a.seg_len and a.engine == 'fused+chains':
        plan.seg_len = a.seg_len                # transitions of a segment; 0: the library's choice
    t0 = time.perf_counter()
    Q.update(verbose=False)
    print('log p(activity) = %.6f  (%.1f ms, set-up included)'
          % (Q.L[0], 1e3 * (time.perf_counter() - t0)))
    if a.engine == 'fused+chains':
        print('segment length in use: %d' % plan.chains_per_wg)
    p_rainy = Y.parents[0].get_moments()[0][:, 0]
    print('days whose likelier weather is the true one: %d of %d'
          % (np.sum((p_rainy > 0.5) == (weather == 0)), a.steps))


if __name__ == '__main__':
    main()
