#!/usr/bin/env python
"""
One sweep of the driven state-space model of tests/chain_in_models.py case b ([A | B], nu shared by
B sequences, constant inputs with the sequence plate) with the tune key chain_input_stats on and
off, and vmp_chain_input_stats alone:

    python tools/bench_chain_in.py [--B 10000] [--N 1000] [--D 4] [--K 3] [--M 4] [--sweeps 3]

Prints one JSON line: median seconds per sweep for both settings, peak device memory, and the
kernel's bytes/s against the 8 ny (N D + (N-1) K) bytes of the means of the states and the inputs.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(B, N, D, K, M, rs):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    alpha = N_.Gamma(1e-5, 1e-5, plates=(D + K,), name='alpha')
    A = N_.GaussianARD(0, alpha, shape=(D + K,), plates=(D,), name='A')
    A.initialize_from_value(np.concatenate([0.9 * np.identity(D), 0.1 * np.ones((D, K))], axis=-1))
    nu = N_.Gamma(1e-3, 1e-3, plates=(D,), name='nu')
    X = N_.GaussianMarkovChain(np.zeros(D), 1e-3 * np.identity(D), A, nu, n=N,
                               inputs=rs.normal(size=(B, N - 1, K)), plates=(B,), name='X')
    X.initialize_from_value(rs.normal(size=(B, N, D)))
    gamma = N_.Gamma(1e-5, 1e-5, plates=(D,), name='gamma')
    gamma.initialize_from_value(1e-2 * np.ones(D))
    C = N_.GaussianARD(0, gamma, shape=(D,), plates=(M, 1, 1), name='C')
    C.initialize_from_value(rs.normal(size=(M, 1, 1, D)))
    tau = N_.Gamma(1e-5, 1e-5, name='tau')
    tau.initialize_from_value(1e2)
    F = N_.SumMultiply('i,i', C, X, name='F')
    Y = N_.GaussianARD(F, tau, name='Y')
    Y.observe(rs.normal(size=(M, B, N)))
    Q = VB(Y, F, C, gamma, X, A, alpha, nu, tau)
    Q.ignore_bound_checks = True
    return Q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=10000)
    ap.add_argument('--N', type=int, default=1000)
    ap.add_argument('--D', type=int, default=4)
    ap.add_argument('--K', type=int, default=3)
    ap.add_argument('--M', type=int, default=4)
    ap.add_argument('--sweeps', type=int, default=3)
    a = ap.parse_args()
    os.environ['BAYESPY_AMD_GRAPH'] = '0'
    from bayespy_amd.device import get_runtime
    from bayespy_amd.utils import linalg
    from bayespy_amd.darray import DArray
    rt = get_runtime()
    torch = rt.torch
    out = dict(B=a.B, N=a.N, D=a.D, K=a.K, M=a.M)
    # the kernel alone
    x = DArray(torch.randn(a.B, a.N, a.D, dtype=torch.float64, device=rt.device))
    z = DArray(torch.randn(a.B, a.N - 1, a.K, dtype=torch.float64, device=rt.device))
    for _ in range(3):
        linalg.chain_input_stats(x, z)
    rt.synchronize()
    ts = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        linalg.chain_input_stats(x, z)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    out['kernel_s'] = float(np.median(ts))
    out['kernel_bytes_per_s'] = 8.0 * a.B * (a.N * a.D + (a.N - 1) * a.K) / out['kernel_s']
    del x, z
    for on in (1, 0, 1, 0):
        rt.set_tune('chain_input_stats', on)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            Q = build(a.B, a.N, a.D, a.K, a.M, np.random.RandomState(1))
            Q.update(repeat=1, verbose=False)          # forms the state, warms the caches
            ts = []
            for _ in range(a.sweeps):
                rt.synchronize()
                t0 = time.perf_counter()
                Q.update(repeat=1, verbose=False)
                rt.synchronize()
                ts.append(time.perf_counter() - t0)
        key = 'on' if on else 'off'
        out.setdefault('sweep_s_' + key, []).append(float(np.median(ts)))
        out['peak_bytes_' + key] = int(torch.cuda.max_memory_allocated())
        out['L_' + key] = float(Q.L[a.sweeps])
        del Q
    rt.set_tune('chain_input_stats', 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
