#!/usr/bin/env python
"""
Timed legs of the fused diagonal-Gaussian-mixture block with missing observations
(inference/plans/dgmm_masked.py) against the block without a mask on the same data, in one
session; one JSON line each.  The protocol, the data and the model are those of tools/bench_dgmm.py.

  (i)  N = 1e6, D = 256, K = 32, 30 % hidden: ms per ``Q.update()`` and per pass alone
       (``vmp_dgmm_pass_masked`` on the same state), masked and unmasked, the ratios, and the masked
       pass's fraction of the fp64 matrix peak (12 N D K flops) and of the HBM rate (16 N D bytes:
       above D = 32 the packed y is read twice);
  (ii) N = 1e5, D = 64, K = 32, 30 % hidden: the same, and the generic engine on the masked model,
       with the peak allocation of each.

    python tools/bench_dgmm_masked.py [--legs i,ii] [--steps 10] [--warmup 3] [--out profiles/dgmm/...json]
"""
import argparse
import gc
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_dgmm import FP64_MATRIX_PEAK_TFLOPS, HBM_TBPS, make_data, timed      # noqa: E402

HIDDEN = 0.3


def build(y, mask, centres, K, engine):
    """The model of tools/bench_dgmm.py; ``mask`` None: fully observed."""
    from bayespy_amd import nodes
    from bayespy_amd.inference import VB
    N, D = y.shape
    alpha = nodes.Dirichlet(K * [1.0], name='alpha')
    Z = nodes.Categorical(alpha, plates=(N, 1), name='Z')
    mu = nodes.GaussianARD(0.0, 1e-3, plates=(D, K), name='mu')
    tau = nodes.Gamma(1e-2, 1e-2, plates=(D, K), name='tau')
    Y = nodes.Mixture(Z, nodes.GaussianARD, mu, tau, name='Y')
    if mask is None:
        Y.observe(y)
    else:
        Y.observe(y, mask=mask)
    mu.initialize_from_value(centres.T + 0.5 * np.random.RandomState(1).normal(size=(D, K)))
    return VB(Y, Z, mu, tau, alpha, engine=engine)


def leg(tag, N, D, K, steps, warmup, generic):
    import torch
    gc.collect()
    y, centres = make_data(N, D, K)
    g = torch.Generator(device='cuda').manual_seed(1)
    mask = torch.rand(N, D, device='cuda', generator=g) >= HIDDEN
    out = dict(leg=tag, N=N, D=D, K=K, hidden=HIDDEN, observed=int(mask.sum().item()),
               y_bytes=int(y.numel() * 8), ndk_bytes=int(8 * N * D * K))
    for name, m in (('unmasked', None), ('masked', mask)):
        gc.collect()                    # the plan before this one is gone: y and the mask remain
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        Q = build(y, m, centres, K, 'fused')
        plan = Q.plans[0]
        r = dict(plan=type(plan).__name__)
        r['update'] = timed(lambda: Q.update(verbose=False), steps, warmup)
        r['pass_alone'] = timed(lambda: plan._run_pass(), steps, warmup)
        r['pass_share'] = r['pass_alone']['median_ms'] / r['update']['median_ms']
        r['chunk_rows'] = int(plan.chunk)
        r['peak_alloc_bytes'] = int(torch.cuda.max_memory_allocated())
        r['peak_alloc_above_inputs_bytes'] = r['peak_alloc_bytes'] - int(base)
        r['L'] = float(Q.L[Q.iter - 1])
        sec = r['pass_alone']['median_ms'] * 1e-3
        products, block = (3, 32) if m is not None else (2, 64)
        reads = 1 if D <= block else 2
        r['y_reads'] = reads
        r['pass_tflops'] = 4.0 * products * N * D * K / sec / 1e12
        r['pass_tbps'] = 8.0 * reads * N * D / sec / 1e12
        r['pass_fraction_of_fp64_matrix_peak'] = r['pass_tflops'] / FP64_MATRIX_PEAK_TFLOPS
        r['pass_fraction_of_hbm_rate'] = r['pass_tbps'] / HBM_TBPS
        out[name] = r
        del Q, plan
    out['masked_pass_over_unmasked'] = \
        out['masked']['pass_alone']['median_ms'] / out['unmasked']['pass_alone']['median_ms']
    out['masked_update_over_unmasked'] = \
        out['masked']['update']['median_ms'] / out['unmasked']['update']['median_ms']
    if generic:
        gc.collect()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        Q = build(y, mask, centres, K, 'generic')
        r = timed(lambda: Q.update(verbose=False), steps, warmup)
        r['plan'] = type(Q.plans[0]).__name__
        r['peak_alloc_bytes'] = int(torch.cuda.max_memory_allocated())
        r['peak_alloc_above_inputs_bytes'] = r['peak_alloc_bytes'] - int(base)
        r['L'] = float(Q.L[Q.iter - 1])
        out['generic'] = r
        out['generic_over_masked'] = r['median_ms'] / out['masked']['update']['median_ms']
        del Q
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='i,ii')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    for name in a.legs.split(','):
        np.random.seed(0)
        if name == 'i':
            r = leg('i', 10 ** 6, 256, 32, a.steps, a.warmup, generic=False)
        elif name == 'ii':
            r = leg('ii', 10 ** 5, 64, 32, a.steps, a.warmup, generic=True)
        else:
            raise SystemExit('unknown leg %r' % name)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
