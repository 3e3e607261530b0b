#!/usr/bin/env python
"""
Timed legs of the fused hidden-Markov-model block (inference/plans/hmm.py); one JSON line each.

At B = 2e4 chains, T = 1000 steps, D = 2, K = 8 with learned emissions (the model script of
tests/hmm_models.py, Z from fixed random labels):
  fused    ms per ``Q.update()`` with engine='fused';
  pass     ``vmp_hmm_fused_pass`` alone on the same state, with its bytes per chain step (y read
           twice, the forward state written and read once: 16 D + 16 K) and the exponentials per
           second ((3 K + 2) K per chain step);
  generic  ms per ``Q.update()`` of the same script with engine='generic' (the yardstick: logP and
           zz of shape (B, T-1, K, K), 10 GB each).

  masked   (with --observed and / or --ragged) ``vmp_hmm_fused_pass_masked`` on the same state
           after ``Y.observe(y, mask=m)``: one line per mask -- a fraction of the steps observed at
           random (1.0 is a mask of ones), or sequence lengths uniform in 1 ... T as trailing masks;
           NaN stands at the masked positions.  Without --out these lines (and the unmasked pass
           of the same build before them) go to profiles/hmm_fused/bench_hmm_masked.json.

  cat      (--emissions categorical) the same three legs for the discrete block
           (inference/plans/hmm_cat.py): M = 16 words, learned P, Z from fixed random labels; the
           pass is ``vmp_hmm_fused_pass_categorical`` (8 + 16 K bytes per chain step: the int32 word read
           twice, the forward state written and read once; the <log P> rows come from L2).
           Without --out these lines go to profiles/hmm_fused/bench_hmm_cat.json.
           --engine fused+words (inference/plans/hmm_vocab.py) with --M 128,4096,65536: the legs once
           per vocabulary in one process; the pass is ``vmp_hmm_vocab_pass`` above 128 words
           (12 + 32 K bytes per chain step), and at 128 words or fewer both the sequential pass and
           the vocabulary pass on the same state.

  wide     (--engine fused+emissions, 9 <= D <= 32) the same legs on the wide-emission form
           (inference/plans/hmm_wide.py); the pass is ``vmp_hmm_wide_pass`` (16 D + 24 KP + 32 K bytes
           per chain step: y read by the emission and the statistics kernel, E written once and
           read twice, the forward state written and read and gamma written and read in its
           place).  --wide-pass (any D <= 8, engine fused) times ``vmp_hmm_wide_pass`` on the state
           of the narrow plan right after ``vmp_hmm_fused_pass``, in the same process.

  chains   (--engine fused+chains, D <= 32) the same legs on the long-chain form
           (inference/plans/hmm_seg.py); the pass is ``vmp_hmm_seg_pass``, one ``pass`` line per
           value of --seg-len (comma-separated; 0 = the library's choice), each with the segment
           length in use.  --wide-pass then times ``vmp_hmm_wide_pass``, the sequential chain
           stage, on the same state in the same process.

  mult     (--emissions multinomial --engine fused+counts, or fused+states with --K 65 .. 128, --M 64,256,1024, --trials n) the legs
           for the multinomial-emission form (inference/plans/hmm_mult.py): count vectors of n
           trials drawn on the device, learned P, Z from fixed random labels; the pass is
           ``vmp_hmm_mult_pass`` (4 M + 24 KP + 32 K bytes per chain step: the uint16 counts read by
           the emission and the statistics kernel, E written once and read twice, the forward
           state written and read and gamma written and read in its place); a ``kernels`` line
           gives the device time of every kernel of one pass.

  diag     (--emissions diagonal --engine fused+diagonal, --dims 64,256,1024) the legs for the
           diagonal-Gaussian-emission form (inference/plans/hmm_diag.py): y drawn on the device,
           B capped so that y stays at or below 2^30 doubles, Z from fixed random labels; the pass
           is ``vmp_hmm_diag_pass`` (16 D + 24 KP + 32 K bytes per chain step); a ``kernels`` line
           gives the device time of every kernel of one pass and the rate of the two plate kernels
           against one read of y, a ``kernels_mult`` line the kernels of ``vmp_hmm_mult_pass`` at
           the same (B, T, K) in the same process (the chain stage is the same kernel); the
           ``compare`` lines time ``Q.update()`` on this form and on the generic engine at
           --generic-B chains, with peak memory above the resident y and the bound.

    python tools/bench_hmm_fused.py [--legs fused,pass,generic] [--B 20000] [--T 1000] [--steps 5]
                                    [--warmup 2] [--out profiles/...json]
    python tools/bench_hmm_fused.py --legs pass --observed 1.0,0.7 --ragged

Every leg warms up, then times ``steps`` calls one by one between device synchronisations and
reports the median and the extremes.
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def make_data(B, T, D, K, seed=0):
    rs = np.random.RandomState(seed)
    mu = 5.0 * rs.normal(size=(K, D))
    z = np.empty((B, T), dtype=np.int64)
    z[:, 0] = rs.randint(K, size=B)
    for t in range(1, T):                           # sticky chains
        z[:, t] = np.where(rs.rand(B) < 0.9, z[:, t - 1], rs.randint(K, size=B))
    y = mu[z] + rs.normal(size=(B, T, D))
    return y, mu, rs.randint(K, size=(B, T))


def build(y, mu, z0, engine):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from hmm_models import build_hmm
    m = build_hmm(dict(nodes=nodes), y, mu, None, learned=True)
    m['Z'].initialize_from_value(z0)
    Q = VB(m['Y'], m['mu'], m['Lambda'], m['A'], m['a0'], m['Z'], engine=engine)
    Q.ignore_bound_checks = True
    return Q


def make_words(B, T, M, K, seed=0):
    rs = np.random.RandomState(seed)
    P = rs.dirichlet(0.3 * np.ones(M), size=K)
    z = np.empty((B, T), dtype=np.int64)
    z[:, 0] = rs.randint(K, size=B)
    for t in range(1, T):                           # sticky chains
        z[:, t] = np.where(rs.rand(B) < 0.9, z[:, t - 1], rs.randint(K, size=B))
    u = rs.rand(B, T)
    y = np.empty((B, T), dtype=np.int64)
    for k in range(K):                              # the number of cumulative sums below u
        y[z == k] = np.searchsorted(np.cumsum(P[k]), u[z == k]).clip(0, M - 1)
    return y, rs.randint(K, size=(B, T))


def build_cat(y, z0, K, M, engine):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    B, T = y.shape
    a0 = N_.Dirichlet(1e-3 * np.ones(K), name='a0')
    A = N_.Dirichlet(1e-3 * np.ones((K, K)), name='A')
    P = N_.Dirichlet(np.ones((K, M)), name='P')
    Z = N_.CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z')
    Y = N_.Mixture(Z, N_.Categorical, P, name='Y')
    Y.observe(y)
    Z.initialize_from_value(z0)
    Q = VB(Y, P, A, a0, Z, engine=engine)
    Q.ignore_bound_checks = True
    return Q


def categorical_legs(a, emit, M):
    import torch
    B, T, K = a.B, a.T, a.K
    y, z0 = make_words(B, T, M, K)
    legs = a.legs.split(',')
    if 'fused' in legs or 'pass' in legs:
        torch.cuda.reset_peak_memory_stats()
        Q = build_cat(y, z0, K, M, a.engine)
        plan = Q.plans[0]
        words = type(plan).__name__ == 'VocabCategoricalHMMPlan'
        assert words == (a.engine == 'fused+words' and M > 128)
        assert words or type(plan).__name__ == 'CategoricalHMMPlan'
        if 'fused' in legs:
            emit(dict(leg='fused', what='Q.update()',
                      **timed(lambda: Q.update(verbose=False), a.steps, a.warmup)))
            emit(dict(leg='fused_bound', L=float(Q.L[Q.iter - 1]),
                      peak_GB=torch.cuda.max_memory_allocated() / 1e9))
        else:
            Q.update(verbose=False)
        def pass_leg(what, nbytes):
            r = timed(lambda: plan._run_pass(refresh=False), a.steps, a.warmup)
            steps_total = float(B) * T
            s = 1e-3 * r['ms_median']
            emit(dict(leg='pass', what=what, bytes_per_chain_step=nbytes,
                      GB_per_s=steps_total * nbytes / s / 1e9,
                      exp_per_chain_step=(3 * K + 2) * K,
                      Gexp_per_s=steps_total * (3 * K + 2) * K / s / 1e9, **r))
        # the vocabulary pass: the word read twice, la written and read, gamma written over it and
        # read by the count kernel, 4 bytes of layout
        vocab_bytes = 12 + 32 * K
        if 'pass' in legs and words:
            pass_leg('vmp_hmm_vocab_pass', vocab_bytes)
        elif 'pass' in legs:
            pass_leg('vmp_hmm_fused_pass_categorical', 8 + 16 * K)
            if a.engine == 'fused+words':
                # the vocabulary pass on the state of the sequential plan, in the same process
                from bayespy_amd.inference.plans.hmm_vocab import VocabCatHMMKernels
                seq_k, seq_ws = plan._kernels, plan.ws
                from bayespy_amd.inference.plans.hmm_vocab import word_layout
                plan._kernels = VocabCatHMMKernels(plan.rt)
                plan._kernels.layout = word_layout(torch, plan.yd, plan.maskd, M)
                plan.ws = plan.rt.empty(int(plan._kernels.plan(B, T, M, K)[1]))
                pass_leg('vmp_hmm_vocab_pass', vocab_bytes)
                plan._kernels, plan.ws = seq_k, seq_ws
        del Q, plan
        torch.cuda.empty_cache()
    if 'generic' in legs:
        try:
            torch.cuda.reset_peak_memory_stats()
            Q = build_cat(y, z0, K, M, 'generic')
            emit(dict(leg='generic', what='Q.update()',
                      **timed(lambda: Q.update(verbose=False), a.steps, a.warmup)))
            emit(dict(leg='generic_bound', L=float(Q.L[Q.iter - 1]),
                      peak_GB=torch.cuda.max_memory_allocated() / 1e9))
        except (RuntimeError, MemoryError) as exc:         # out of memory at this size
            emit(dict(leg='generic', error=str(exc)[:200]))


def make_counts(B, T, M, K, n, seed=0):
    """(x (B, T, M) uint8 on the device, z0): n trials per step from sticky chains."""
    import torch
    rs = np.random.RandomState(seed)
    gen = torch.Generator(device='cuda').manual_seed(seed)
    P = torch.from_numpy(rs.dirichlet(0.3 * np.ones(M), size=K)).cuda()
    z = np.empty((B, T), dtype=np.int64)
    z[:, 0] = rs.randint(K, size=B)
    for t in range(1, T):                           # sticky chains
        z[:, t] = np.where(rs.rand(B) < 0.9, z[:, t - 1], rs.randint(K, size=B))
    zd = torch.from_numpy(z.reshape(-1)).cuda()
    x = torch.zeros(B * T, M, dtype=torch.uint8, device='cuda')
    for r0 in range(0, B * T, 1 << 18):             # in blocks of rows: the draws are int64
        zr = zd[r0:r0 + (1 << 18)]
        words = torch.multinomial(P, n * 64, replacement=True, generator=gen)     # K x (64 n)
        pick = torch.randint(64, (zr.numel(), 1), device='cuda', generator=gen) * n \
            + torch.arange(n, device='cuda')
        idx = words[zr[:, None], pick]
        cnt = torch.zeros(zr.numel(), M, dtype=torch.int32, device='cuda')
        cnt.scatter_add_(1, idx, torch.ones_like(idx, dtype=torch.int32))
        x[r0:r0 + (1 << 18)] = cnt.to(torch.uint8)
    return x.reshape(B, T, M), rs.randint(K, size=(B, T))


def multinomial_legs(a, emit, M):
    import torch
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    B, T, K, n = a.B, a.T, a.K, a.trials
    assert n <= 255
    x, z0 = make_counts(B, T, M, K, n)
    legs = a.legs.split(',')
    KP = max(2, 1 << (K - 1).bit_length())

    def build_mult(engine):
        a0 = N_.Dirichlet(1e-3 * np.ones(K), name='a0')
        A = N_.Dirichlet(1e-3 * np.ones((K, K)), name='A')
        P = N_.Dirichlet(np.ones((K, M)), name='P')
        Z = N_.CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z')
        Y = N_.Mixture(Z, N_.Multinomial, n, P, name='Y')
        Y.observe(x if engine != 'generic' else x.cpu().numpy())     # generic: host counts
        Z.initialize_from_value(z0)
        Q = VB(Y, P, A, a0, Z, engine=engine)
        Q.ignore_bound_checks = True
        return Q
    if 'fused' in legs or 'pass' in legs:
        torch.cuda.reset_peak_memory_stats()
        Q = build_mult(a.engine)
        plan = Q.plans[0]
        assert type(plan).__name__ == ('WideStateMultinomialHMMPlan' if K > 64 else 'MultinomialHMMPlan')
        emit(dict(leg='fused', what='Q.update()',
                  **timed(lambda: Q.update(verbose=False), a.steps, a.warmup)))
        emit(dict(leg='fused_bound', L=float(Q.L[Q.iter - 1]),
                  peak_GB=torch.cuda.max_memory_allocated() / 1e9))
        if 'pass' in legs:
            r = timed(lambda: plan._run_pass(refresh=False), a.steps, a.warmup)
            nbytes = 4 * M + 24 * KP + 32 * K
            emit(dict(leg='pass', what='vmp_hmm_states_pass' if K > 64 else 'vmp_hmm_mult_pass',
                      bytes_per_chain_step=nbytes,
                      GB_per_s=float(B) * T * nbytes / (1e-3 * r['ms_median']) / 1e9,
                      Gflop_per_s_each_product=2.0 * B * T * M * K / (1e-3 * r['ms_median']) / 1e9,
                      **r))
            from torch.profiler import profile, ProfilerActivity
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                plan._run_pass(refresh=False)
                torch.cuda.synchronize()
            ms = {}
            for e in prof.key_averages():
                name = re.search(r'\w+_kernel', e.key)
                if name and e.device_time_total > 0:
                    ms[name.group(0)] = ms.get(name.group(0), 0.0) + 1e-3 * e.device_time_total
            emit(dict(leg='kernels', ms=ms))
        del Q, plan
        torch.cuda.empty_cache()
    if 'generic' in legs:
        try:
            torch.cuda.reset_peak_memory_stats()
            Q = build_mult('generic')
            emit(dict(leg='generic', what='Q.update()',
                      **timed(lambda: Q.update(verbose=False), a.steps, a.warmup)))
            emit(dict(leg='generic_bound', L=float(Q.L[Q.iter - 1]),
                      peak_GB=torch.cuda.max_memory_allocated() / 1e9))
        except (RuntimeError, MemoryError) as exc:         # out of memory at this size
            emit(dict(leg='generic', error=str(exc)[:200]))


def kernel_ms(fn):
    """Device time per kernel of one call of ``fn`` (torch profiler), by kernel name."""
    import torch
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ms = {}
    for e in prof.key_averages():
        name = re.search(r'\w+_kernel', e.key)
        if name and e.device_time_total > 0:
            ms[name.group(0)] = ms.get(name.group(0), 0.0) + 1e-3 * e.device_time_total
    return ms


def diagonal_legs(a, emit, D):
    import torch
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    T, K = a.T, a.K
    B = min(a.B, (1 << 30) // (T * D))              # y stays at or below 2^30 doubles
    legs = a.legs.split(',')
    KP = max(2, 1 << (K - 1).bit_length())
    rs = np.random.RandomState(0)
    gen = torch.Generator(device='cuda').manual_seed(0)
    z = np.empty((B, T), dtype=np.int64)
    z[:, 0] = rs.randint(K, size=B)
    for t in range(1, T):                           # sticky chains
        z[:, t] = np.where(rs.rand(B) < 0.9, z[:, t - 1], rs.randint(K, size=B))
    means = 3.0 * torch.randn(K, D, dtype=torch.float64, device='cuda', generator=gen)
    y = torch.randn(B, T, D, dtype=torch.float64, device='cuda', generator=gen)
    y += means[torch.from_numpy(z).cuda()]
    z0 = rs.randint(K, size=(B, T))

    def build_diag(engine, Bm):
        a0 = N_.Dirichlet(1e-3 * np.ones(K), name='a0')
        A = N_.Dirichlet(1e-3 * np.ones((K, K)), name='A')
        Z = N_.CategoricalMarkovChain(a0, A, states=T, plates=(Bm,), name='Z')
        mu = N_.GaussianARD(0, 1e-3, shape=(D,), plates=(K,), name='mu')
        tau = N_.Gamma(1e-3, 1e-3, plates=(K, D), name='tau')
        Y = N_.Mixture(Z, N_.GaussianARD, mu, tau, 1, name='Y')
        Y.observe(y[:Bm] if engine != 'generic' else y[:Bm].cpu().numpy())
        Z.initialize_from_value(z0[:Bm])
        Q = VB(Y, mu, tau, A, a0, Z, engine=engine)
        Q.ignore_bound_checks = True
        return Q
    if 'fused' in legs or 'pass' in legs:
        torch.cuda.reset_peak_memory_stats()
        Q = build_diag(a.engine, B)
        plan = Q.plans[0]
        assert type(plan).__name__ == 'DiagGaussianHMMPlan'
        emit(dict(B=B, leg='fused', what='Q.update()',
                  **timed(lambda: Q.update(verbose=False), a.steps, a.warmup)))
        emit(dict(B=B, leg='fused_bound', L=float(Q.L[Q.iter - 1]),
                  peak_GB=torch.cuda.max_memory_allocated() / 1e9))
        if 'pass' in legs:
            r = timed(lambda: plan._run_pass(refresh=False), a.steps, a.warmup)
            nbytes = 16 * D + 24 * KP + 32 * K
            emit(dict(B=B, leg='pass', what='vmp_hmm_diag_pass', bytes_per_chain_step=nbytes,
                      GB_per_s=float(B) * T * nbytes / (1e-3 * r['ms_median']) / 1e9, **r))
            ms = kernel_ms(lambda: plan._run_pass(refresh=False))
            # each plate kernel reads y once: 8 B T D bytes; 4 B T D K flops (y and y^2)
            floor = {k: dict(TB_per_s=8.0 * B * T * D / (1e-3 * v) / 1e12,
                             Tflop_per_s=4.0 * B * T * D * K / (1e-3 * v) / 1e12)
                     for k, v in ms.items() if k in ('hmmd_emit_kernel', 'hmmd_stats_kernel')}
            emit(dict(B=B, leg='kernels', ms=ms, against_y_read_once=floor))
            # the chain stage inside vmp_hmm_mult_pass at the same (B, T, K), in the same process
            from bayespy_amd.inference.plans.hmm_mult import MultHMMKernels
            mk, M = MultHMMKernels(plan.rt), 64
            xp = torch.randint(0, 4, (B * T, M), device='cuda', generator=gen).to(torch.int16)
            Pt = torch.log_softmax(torch.randn(K, M, dtype=torch.float64, device='cuda',
                                               generator=gen), -1).T.contiguous()
            ws = plan.rt.empty(int(mk.plan(B, T, M, K)[1]))
            S = plan.rt.zeros(M, K)
            run = lambda: mk.pass_(B, T, M, K, xp, Pt, plan.used_a0, plan.used_A, None, None, ws,  # noqa: E731
                                   plan.rt.zeros(K), plan.rt.zeros(K, K), S, plan.rt.zeros(8))
            timed(run, 1, a.warmup)
            emit(dict(B=B, leg='kernels_mult', what='vmp_hmm_mult_pass, M = 64', ms=kernel_ms(run)))
            del xp, ws
        del Q, plan
        torch.cuda.empty_cache()
    if 'generic' in legs:
        Bm = min(B, a.generic_B)
        for engine in (a.engine, 'generic'):
            try:
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()        # y of the full B stays resident
                Q = build_diag(engine, Bm)
                emit(dict(B=Bm, leg='compare', engine=engine, what='Q.update()',
                          **timed(lambda: Q.update(verbose=False), a.steps, a.warmup)))
                emit(dict(B=Bm, leg='compare_bound', engine=engine, iterations=int(Q.iter),
                          L=float(Q.L[Q.iter - 1]),
                          peak_GB_above_y=(torch.cuda.max_memory_allocated() - base) / 1e9))
                del Q
            except (RuntimeError, MemoryError, NotImplementedError) as exc:
                emit(dict(B=Bm, leg='compare', engine=engine, error=str(exc)[:200]))


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return dict(ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)),
                steps=steps, warmup=warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='fused,pass,generic')
    ap.add_argument('--B', type=int, default=20000)
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--D', type=int, default=2)
    ap.add_argument('--K', type=int, default=8)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--observed', default=None,
                    help='comma-separated fractions of observed steps for the masked pass')
    ap.add_argument('--ragged', action='store_true',
                    help='masked pass with sequence lengths uniform in 1 ... T')
    ap.add_argument('--emissions', default='gaussian', choices=('gaussian', 'categorical', 'multinomial', 'diagonal'))
    ap.add_argument('--trials', type=int, default=50,
                    help='multinomial legs: trials n of every step (at most 255)')
    ap.add_argument('--M', default='16',
                    help='words of the categorical legs; comma-separated: the legs once per value, '
                         'in one process')
    ap.add_argument('--engine', default='fused',
                    choices=('fused', 'fused+emissions', 'fused+chains', 'fused+words',
                             'fused+counts', 'fused+diagonal', 'fused+states'))
    ap.add_argument('--dims', default='64,256,1024',
                    help='diagonal legs: comma-separated D, the legs once per value; B is capped '
                         'so that y stays at or below 2^30 doubles')
    ap.add_argument('--generic-B', type=int, default=64,
                    help='diagonal legs: chains of the comparison with the generic engine')
    ap.add_argument('--seg-len', default='0',
                    help='fused+chains: comma-separated segment lengths of the pass legs (0 = the '
                         "library's choice)")
    ap.add_argument('--wide-pass', action='store_true',
                    help='also time vmp_hmm_wide_pass on the state of the narrow plan')
    a = ap.parse_args()
    import torch
    from bayespy_amd.inference.plans.hmm import HMMPlan
    B, T, D, K = a.B, a.T, a.D, a.K
    cat = a.emissions == 'categorical'
    shape = dict(B=B, T=T, M=0, K=K, emissions='categorical') if cat else dict(B=B, T=T, D=D, K=K)
    lines = []

    def emit(rec):
        rec = dict(shape, **rec)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    if a.emissions == 'diagonal':
        shape = dict(T=T, D=0, K=K, emissions='diagonal')
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'hmm_fused', 'bench_hmm_diag.json')
        for D in a.dims.split(','):
            shape['D'] = int(D)
            diagonal_legs(a, emit, int(D))
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return
    if a.emissions == 'multinomial':
        shape = dict(B=B, T=T, M=0, K=K, emissions='multinomial', trials=a.trials)
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'hmm_fused', 'bench_hmm_mult.json')
        for M in a.M.split(','):
            shape['M'] = int(M)
            multinomial_legs(a, emit, int(M))
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return
    if cat:
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'hmm_fused', 'bench_hmm_cat.json')
        for M in a.M.split(','):
            shape['M'] = int(M)
            categorical_legs(a, emit, int(M))
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return
    y, mu, z0 = make_data(B, T, D, K)

    legs = a.legs.split(',')
    masks = [('observed %g' % float(f), float(f)) for f in (a.observed or '').split(',') if f]
    if a.ragged:
        masks.append(('ragged', None))
    if masks and 'pass' not in legs:
        legs.append('pass')
    if masks and a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'hmm_fused', 'bench_hmm_masked.json')
    if 'fused' in legs or 'pass' in legs:
        torch.cuda.reset_peak_memory_stats()
        Q = build(y, mu, z0, a.engine)
        plan = Q.plans[0]
        wide = type(plan).__name__ == 'WideHMMPlan'
        seg = type(plan).__name__ == 'SegmentedHMMPlan'
        assert wide == (a.engine == 'fused+emissions' and D > 8) and isinstance(plan, HMMPlan)
        assert seg == (a.engine == 'fused+chains')
        KP = max(2, 1 << (K - 1).bit_length())
        step_bytes = 16 * D + 24 * KP + 32 * K if wide or seg else 16 * D + 16 * K
        if 'fused' in legs:
            emit(dict(leg='fused', what='Q.update()',
                      **timed(lambda: Q.update(verbose=False), a.steps, a.warmup)))
            emit(dict(leg='fused_bound', L=float(Q.L[Q.iter - 1]),
                      peak_GB=torch.cuda.max_memory_allocated() / 1e9))
        else:
            Q.update(verbose=False)

        def pass_leg(leg, what, nbytes):
            r = timed(lambda: plan._run_pass(refresh=False), a.steps, a.warmup)
            steps_total = float(B) * T
            s = 1e-3 * r['ms_median']
            emit(dict(leg=leg, what=what, bytes_per_chain_step=nbytes,
                      GB_per_s=steps_total * nbytes / s / 1e9, exp_per_chain_step=(3 * K + 2) * K,
                      Gexp_per_s=steps_total * (3 * K + 2) * K / s / 1e9, **r))
        if 'pass' in legs and seg:
            for L in a.seg_len.split(','):
                plan.seg_len = int(L)
                shape['seg_len'] = plan.chains_per_wg
                pass_leg('pass', 'vmp_hmm_seg_pass', step_bytes)
            del shape['seg_len']
        elif 'pass' in legs:
            pass_leg('pass', 'vmp_hmm_wide_pass' if wide else 'vmp_hmm_fused_pass', step_bytes)
        if a.wide_pass and not wide:
            from bayespy_amd.inference.plans.hmm_wide import WideHMMKernels
            narrow_k, narrow_ws = plan._kernels, plan.ws
            plan._kernels = WideHMMKernels(plan.rt)
            plan.ws = plan.rt.empty(int(plan._kernels.plan(B, T, D, K)[1]))
            pass_leg('pass_wide', 'vmp_hmm_wide_pass', 16 * D + 24 * KP + 32 * K)
            plan._kernels, plan.ws = narrow_k, narrow_ws
        rs = np.random.RandomState(1)
        for name, frac in masks:
            if frac is None:
                m = np.arange(T)[None, :] < rs.randint(1, T + 1, size=B)[:, None]
            else:
                m = rs.rand(B, T) < frac
            plan.Y.observe(np.where(m[..., None], y, np.nan), mask=m)
            assert plan.Y._plan is plan and plan.has_state()     # the posteriors stay
            plan._materialize()
            assert plan.maskd is not None
            r = timed(lambda: plan._run_pass(refresh=False), a.steps, a.warmup)
            emit(dict(leg='pass_masked', what='vmp_hmm_fused_pass_masked', mask=name,
                      observed_fraction=float(m.mean()),
                      chains_without_observation=int((~m.any(axis=1)).sum()), **r))
        del Q, plan
        torch.cuda.empty_cache()
    if 'generic' in legs:
        try:
            torch.cuda.reset_peak_memory_stats()
            Q = build(y, mu, z0, 'generic')
            emit(dict(leg='generic', what='Q.update()',
                      **timed(lambda: Q.update(verbose=False), a.steps, a.warmup)))
            emit(dict(leg='generic_bound', L=float(Q.L[Q.iter - 1]),
                      peak_GB=torch.cuda.max_memory_allocated() / 1e9))
        except (RuntimeError, MemoryError) as exc:         # out of memory at this size
            emit(dict(leg='generic', error=str(exc)[:200]))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
