#!/usr/bin/env python
"""
Sweep times of the fused latent-Dirichlet-allocation block (inference/plans/lda.py) and, where it
can hold the model, of the generic engine on the same inputs in the same process.

    python tools/bench_lda.py                       # the standard sizes
    python tools/bench_lda.py --tokens 1000000 --documents 10000 --vocabulary 10000 --topics 16

One process, seeded inputs, HIP events around whole sweeps (``Q.update()``: topics, p_word,
p_topic and the bound) after warm-up sweeps; the median over the timed sweeps is reported.  The
parts of the token pass are timed one by one through the ``phases`` argument of
``vmp_lda_token_pass``.  One JSON line per size:

  ms_per_sweep            block, whole sweep
  ms_pass_doc/_word/_dots the document-order pass, the word-order pass, the two dot products
  bytes_per_token         what the two passes move per token by design: pass A reads doc and word
                          (4 + 4) and writes lse (8); pass B reads word, doc, pos (12) and lse (8)
                          = 36 B, table rows (cached) not counted
  hbm_fraction            bytes_per_token * tokens / (ms_pass_doc + ms_pass_word) / peak bandwidth
  generic_ms_per_sweep    engine='generic' on the same model (--generic-max-tokens bounds its size)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12           # MI355X peak HBM3E bandwidth
BYTES_PER_TOKEN = 4 + 4 + 8 + 12 + 8


def build(n, D, V, K, docs, corpus, engine=None):
    from bayespy_amd import nodes
    from bayespy_amd.inference import VB
    p_topic = nodes.Dirichlet(np.ones(K), plates=(D,), name='p_topic')
    p_word = nodes.Dirichlet(np.ones(V), plates=(K,), name='p_word')
    topics = nodes.Categorical(nodes.Gate(docs, p_topic), plates=(n,), name='topics')
    words = nodes.Categorical(nodes.Gate(topics, p_word), name='words')
    words.observe(corpus)
    np.random.seed(1)
    p_topic.initialize_from_random()
    p_word.initialize_from_random()
    Q = VB(words, topics, p_word, p_topic, engine=engine)
    Q.ignore_bound_checks = True
    return Q


def time_sweeps(Q, warmup, steps):
    import torch
    Q.update(repeat=warmup, verbose=False)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream())
        Q.update(repeat=1, verbose=False)
        b.record(torch.cuda.current_stream())
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def time_phases(plan, steps):
    import torch
    out = {}
    rt = plan.rt
    for name, ph in (('ms_pass_doc', 1), ('ms_pass_word', 2), ('ms_dots', 4)):
        ms = []
        for i in range(steps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            rt.sync_stream()
            a.record(torch.cuda.current_stream())
            plan.kernels.token_pass(plan.n, plan.D, plan.V, plan.K, plan.lay, None,
                                    plan.used_theta, plan.used_beta_t, ph, plan.lse, plan.ws,
                                    plan.Ndk, plan.Nvk, plan.scal)
            b.record(torch.cuda.current_stream())
            b.synchronize()
            if i >= 2:
                ms.append(a.elapsed_time(b))
        out[name] = float(np.median(ms))
    return out


def run(n, D, V, K, warmup, steps, generic):
    import torch
    from bayespy_amd.inference.plans.lda import LDAPlan
    rs = np.random.RandomState(12345)
    docs = rs.randint(D, size=n)
    corpus = (rs.zipf(1.2, size=n) - 1) % V
    Q = build(n, D, V, K, docs, corpus)
    assert isinstance(Q.plans[0], LDAPlan)
    med, best = time_sweeps(Q, warmup, steps)
    res = dict(tokens=n, documents=D, vocabulary=V, topics=K, ms_per_sweep=med,
               ms_per_sweep_min=best, L=float(Q.L[Q.iter - 1]))
    res.update(time_phases(Q.plans[0], steps))
    res['bytes_per_token'] = BYTES_PER_TOKEN
    t = (res['ms_pass_doc'] + res['ms_pass_word']) * 1e-3
    res['hbm_fraction'] = BYTES_PER_TOKEN * n / t / HBM_BYTES_PER_S if t > 0 else None
    res['peak_memory_mb'] = torch.cuda.max_memory_allocated() / 1e6
    del Q
    if generic:
        Qg = build(n, D, V, K, docs, corpus, engine='generic')
        gmed, gbest = time_sweeps(Qg, warmup, steps)
        res['generic_ms_per_sweep'] = gmed
        res['generic_ms_per_sweep_min'] = gbest
        res['generic_L'] = float(Qg.L[Qg.iter - 1])
        del Qg
    torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--tokens', type=int)
    ap.add_argument('--documents', type=int)
    ap.add_argument('--vocabulary', type=int)
    ap.add_argument('--topics', type=int)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--generic', action='store_true', help='also time engine="generic"')
    ap.add_argument('--generic-max-tokens', type=int, default=200000,
                    help='largest standard size at which the generic engine is timed too')
    a = ap.parse_args()
    if a.tokens:
        run(a.tokens, a.documents, a.vocabulary, a.topics, a.warmup, a.steps, a.generic)
        return
    # the doc example's size, a size the generic engine still holds (its tokens x V fp64 arrays:
    # 2e5 x 2e3 x 8 B = 3.2 GB each), and corpus scale
    for n, D, V, K in ((10000, 10, 100, 5), (200000, 2000, 2000, 16),
                       (10 ** 7, 10 ** 5, 10 ** 5, 16), (10 ** 7, 10 ** 5, 10 ** 5, 64)):
        run(n, D, V, K, a.warmup, a.steps, n <= a.generic_max_tokens)


if __name__ == '__main__':
    main()
