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

    python tools/bench_lda.py --tokens 2000000 --documents 20000 --vocabulary 20000 \
        --topics 256 --engine fused+topics          # the wide-topic form (65 .. 1024 topics)

``--concentrations`` times the model with both concentrations learnt (DirichletConcentration
parents, ``engine='fused+topics+hyper'``) beside the same model with constant concentrations in the
same process, and the statistics pass, the prior fill and a whole concentration update alone.

With more than 64 topics on ``--engine fused+topics`` the table rows are the traffic (a row of 8 K
bytes is gathered per token and pass; the row indexed by the segment stays in registers), so the JSON
line also carries

  algorithmic_bytes_per_token   2 * 8 K (one gathered row per pass) + 36 (indices and lse)
  gb_per_sweep                  algorithmic_bytes_per_token * tokens / 1e9
  stream_fraction               gb_per_sweep / (ms_pass_doc + ms_pass_word) / 6.3 TB/s, the rate a
                                streaming kernel reaches on this chip

    python tools/bench_lda.py --svi                 # stochastic VI: the mini-batch form of the block

``--svi`` times whole SVI steps (``observe`` and ``set_value`` of a new batch that lives on the
device, ``update('topics')``, ``gradient_step`` on both Dirichlets) with ``engine='fused'`` and,
where the generic engine can hold the batch, ``engine='generic'``; then the transposed step kernel
of ``vmp_lda_dirichlet_step`` against ``vmp_lda_dirichlet`` on the same V x K table (scale = 1,
mult = 1: the same work).  One JSON line per size:

  ms_per_step / _min / _max / _spread   median, extremes and (max - min) / median of the timed steps
  generic_ms_per_step ...               the same for engine='generic'
  ms_step_kernel, ms_dirichlet          the two kernels on a V x K table; step_bytes_per_s against
                                        hbm_fraction = bytes / s / 8 TB/s, bytes = 8 V K (prior +
                                        counts + alpha read and written + elog) = 40 V K
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12           # MI355X peak HBM3E bandwidth
STREAM_BYTES_PER_S = 6.3e12        # what a streaming kernel reaches of it
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


def build_learnt(n, D, V, K, docs, corpus, engine):
    """The model of ``build`` with both concentrations learnt (DirichletConcentration parents)."""
    from bayespy_amd import nodes
    from bayespy_amd.inference import VB
    a = nodes.DirichletConcentration(K, name='conc_topic')
    b = nodes.DirichletConcentration(V, name='conc_word')
    p_topic = nodes.Dirichlet(a, plates=(D,), name='p_topic')
    p_word = nodes.Dirichlet(b, plates=(K,), name='p_word')
    topics = nodes.Categorical(nodes.Gate(docs, p_topic), plates=(n,), name='topics')
    words = nodes.Categorical(nodes.Gate(topics, p_word), name='words')
    words.observe(corpus)
    np.random.seed(1)
    p_topic.initialize_from_random()
    p_word.initialize_from_random()
    Q = VB(words, topics, p_word, p_topic, a, b, engine=engine)
    Q.ignore_bound_checks = True
    return Q


def time_calls(fn, steps):
    """Median milliseconds of ``fn()`` between two events, after two untimed calls."""
    import torch
    ms = []
    for i in range(steps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream())
        fn()
        b.record(torch.cuda.current_stream())
        b.synchronize()
        if i >= 2:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def run_concentrations(n, D, V, K, warmup, steps):
    """Sweeps with both concentrations learnt beside the same tree with constant concentrations,
    and the statistics pass alone against the two table reads it must make."""
    import torch
    rs = np.random.RandomState(12345)
    docs = rs.randint(D, size=n)
    corpus = (rs.zipf(1.2, size=n) - 1) % V
    engine = 'fused+topics+hyper'
    res = dict(mode='concentrations', tokens=n, documents=D, vocabulary=V, topics=K, engine=engine)
    Qc = build(n, D, V, K, docs, corpus, engine='fused+topics')
    res['constant_plan'] = type(Qc.plans[0]).__name__
    res['constant_ms_per_sweep'], res['constant_ms_per_sweep_min'] = time_sweeps(Qc, warmup, steps)
    res.update({'constant_' + k: v for k, v in time_phases(Qc.plans[0], steps).items()})
    del Qc
    torch.cuda.empty_cache()
    Q = build_learnt(n, D, V, K, docs, corpus, engine)
    plan = Q.plans[0]
    res['plan'] = type(plan).__name__
    res['ms_per_sweep'], res['ms_per_sweep_min'] = time_sweeps(Q, warmup, steps)
    res['L'] = float(Q.L[Q.iter - 1])
    res.update(time_phases(plan, steps))
    rt, k = plan.rt, plan.kernels
    for key, name in (('conc_topic', 'topic'), ('conc_word', 'word')):
        rows, cols, r_s, c_s, alpha, elog, prior = plan._table(key)
        h = plan.hyper[key]
        rt.sync_stream()
        ms = time_calls(lambda: k.stats(rows, cols, r_s, c_s, alpha, elog, h['ws'], h['S'],
                                        h['qterm']), steps)
        res['ms_stats_' + name] = ms
        res['stats_%s_gb_per_s' % name] = 2 * 8.0 * rows * cols / (ms * 1e-3) / 1e9
        res['ms_fill_' + name] = time_calls(
            lambda: k.prior_fill(rows, cols, r_s, c_s, h['a'], prior), steps)
        node = plan.roles[key]
        res['ms_update_' + name] = time_calls(lambda: plan.update(node), steps)
        res['fixed_point_steps_' + name] = int(h['status'][2].item())
    t = res['ms_pass_doc'] + res['ms_pass_word']
    res['stats_over_token_pass'] = (res['ms_stats_topic'] + res['ms_stats_word']) / t
    res['peak_memory_mb'] = torch.cuda.max_memory_allocated() / 1e6
    print(json.dumps(res), flush=True)
    return res


def run(n, D, V, K, warmup, steps, generic, engine=None):
    import torch
    from bayespy_amd.inference.plans.lda import LDAPlan
    rs = np.random.RandomState(12345)
    docs = rs.randint(D, size=n)
    corpus = (rs.zipf(1.2, size=n) - 1) % V
    if engine == 'generic':
        Q = build(n, D, V, K, docs, corpus, engine='generic')
        med, best = time_sweeps(Q, warmup, steps)
        res = dict(tokens=n, documents=D, vocabulary=V, topics=K, engine=engine,
                   generic_ms_per_sweep=med, generic_ms_per_sweep_min=best,
                   generic_L=float(Q.L[Q.iter - 1]),
                   peak_memory_mb=torch.cuda.max_memory_allocated() / 1e6)
        print(json.dumps(res), flush=True)
        return res
    Q = build(n, D, V, K, docs, corpus, engine=engine)
    assert isinstance(Q.plans[0], LDAPlan)
    med, best = time_sweeps(Q, warmup, steps)
    res = dict(tokens=n, documents=D, vocabulary=V, topics=K, ms_per_sweep=med,
               ms_per_sweep_min=best, L=float(Q.L[Q.iter - 1]))
    if engine is not None:
        res['engine'] = engine
        res['plan'] = type(Q.plans[0]).__name__
    res.update(time_phases(Q.plans[0], steps))
    res['bytes_per_token'] = BYTES_PER_TOKEN
    t = (res['ms_pass_doc'] + res['ms_pass_word']) * 1e-3
    res['hbm_fraction'] = BYTES_PER_TOKEN * n / t / HBM_BYTES_PER_S if t > 0 else None
    if K > 64:
        alg = 2 * 8 * K + BYTES_PER_TOKEN
        res['algorithmic_bytes_per_token'] = alg
        res['gb_per_sweep'] = alg * n / 1e9
        res['stream_fraction'] = alg * n / t / STREAM_BYTES_PER_S if t > 0 else None
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


def build_svi(n, S, D, V, K, docs, corpus, engine):
    from bayespy_amd import nodes
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments
    p_topic = nodes.Dirichlet(np.ones(K), plates=(D,), name='p_topic')
    p_word = nodes.Dirichlet(np.ones(V), plates=(K,), name='p_word')
    idx = nodes.Constant(CategoricalMoments(D), docs[:S], name='document_indices')
    topics = nodes.Categorical(nodes.Gate(idx, p_topic), plates=(S,), plates_multiplier=(n / S,),
                               name='topics')
    words = nodes.Categorical(nodes.Gate(topics, p_word), name='words')
    words.observe(corpus[:S])
    np.random.seed(1)
    p_topic.initialize_from_random()
    p_word.initialize_from_random()
    Q = VB(words, topics, p_word, p_topic, idx, engine=engine)
    Q.ignore_bound_checks = True
    return Q


def time_svi_steps(Q, n, S, docs_d, corpus_d, warmup, steps, device_batches):
    """Median / min / max milliseconds of whole SVI steps on seeded batches."""
    import torch
    g = torch.Generator(device='cuda')
    g.manual_seed(7)
    Q.update(verbose=False)
    ms = []
    for it in range(warmup + steps):
        subset = torch.randint(n, (S,), generator=g, device='cuda')
        bw, bd = corpus_d[subset], docs_d[subset]
        if not device_batches:
            bw, bd = bw.cpu().numpy(), bd.cpu().numpy()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream())
        Q['words'].observe(bw)
        Q['document_indices'].set_value(bd)
        Q.update('topics', verbose=False)
        Q.gradient_step('p_topic', 'p_word', scale=(it + 1) ** (-0.7))
        b.record(torch.cuda.current_stream())
        b.synchronize()
        if it >= warmup:
            ms.append(a.elapsed_time(b))
    med = float(np.median(ms))
    return dict(ms_per_step=med, ms_per_step_min=float(np.min(ms)),
                ms_per_step_max=float(np.max(ms)),
                ms_per_step_spread=float((np.max(ms) - np.min(ms)) / med)), float(Q.L[Q.iter - 1])


def run_svi(n, S, D, V, K, warmup, steps, generic):
    import torch
    from bayespy_amd.inference.plans.lda import LDASVIPlan
    rs = np.random.RandomState(12345)
    docs = rs.randint(D, size=n)
    corpus = (rs.zipf(1.2, size=n) - 1) % V
    docs_d, corpus_d = torch.from_numpy(docs).cuda(), torch.from_numpy(corpus).cuda()
    Q = build_svi(n, S, D, V, K, docs, corpus, 'fused')
    assert type(Q.plans[0]) is LDASVIPlan
    res = dict(mode='svi', tokens=n, batch=S, documents=D, vocabulary=V, topics=K)
    t, L = time_svi_steps(Q, n, S, docs_d, corpus_d, warmup, steps, True)
    res.update(t)
    res['L'] = L
    del Q
    if generic:
        Qg = build_svi(n, S, D, V, K, docs, corpus, 'generic')
        t, L = time_svi_steps(Qg, n, S, docs_d, corpus_d, warmup, steps, False)
        res.update({'generic_' + k: v for k, v in t.items()})
        res['generic_L'] = L
        del Qg
    torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    return res


def run_step_kernel(V, K, warmup, steps):
    """The transposed step kernel against vmp_lda_dirichlet on the same V x K table."""
    import torch
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.lda import LDAKernels
    rt = get_runtime()
    k = LDAKernels(rt)
    g = torch.Generator(device='cuda')
    g.manual_seed(3)
    prior = torch.rand(V, K, generator=g, device='cuda', dtype=torch.float64) + 0.05
    counts = torch.rand(V, K, generator=g, device='cuda', dtype=torch.float64) * 30.0
    alpha, elog = torch.empty_like(prior), torch.empty_like(prior)
    out = rt.zeros(1)
    ws = rt.empty(max(k.dirichlet_step_ws(K, V, 1, K), 1024))

    def timed(fn):
        ms = []
        for it in range(warmup + steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            rt.sync_stream()
            a.record(torch.cuda.current_stream())
            fn()
            b.record(torch.cuda.current_stream())
            b.synchronize()
            if it >= warmup:
                ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))
    new = timed(lambda: k.dirichlet_step(K, V, 1, K, prior, counts, 1.0, 1.0, alpha, elog, ws, out))
    a_new, b_new = alpha.clone(), float(out.item())
    old = timed(lambda: k.dirichlet(K, V, 1, K, prior, counts, alpha, elog, ws, out))
    same = bool(torch.equal(a_new, alpha)) and abs(b_new - float(out.item())) \
        <= 1e-10 * abs(b_new) + 1e-9
    nbytes = 8.0 * V * K * 5
    res = dict(mode='step_kernel', vocabulary=V, topics=K, ms_step_kernel=new[0],
               ms_step_kernel_min=new[1], ms_step_kernel_max=new[2], ms_dirichlet=old[0],
               ms_dirichlet_min=old[1], ms_dirichlet_max=old[2], bytes=nbytes,
               step_bytes_per_s=nbytes / (new[0] * 1e-3),
               hbm_fraction=nbytes / (new[0] * 1e-3) / HBM_BYTES_PER_S, same_result=same)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--svi', action='store_true',
                    help='time stochastic-VI steps (engine="fused") and the Dirichlet step kernel')
    ap.add_argument('--batch', type=int, help='tokens per mini-batch (with --svi --tokens)')
    ap.add_argument('--tokens', type=int)
    ap.add_argument('--documents', type=int)
    ap.add_argument('--vocabulary', type=int)
    ap.add_argument('--topics', type=int,
                    help='number of topics; above 64 needs --engine fused+topics (or generic)')
    ap.add_argument('--engine', default=None,
                    help="engine of the timed VB (default: the default engine; 'fused+topics' for "
                         "65 .. 1024 topics; 'generic' times the generic engine alone)")
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--generic', action='store_true', help='also time engine="generic"')
    ap.add_argument('--generic-max-tokens', type=int, default=200000,
                    help='largest standard size at which the generic engine is timed too')
    ap.add_argument('--concentrations', action='store_true',
                    help="both concentrations learnt (engine 'fused+topics+hyper') beside the same "
                         "model with constant concentrations; without sizes: 2e6 tokens, D = V = 2e4, "
                         "K = 64 and 256")
    a = ap.parse_args()
    if a.concentrations:
        if a.tokens:
            run_concentrations(a.tokens, a.documents, a.vocabulary, a.topics, a.warmup, a.steps)
            return
        for K in (64, 256):
            run_concentrations(2000000, 20000, 20000, K, a.warmup, a.steps)
        return
    if a.svi:
        steps = max(a.steps, 20)
        if a.tokens:
            run_svi(a.tokens, a.batch, a.documents, a.vocabulary, a.topics, a.warmup, steps,
                    a.generic)
            return
        # the corpus of examples/lda.py with batches of 1e4 and 1e5 tokens, and a size at which the
        # generic engine holds its tokens x V arrays (1e4 x 2e3 x 8 B = 160 MB each)
        run_svi(200000, 10000, 2000, 2000, 16, a.warmup, steps, True)
        run_svi(2000000, 10000, 20000, 20000, 20, a.warmup, steps, False)
        run_svi(2000000, 100000, 20000, 20000, 20, a.warmup, steps, False)
        for K in (16, 64):
            run_step_kernel(100000, K, a.warmup, steps)
        return
    if a.tokens:
        run(a.tokens, a.documents, a.vocabulary, a.topics, a.warmup, a.steps, a.generic,
            engine=a.engine)
        return
    # the doc example's size, a size the generic engine still holds (its tokens x V fp64 arrays:
    # 2e5 x 2e3 x 8 B = 3.2 GB each), and corpus scale
    for n, D, V, K in ((10000, 10, 100, 5), (200000, 2000, 2000, 16),
                       (10 ** 7, 10 ** 5, 10 ** 5, 16), (10 ** 7, 10 ** 5, 10 ** 5, 64)):
        run(n, D, V, K, a.warmup, a.steps, n <= a.generic_max_tokens)


if __name__ == '__main__':
    main()
