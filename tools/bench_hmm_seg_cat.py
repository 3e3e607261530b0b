#!/usr/bin/env python
"""
The segmented against the sequential chain pass of the discrete hidden-Markov-model block, on the
same device state in one process; one JSON line per leg.

  seg   ``vmp_hmm_seg_pass_categorical`` (csrc/vmp_hmm_seg_cat.hip), one line per value of
        --seg-len (comma-separated; 0 = the library's choice) with the segment length in use
  seq   ``vmp_hmm_fused_pass_categorical`` (csrc/vmp_hmm_cat.hip) on the same words and tables
  diff  the largest absolute difference of every sum between the two passes

    python tools/bench_hmm_seg_cat.py [--B 1] [--T 200000] [--K 16] [--M 64]
                                      [--seg-len 128,256,512,0] [--steps 10] [--warmup 3]
                                      [--no-seq] [--out file.json]

Every leg warms up, then times ``steps`` calls one by one between device synchronisations and
reports the median and the extremes.  Dirichlet <log> tables and sticky chains, seeded.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_inputs(B, T, M, K, seed=0):
    from scipy import special
    rs = np.random.RandomState(seed)

    def elog(al):
        return special.digamma(al) - special.digamma(al.sum(-1, keepdims=True))
    Pt = elog(rs.gamma(0.3, size=(K, M)) + 0.05).T.copy()
    la0 = elog(rs.gamma(1.0, size=K) + 0.05)
    lA = elog(rs.gamma(1.0, size=(K, K)) + 0.05 + 10.0 * np.identity(K))
    return rs.randint(M, size=(B, T)), Pt, la0, lA


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
    ap.add_argument('--B', type=int, default=1)
    ap.add_argument('--T', type=int, default=200000)
    ap.add_argument('--K', type=int, default=16)
    ap.add_argument('--M', type=int, default=64)
    ap.add_argument('--seg-len', default='128,256,512,0')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-seq', action='store_true', help='skip the sequential pass')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this tool needs a GPU'
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.hmm_cat import CatHMMKernels
    from bayespy_amd.inference.plans.hmm_seg_cat import SegmentedCatHMMKernels
    B, T, M, K = a.B, a.T, a.M, a.K
    rt = get_runtime()
    y, Pt, la0, lA = make_inputs(B, T, M, K)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(rt.device)  # noqa: E731
    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.int32)).to(rt.device)
    Pd, a0d, Ad = up(Pt), up(la0), up(lA)
    shape = dict(B=B, T=T, M=M, K=K)
    lines = []

    def emit(rec):
        lines.append(json.dumps(dict(shape, **rec)))
        print(lines[-1], flush=True)

    def leg(k, name, what, **extra):
        used, wsd = k.plan(B, T, M, K)
        ws = rt.empty(int(wsd))
        out = dict(z0sum=rt.zeros(K), xisum=rt.zeros(K, K), S=rt.zeros(M, K), scal=rt.zeros(8))

        def call():
            k.pass_(B, T, M, K, yd, Pd, a0d, Ad, None, None, ws, out['z0sum'], out['xisum'],
                    out['S'], out['scal'])
        r = timed(call, a.steps, a.warmup)
        emit(dict(leg=name, what=what, workspace_GB=8e-9 * int(wsd), **extra, **r,
                  **({'seg_len': int(used)} if name == 'seg' else {})))
        return {key: v.cpu().numpy().copy() for key, v in out.items()}

    seg = None
    for L in a.seg_len.split(','):
        k = SegmentedCatHMMKernels(rt)
        k.seg_len = int(L)
        seg = leg(k, 'seg', 'vmp_hmm_seg_pass_categorical', seg_len_asked=int(L))
    if not a.no_seq:
        seq = leg(CatHMMKernels(rt), 'seq', 'vmp_hmm_fused_pass_categorical')
        seg['scal'], seq['scal'] = seg['scal'][:4], seq['scal'][:4]
        emit(dict(leg='diff', logZ=float(seq['scal'][0]),
                  **{key: float(np.max(np.abs(seg[key] - seq[key]))) for key in seg}))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
