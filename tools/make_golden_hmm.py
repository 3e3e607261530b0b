#!/usr/bin/env python
"""
Fixtures of the Gaussian hidden-Markov-model scripts from the LIVE reference:
tests/golden/hmm_fused.npz, or with ``masked`` tests/golden/hmm_masked.npz.  Runs the model scripts
of tests/hmm_models.py on the reference, imported the way oracle/make_golden.py imports it, and
stores the inputs (in_*; masked: NaN at every masked position of y), the bound after every sweep,
every per-node bound term, the final moments of Z, A and a0 (and mu, Lambda) and, masked, the masks
of Z and Y.

    python tools/make_golden_hmm.py [fused|masked]
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main(which='fused'):
    from oracle.make_golden import _import_reference, OUT
    _import_reference()
    import bayespy.nodes
    from bayespy.inference import VB
    import hmm_models
    if which == 'masked':
        g = hmm_models.make_masked_inputs(np.random.RandomState(4116))
    elif which == 'fused':
        g = hmm_models.make_hmm_inputs(np.random.RandomState(4115))
    else:
        raise SystemExit('usage: make_golden_hmm.py [fused|masked]')
    mods = dict(nodes=bayespy.nodes, VB=VB)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = hmm_models.run_hmm_cases(mods, g)
    out = {'in_' + k: v for k, v in g.items()}
    for k, v in res.items():
        if not k.endswith('_plan'):
            out[k] = np.array(v)
    fn = os.path.join(OUT, 'hmm_%s.npz' % which)
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for k in sorted(out):
        if k.endswith('_L') or k.endswith('_Z_mask'):
            print(k, out[k])


if __name__ == '__main__':
    main(*sys.argv[1:2])
