#!/usr/bin/env python
"""
Fixtures of the latent-Dirichlet-allocation models from the LIVE reference: tests/golden/lda.npz.
Runs the model scripts of tests/lda_models.py on the reference, imported the way
oracle/make_golden.py imports it, and stores the inputs (in_*), the bound after every sweep, every
per-node bound term and the final moments of the four nodes (the tokens x vocabulary one-hot
moments of ``words`` are stored as the indices of their ones: they hold nothing else).

    python tools/make_golden_lda.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    from oracle.make_golden import _import_reference, OUT
    _import_reference()
    import bayespy.nodes
    from bayespy.inference import VB
    from bayespy.inference.vmp.nodes.categorical import CategoricalMoments
    import lda_models
    g = lda_models.make_lda_inputs(np.random.RandomState(1207))
    mods = dict(nodes=bayespy.nodes, VB=VB, CategoricalMoments=CategoricalMoments)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = lda_models.run_lda_cases(mods, g)
        res.update(lda_models.run_lda_svi(mods, g))
    out = {'in_' + k: v for k, v in g.items()}
    for k, v in res.items():
        if k.endswith('_plan'):
            continue
        if k.endswith('_words_u0'):
            assert np.all((v == 0) | (v == 1)) and np.all(v.sum(-1) == 1)
            v = np.argmax(v, axis=-1).astype(np.int32)
        out[k] = np.array(v)
    fn = os.path.join(OUT, 'lda.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for k in sorted(out):
        if k.endswith('_L'):
            print(k, out[k])


if __name__ == '__main__':
    main()
