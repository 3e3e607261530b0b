#!/usr/bin/env python
"""
Fixtures of the deterministic-annealing scripts from the LIVE reference: tests/golden/anneal.npz.
Runs the model scripts of tests/anneal_models.py on the reference, imported the way
oracle/make_golden.py imports it, and stores the inputs (in_*), the bound after every iteration,
every per-node bound term and the final moments of every node.  Every stored value must be finite.

    python tools/make_golden_anneal.py
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
    import anneal_models
    g = anneal_models.make_inputs(np.random.RandomState(2718))
    mods = dict(nodes=bayespy.nodes, VB=VB)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = anneal_models.run_cases(mods, g)
        res.update(anneal_models.run_diag_cases(mods, g))
    out = {'in_' + k: v for k, v in g.items()}
    for k, v in res.items():
        if not k.endswith('_plan'):
            out[k] = np.array(v)
    for k, v in out.items():
        assert np.all(np.isfinite(v)), 'not finite: ' + k
    fn = os.path.join(OUT, 'anneal.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for k in sorted(out):
        if k.endswith('_L'):
            print(k, out[k])


if __name__ == '__main__':
    main()
