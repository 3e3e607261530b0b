#!/usr/bin/env python
"""
Fixtures of the GaussianMarkovChain with input signals from the LIVE reference:
tests/golden/chain_in.npz.  Runs the model scripts of tests/chain_in_models.py on the reference,
imported the way oracle/make_golden.py imports it, and stores the inputs (in_*), the bound after
every sweep, the per-node bound terms and the final moments; and the moments of the reference's own
closed-form case (cf_u0, cf_u1, cf_u2).  The reference's bound must not decrease on any case, or
nothing is written.

    python tools/make_golden_chain_in.py
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
    import chain_in_models as m
    g = m.make_chain_in_inputs(np.random.RandomState(7412))
    out = {'in_' + k: v for k, v in g.items()}
    for tag in m.TAGS:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res = m.run_chain_in_case(bayespy.nodes, VB, g, tag, expand_shared_inputs=True)
        L = res[tag + '_L']
        assert np.all(np.isfinite(L)), (tag, L)
        assert np.all(np.diff(L) >= -1e-9 * np.abs(L[1:])), 'bound of %s decreases: %s' % (tag, L)
        print(tag, L)
        out.update(res)
    c = m.CLOSED_FORM
    X = bayespy.nodes.GaussianMarkovChain([c['mu']], [[c['Lambda']]], [[c['A'], c['B']]], [c['v']],
                                          inputs=c['inputs'])
    X.update()
    for i, ui in enumerate(X.get_moments()):
        out['cf_u%d' % i] = np.array(ui)
    fn = os.path.join(OUT, 'chain_in.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')


if __name__ == '__main__':
    main()
