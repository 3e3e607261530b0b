#!/usr/bin/env python
"""
Fixture of the hidden-Markov-model script with multinomial emissions and 65 states from the LIVE
reference on the CPU: tests/golden/hmm_states.npz.  Runs the model script of
tests/hmm_states_models.py on the reference and stores what tools/make_golden_hmm_mult.py stores.

    python tools/make_golden_hmm_states.py
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
    import hmm_states_models
    g = hmm_states_models.make_inputs(np.random.RandomState(4121))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = hmm_states_models.run_cases(dict(nodes=bayespy.nodes, VB=VB), g)
    out = {'in_' + k: v for k, v in g.items()}
    for k, v in res.items():
        if not k.endswith('_plan') and not k.endswith('_model'):
            out[k] = np.array(v)
    fn = os.path.join(OUT, 'hmm_states.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    print('s_L', out['s_L'])


if __name__ == '__main__':
    main()
