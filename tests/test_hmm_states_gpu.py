"""GPU: ``vmp_hmm_states_pass`` alone against the long-double restatement of tests/hmm_mult_host.py
(the allowance rule of DESIGN.md 4.14 / 4.15 unchanged), a mask with 0xFFFF in the masked rows, the
prior pass, fixed labels, the plan entry, and the fixture model of tests/golden/hmm_states.npz
through engine='fused+states'.  Measured figures: DESIGN.md section 4.15h."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

pytestmark = pytest.mark.gpu

from hmm_states_host import ALL, SUMS, compare, pass_inputs  # noqa: E402
from hmm_fused_host import mixed_mask  # noqa: E402


def gpu_pass(x, Pt, la0, lA, labels=None, want=False, mask=None, fill=None):
    """``Pt``: (M, K) or an integer M (no emission term); ``fill``: the packed masked rows."""
    import torch
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.hmm_states import WideStateHMMKernels
    rt = get_runtime()
    k = WideStateHMMKernels(rt)
    B, T, M = x.shape
    K = len(la0)
    xp = np.array(x, dtype=np.uint16)
    if fill is not None:
        xp[np.asarray(mask) == 0] = fill
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(rt.device)  # noqa: E731
    ws = rt.empty(int(k.plan(B, T, M, K)[1]))
    z0sum, xisum, S, scal = rt.zeros(K), rt.zeros(K, K), rt.zeros(M, K), rt.zeros(8)
    g, z0, zz = [rt.empty(*d) if want else None for d in ((B, T, K), (B, K), (B, T - 1, K, K))]
    lab = None if labels is None else torch.from_numpy(
        np.ascontiguousarray(labels, dtype=np.int32)).to(rt.device)
    md = None if mask is None else torch.from_numpy(
        np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)).to(rt.device)
    k.pass_(B, T, M, K, torch.from_numpy(xp.view(np.int16)).to(rt.device),
            None if isinstance(Pt, int) else up(Pt), up(la0), up(lA), lab, md, ws, z0sum, xisum, S,
            scal, g, z0, zz)
    rt.sync_stream()
    s = scal.cpu().numpy()
    out = dict(z0sum=z0sum.cpu().numpy(), xisum=xisum.cpu().numpy(), S=S.cpu().numpy(),
               logZ=float(s[0]), ge=float(s[1]), dots=s[2:4].copy())
    if want:
        out.update(gamma=g.cpu().numpy(), z0=z0.cpu().numpy(), zz=zz.cpu().numpy())
    return out


# (B, T, M, K, band): the smallest (one chain in a tile of 16, 63 padded states); two tiles, the
# second with one chain, no padding; three tiles, M past a word chunk; a left-to-right band of -inf
@pytest.mark.parametrize('B,T,M,K,band', [(1, 2, 1, 65, False), (17, 3, 3, 128, False),
                                          (33, 7, 65, 100, False), (2, 5, 9, 97, True)])
def test_pass_against_long_double(B, T, M, K, band):
    x, Pt, la0, lA = pass_inputs(B, T, M, K, band)
    got = gpu_pass(x, Pt, la0, lA, want=True)
    assert compare(got, x, Pt, la0, lA, ALL, label=str((B, T, M, K))) == []
    # the optional outputs off, a second call, a mask of ones: the bits of the NULL mask
    off, again = gpu_pass(x, Pt, la0, lA), gpu_pass(x, Pt, la0, lA)
    ones = gpu_pass(x, Pt, la0, lA, mask=np.ones((B, T)))
    for k in SUMS + ('dots',):
        np.testing.assert_array_equal(off[k], got[k], err_msg=k)
        np.testing.assert_array_equal(again[k], off[k], err_msg=k)
        np.testing.assert_array_equal(ones[k], off[k], err_msg=k)


def test_masked_pass_against_long_double():
    B, T, M, K = 6, 13, 5, 70
    x, Pt, la0, lA = pass_inputs(B, T, M, K)
    mask = np.ones((B, T), bool)
    mask[0, 4:7] = False                    # a hole
    mask[1, 0] = mask[1, -1] = False        # the first and the last step
    mask[2] = False                         # nothing observed
    mask[3, 5:], mask[4, 1:] = False, False     # ragged tails, one leaves step 0 alone
    got = gpu_pass(x, Pt, la0, lA, want=True, mask=mask, fill=0xFFFF)
    seen = np.where(mask[..., None], x, 0)  # the restatement never sees the masked rows
    assert compare(got, seen, Pt, la0, lA, ALL, label='masked', mask=mask) == []


def test_prior_pass_and_labels():
    B, T, M, K = 5, 7, 6, 66
    x, Pt, la0, lA = pass_inputs(B, T, M, K)
    assert compare(gpu_pass(x, M, la0, lA), x, M, la0, lA, label='prior') == []
    lab = np.random.RandomState(1).randint(K, size=(B, T))
    onehot = np.eye(K)[lab]
    for mask in (None, mixed_mask(B, T, np.random.RandomState(2))):
        r = gpu_pass(x, Pt, la0, lA, labels=lab, want=True, mask=mask, fill=0xFFFF)
        obs = np.ones((B, T), bool) if mask is None else mask
        ob = obs.any(axis=1)
        np.testing.assert_array_equal(r['gamma'], onehot)
        np.testing.assert_array_equal(r['zz'], onehot[:, :-1, :, None] * onehot[:, 1:, None, :])
        np.testing.assert_array_equal(r['z0sum'], onehot[ob, 0].sum(0))
        np.testing.assert_array_equal(r['xisum'], np.einsum('bti,btj->ij', onehot[ob, :-1],
                                                            onehot[ob, 1:]))
        np.testing.assert_array_equal(r['S'], np.einsum('btm,btk->mk', x * obs[..., None], onehot))
        assert r['logZ'] == 0 and r['ge'] == 0


def _on_states(Q):
    assert type(Q.plans[0]).__name__ == 'WideStateMultinomialHMMPlan' and len(Q.plans) == 1


def test_fixture_model_through_the_states_engine(tmp_path):
    """Fails without the feature: engine='fused+states' matches nothing."""
    from hmm_states_models import run_cases
    from test_hmm_cat_host import _mods, L_RTOL, MOM_TOL
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'hmm_states.npz'))
    gin = {k[3:]: g[k] for k in g.files if k.startswith('in_')}
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_cases(_mods(_on_states, engine='fused+states'), gin)
    checked = 0
    for k, v in res.items():
        if k.endswith('_plan') or k.endswith('_model'):
            continue
        if k.endswith('_mask'):
            np.testing.assert_array_equal(v, g[k], err_msg=k)
        elif '_u' in k:
            np.testing.assert_allclose(v, g[k], err_msg=k, **MOM_TOL)
        else:
            np.testing.assert_allclose(v, g[k], err_msg=k, rtol=L_RTOL)
        checked += 1
    assert checked == len([k for k in g.files if not k.startswith('in_')]) == 11 + 2
    assert not g['s_Y_mask'].all()
    Q = res['s_plan']
    fn = str(tmp_path / 'states.ckpt')
    Q.save(filename=fn)
    Q.update(repeat=2, verbose=False)
    L6 = Q.L[:6].copy()
    Q.load(filename=fn)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:6], L6)


def test_plan_entry():
    from bayespy_amd import _lib
    lib = _lib.load()
    lim = [ctypes.c_int32() for _ in range(4)]
    assert lib.vmp_hmm_states_limits(*[ctypes.byref(v) for v in lim]) == _lib.VMP_OK
    assert tuple(v.value for v in lim) == (128, 65, 1024, 65534)

    def plan(B, T, M, K):
        c, w = ctypes.c_int64(), ctypes.c_int64()
        return lib.vmp_hmm_states_plan(B, T, M, K, ctypes.byref(c), ctypes.byref(w)), c.value, w.value
    for B, T, M, K in [(1, 2, 1, 65), (17, 3, 3, 128), (33, 7, 65, 100), (4096, 1000, 1024, 128),
                       (70000, 2, 3, 65)]:
        rc, c, w = plan(B, T, M, K)
        assert rc == _lib.VMP_OK and w >= B * T * (K + 128) > 0 and c % 16 == 0 and c > 0
    assert plan(1, 9, 3, 64)[0] == plan(1, 9, 3, 129)[0] == _lib.VMP_ERR_UNSUPPORTED
    assert plan(1, 1, 3, 65)[0] == _lib.VMP_ERR_INVALID
