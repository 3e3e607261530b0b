"""GPU: ``vmp_hmm_diag_pass`` alone against the long-double restatement of tests/hmm_diag_host.py
(the allowance rule of DESIGN.md 4.14 / 4.15 unchanged), masks with NaN in the masked rows, the
prior pass, fixed labels, the plan entry, and the fixture models of tests/golden/hmm_diag.npz
through engine='fused+diagonal'.  Measured figures: DESIGN.md section 4.15g."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

pytestmark = pytest.mark.gpu

from hmm_diag_host import ALL, SUMS, compare, pass_inputs  # noqa: E402
from hmm_fused_host import mixed_mask  # noqa: E402

CHUNK = 32      # VMP_HMMD_D_CHUNK of csrc/vmp_hmm_diag_dev.h


def gpu_pass(y, tables, la0, lA, labels=None, want=False, mask=None):
    """``tables``: (h, q, g) or None (no emission term)."""
    import torch
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.hmm_diag import DiagHMMKernels
    rt = get_runtime()
    k = DiagHMMKernels(rt)
    B, T, D = y.shape
    K = len(la0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(rt.device)  # noqa: E731
    ws = rt.empty(int(k.plan(B, T, D, K)[1]))
    z0sum, xisum, scal = rt.zeros(K), rt.zeros(K, K), rt.zeros(8)
    S1, S2, Nk = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K)
    g, z0, zz = [rt.empty(*d) if want else None for d in ((B, T, K), (B, K), (B, T - 1, K, K))]
    lab = None if labels is None else torch.from_numpy(
        np.ascontiguousarray(labels, dtype=np.int32)).to(rt.device)
    md = None if mask is None else torch.from_numpy(
        np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)).to(rt.device)
    h, q, gk = (None,) * 3 if tables is None else (up(a) for a in tables)
    k.pass_(B, T, D, K, up(y), h, q, gk, up(la0), up(lA), lab, md, ws, z0sum, xisum, S1, S2, Nk,
            scal, g, z0, zz)
    rt.sync_stream()
    s = scal.cpu().numpy()
    out = dict(z0sum=z0sum.cpu().numpy(), xisum=xisum.cpu().numpy(), S1=S1.cpu().numpy(),
               S2=S2.cpu().numpy(), Nk=Nk.cpu().numpy(), logZ=float(s[0]), ge=float(s[1]),
               dots=s[2:4].copy())
    if want:
        out.update(gamma=g.cpu().numpy(), z0=z0.cpu().numpy(), zz=zz.cpu().numpy())
    return out


# (B, T, D, K): the smallest; D = c + 1 odd, one past a dimension chunk, 21 rows; D = 1024, K = 64
# (eight slabs, NT = 4, LDS above 48 KB); 70 rows (two emission blocks, five row ranges), two
# slabs, KP = 32; 33 rows, KP = 64 padded; two workgroups of chains at KP = 2
SHAPES = [(1, 2, 1, 1), (3, 7, CHUNK + 1, 3), (1, 5, 1024, 64), (2, 35, 130, 17), (3, 11, 6, 33),
          (33, 2, 3, 2)]


@pytest.mark.parametrize('B,T,D,K,mean', [s + (0.0,) for s in SHAPES] + [(2, 9, 130, 5, 50.0)])
def test_pass_against_long_double(B, T, D, K, mean):
    """mean = 50: y ~ N(50, 1) per dimension, so that terms 1/2 tau y^2 of order 1e3 to 1e5 cancel
    in e.  Measured on MI355X: every key within the allowance; the worst ratio of error to allowance
    over this test, the masked test and the prior pass is 0.36 (gamma of the masked pass at D = 130),
    0.33 among the shapes here (z0sum at (3, 11, 6, 33))."""
    y, tables, la0, lA = pass_inputs(B, T, D, K, mean)
    got = gpu_pass(y, tables, la0, lA, want=True)
    assert compare(got, y, tables, la0, lA, ALL, label=str((B, T, D, K, mean))) == []
    # the optional outputs off, a second call, a mask of ones: the bits of the NULL mask
    off, again = gpu_pass(y, tables, la0, lA), gpu_pass(y, tables, la0, lA)
    ones = gpu_pass(y, tables, la0, lA, mask=np.ones((B, T)))
    for k in SUMS + ('dots',):
        np.testing.assert_array_equal(off[k], got[k], err_msg=k)
        np.testing.assert_array_equal(again[k], off[k], err_msg=k)
        np.testing.assert_array_equal(ones[k], off[k], err_msg=k)


@pytest.mark.parametrize('D', [5, 130])
def test_masked_pass_against_long_double(D):
    B, T, K = 6, 13, 5
    y, tables, la0, lA = pass_inputs(B, T, D, K)
    mask = np.ones((B, T), bool)
    mask[0, 4:7] = False                    # a hole
    mask[1, 0] = mask[1, -1] = False        # the first and the last step
    mask[2] = False                         # nothing observed
    mask[3, 5:], mask[4, 1:] = False, False     # ragged tails, one leaves step 0 alone
    got = gpu_pass(np.where(mask[..., None], y, np.nan), tables, la0, lA, want=True, mask=mask)
    seen = np.where(mask[..., None], y, 0)  # the restatement never sees the masked rows
    assert compare(got, seen, tables, la0, lA, ALL, label='masked %d' % D, mask=mask) == []


def test_prior_pass_and_labels():
    B, T, D, K = 5, 7, 70, 3
    y, tables, la0, lA = pass_inputs(B, T, D, K)
    assert compare(gpu_pass(y, None, la0, lA), y, None, la0, lA, label='prior') == []
    lab = np.random.RandomState(1).randint(K, size=(B, T))
    onehot = np.eye(K)[lab]
    y = np.round(y * 16) / 16               # products and sums of these are exact in float64
    for mask in (None, mixed_mask(B, T, np.random.RandomState(2))):
        obs = np.ones((B, T), bool) if mask is None else mask
        r = gpu_pass(np.where(obs[..., None], y, np.nan), tables, la0, lA, labels=lab, want=True,
                     mask=mask)
        ob, yo = obs.any(axis=1), y * obs[..., None]
        np.testing.assert_array_equal(r['gamma'], onehot)
        np.testing.assert_array_equal(r['zz'], onehot[:, :-1, :, None] * onehot[:, 1:, None, :])
        np.testing.assert_array_equal(r['z0sum'], onehot[ob, 0].sum(0))
        np.testing.assert_array_equal(r['xisum'], np.einsum('bti,btj->ij', onehot[ob, :-1],
                                                            onehot[ob, 1:]))
        np.testing.assert_array_equal(r['S1'], np.einsum('btd,btk->dk', yo, onehot))
        np.testing.assert_array_equal(r['S2'], np.einsum('btd,btk->dk', yo * yo, onehot))
        np.testing.assert_array_equal(r['Nk'], (onehot * obs[..., None]).sum((0, 1)))
        assert r['logZ'] == 0 and r['ge'] == 0


def _on_diagonal(Q):
    assert type(Q.plans[0]).__name__ == 'DiagGaussianHMMPlan' and len(Q.plans) == 1


def test_fixture_models_through_the_diagonal_engine(tmp_path):
    """Fails without the feature: engine='fused+diagonal' matches nothing."""
    from bayespy_amd.inference.plans import compile_model
    from hmm_diag_models import CASES, build, run_cases
    from test_hmm_cat_host import _mods, L_RTOL, MOM_TOL
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'hmm_diag.npz'))
    gin = {k[3:]: g[k] for k in g.files if k.startswith('in_')}
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_cases(_mods(_on_diagonal, engine='fused+diagonal'), gin)
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
    assert checked == len([k for k in g.files if not k.startswith('in_')]) == 2 * 15 + 2
    assert g['q_Z_mask'].all() and not g['q_Y_mask'].all() and sorted(CASES) == ['p', 'q']
    # NaN in the masked rows: the same bounds
    nan = run_cases(_mods(_on_diagonal, engine='fused+diagonal'), gin, only=('q',), fill=np.nan)
    np.testing.assert_array_equal(nan['q_L'], res['q_L'])
    Q = res['p_plan']
    fn = str(tmp_path / 'diag.ckpt')
    Q.save(filename=fn)
    Q.update(repeat=2, verbose=False)
    L6 = Q.L[:6].copy()
    Q.load(filename=fn)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:6], L6)
    m = build(_mods(), gin, 'p')
    with pytest.raises(NotImplementedError, match='GaussianARD, not Gaussian'):
        compile_model([m[k] for k in ('Y', 'Z', 'mu', 'tau', 'A', 'a0')], engine='fused')


def test_plan_entry():
    from bayespy_amd import _lib
    lib = _lib.load()
    lim = [ctypes.c_int32() for _ in range(2)]
    assert lib.vmp_hmm_diag_limits(*[ctypes.byref(v) for v in lim]) == _lib.VMP_OK
    assert tuple(v.value for v in lim) == (64, 1024)

    def plan(B, T, D, K):
        c, w = ctypes.c_int64(), ctypes.c_int64()
        return lib.vmp_hmm_diag_plan(B, T, D, K, ctypes.byref(c), ctypes.byref(w)), w.value
    for B, T, D, K in SHAPES + [(2, 9, 130, 5), (6, 13, 5, 5), (6, 13, 130, 5), (5, 7, 70, 3),
                                (4096, 1000, 1024, 64)]:
        KP = max(2, 1 << (K - 1).bit_length())
        rc, w = plan(B, T, D, K)
        assert rc == _lib.VMP_OK and w >= B * T * (K + KP) > 0
    assert plan(1, 9, 3, 65)[0] == plan(1, 9, 1025, 3)[0] == _lib.VMP_ERR_UNSUPPORTED
    assert plan(1, 1, 3, 3)[0] == _lib.VMP_ERR_INVALID
