"""GPU: the fused hidden-Markov-model block with categorical emissions on the real library -- the
fixtures of tests/golden/hmm_cat.npz and hmm.rst's exact posterior through engine='fused', and
``vmp_hmm_fused_pass_categorical`` alone against the long-double restatement of the reference
arithmetic (tests/hmm_cat_host.py ``restate``) and, bit for bit, against the g++ build of the
device header, at the smallest shapes that cross every lane bucket (KP = 2 ... 64, padded and
full), M = 1 / 3 / 128, T = 2 / 7 and one, 64 / KP + 1 and 2 (64 / KP) + 1 chains (a partly filled
lane group, two workgroups, a short last workgroup); masks, words at masked positions, tables below
the underflow of exp and the argument checks of the C ABI.

Measured on MI355X: see DESIGN.md section 4.15, "Categorical emissions"."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

pytestmark = pytest.mark.gpu


def gpu_pass(y, Pt, la0, lA, labels=None, want=False, mask=None):
    """``Pt``: (M, K) word-major, or an integer M for the pass without an emission term."""
    import torch
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.hmm_cat import CatHMMKernels
    rt = get_runtime()
    k = CatHMMKernels(rt)
    B, T = y.shape
    K = len(la0)
    M = Pt if isinstance(Pt, int) else Pt.shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(rt.device)  # noqa: E731
    _, wsd = k.plan(B, T, M, K)
    ws = rt.empty(int(wsd))
    z0sum, xisum, S, scal = rt.zeros(K), rt.zeros(K, K), rt.zeros(M, K), rt.zeros(8)
    g = rt.empty(B, T, K) if want else None
    z0 = rt.empty(B, K) if want else None
    zz = rt.empty(B, T - 1, K, K) if want else None
    i32 = lambda a: None if a is None else torch.from_numpy(  # noqa: E731
        np.ascontiguousarray(a, dtype=np.int32)).to(rt.device)
    md = None if mask is None else torch.from_numpy(
        np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)).to(rt.device)
    table = None if isinstance(Pt, int) else up(Pt)
    k.pass_(B, T, M, K, i32(y), table, up(la0), up(lA), i32(labels), md, ws, z0sum, xisum, S, scal,
            g, z0, zz)
    rt.sync_stream()
    s = scal.cpu().numpy()
    out = dict(z0sum=z0sum.cpu().numpy(), xisum=xisum.cpu().numpy(), S=S.cpu().numpy(),
               logZ=float(s[0]), ge=float(s[1]), dots=s[2:4].copy())
    if want:
        out.update(gamma=g.cpu().numpy(), z0=z0.cpu().numpy(), zz=zz.cpu().numpy())
    return out


def _on_device(Q):
    assert type(Q.plans[0]).__name__ == 'CategoricalHMMPlan' and len(Q.plans) == 1


def test_fixtures_through_the_library():
    """Fails without the feature: engine='fused' raises "Categorical, not Gaussian"."""
    from hmm_cat_models import run_cases
    from test_hmm_cat_host import _mods, _golden, check_fixtures
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_cases(_mods(_on_device, engine='fused'), gin, fill=-1)
    check_fixtures(res, g)


def test_fixture_with_a_device_mask_and_device_words():
    import torch
    from hmm_cat_models import run_cases
    from test_hmm_cat_host import _mods, _golden, MOM_TOL, L_RTOL
    g, gin = _golden()
    gin = dict(gin)
    gin['v_y'] = torch.from_numpy(np.where(gin['v_mask'], gin['v_y'], -1)).cuda()
    res = run_cases(_mods(_on_device, engine='fused'), gin, only=('v',),
                    device_mask=lambda m: torch.from_numpy(m).cuda())
    np.testing.assert_allclose(res['v_L'], g['v_L'], rtol=L_RTOL)
    np.testing.assert_allclose(res['v_P_u0'], g['v_P_u0'], **MOM_TOL)


def test_hmm_rst_exact_posterior():
    from hmm_cat_models import run_cases, RST_A0, RST_A, RST_P
    from test_hmm_cat_host import _mods, _golden
    g, gin = _golden()
    res = run_cases(_mods(_on_device, engine='fused'), gin, only=('i',))
    y = gin['i_y']
    al, logp = RST_A0 * RST_P[:, y[0]], 0.0
    for t in range(1, len(y)):
        logp += np.log(al.sum())
        al = (al / al.sum()) @ RST_A * RST_P[:, y[t]]
    logp += np.log(al.sum())
    np.testing.assert_allclose(res['i_L'][0], logp, rtol=1e-12)
    np.testing.assert_allclose(res['i_L'], g['i_L'], rtol=1e-9)


def _shapes():
    """Every KP once with M = 3 and once with M = 128, both T, the three B of each bucket; M = 1
    at the smallest and (K, M) = (64, 128), the LDS maximum, among them."""
    out = []
    for K, M, T in ((1, 1, 2), (2, 3, 7), (2, 128, 2), (3, 3, 2), (3, 128, 7), (5, 3, 7),
                    (5, 128, 2), (9, 3, 2), (9, 128, 7), (17, 3, 7), (17, 128, 2), (33, 3, 2),
                    (33, 128, 7), (64, 3, 7), (64, 128, 2)):
        KP = 2
        while KP < K:
            KP *= 2
        G = 64 // KP
        out += [(B, T, M, K) for B in (1, G + 1, 2 * G + 1)]
    return out


@pytest.mark.parametrize('B,T,M,K', _shapes())
def test_pass_against_long_double_and_the_host_build(B, T, M, K):
    from hmm_cat_host import compare, hmmc_host, host_pass, pass_inputs, ALL, SUMS
    from hmm_fused_host import mixed_mask
    y, Pt, la0, lA = pass_inputs(B, T, M, K)
    if B > 2:
        assert hmmc_host().hmmc_wgs(B, M, K) in (2, 3)
    got = gpu_pass(y, Pt, la0, lA, want=True)
    assert compare(got, y, Pt, la0, lA, ALL, label=str((B, T, M, K))) == []
    # the optional outputs off: the same bits; a second call: the same bits
    off, again = gpu_pass(y, Pt, la0, lA), gpu_pass(y, Pt, la0, lA)
    for k in SUMS + ('dots',):
        np.testing.assert_array_equal(off[k], got[k], err_msg=k)
        np.testing.assert_array_equal(again[k], off[k], err_msg=k)
    np.testing.assert_allclose(got['dots'], [np.sum(got['z0sum'] * la0), np.sum(got['xisum'] * lA)],
                               rtol=1e-12)
    # a mask of ones: the bits of the unmasked pass; a mixed mask with -1 at its masked positions
    ones = gpu_pass(y, Pt, la0, lA, want=True, mask=np.ones((B, T)))
    for k in ALL:
        np.testing.assert_array_equal(ones[k], got[k], err_msg=k)
    mask = mixed_mask(B, T, np.random.RandomState(B))
    ym = np.where(mask, y, -1)
    masked = gpu_pass(ym, Pt, la0, lA, want=True, mask=mask)
    assert compare(masked, y, Pt, la0, lA, ALL, label='masked ' + str((B, T, M, K)), mask=mask) == []
    # the device against the g++ build of the header.  The sums hold bit for bit where the device's
    # exp and log round as glibc's do; they are not the same functions, so as in the Gaussian
    # block's tests equality is held to the rule above (done), and the one-hot paths, where no
    # exp or log enters, to the bit.
    lab = np.random.RandomState(1).randint(K, size=(B, T))
    for mk, yy in ((None, y), (mask, ym)):
        h = host_pass(yy, Pt, la0, lA, labels=lab, mask=mk)
        d = gpu_pass(yy, Pt, la0, lA, labels=lab, mask=mk)
        for k in SUMS:
            np.testing.assert_array_equal(d[k], h[k], err_msg=k)
    h = host_pass(y, Pt, la0, lA)
    bits = {k: bool(np.array_equal(np.asarray(got[k]), np.asarray(h[k]))) for k in SUMS}
    print(str((B, T, M, K)), 'device sums equal to the host build bit for bit:', bits)


@pytest.mark.parametrize('B,T,M,K', [(5, 7, 4, 3), (3, 4, 128, 33)])
def test_prior_pass_labels_and_words_at_masked_positions(B, T, M, K):
    from hmm_cat_host import compare, pass_inputs, ALL, SUMS
    from hmm_fused_host import mixed_mask
    y, Pt, la0, lA = pass_inputs(B, T, M, K)
    assert compare(gpu_pass(y, M, la0, lA), y, M, la0, lA, label='prior') == []
    lab = np.random.RandomState(1).randint(K, size=(B, T))
    r = gpu_pass(y, Pt, la0, lA, labels=lab, want=True)
    onehot = np.eye(K)[lab]
    np.testing.assert_array_equal(r['gamma'], onehot)
    np.testing.assert_array_equal(r['z0'], onehot[:, 0])
    np.testing.assert_array_equal(r['zz'], onehot[:, :-1, :, None] * onehot[:, 1:, None, :])
    np.testing.assert_array_equal(r['z0sum'], onehot[:, 0].sum(0))
    np.testing.assert_array_equal(r['xisum'], np.einsum('bti,btj->ij', onehot[:, :-1], onehot[:, 1:]))
    np.testing.assert_array_equal(r['S'], np.einsum('btm,btk->mk', np.eye(M)[y], onehot))
    assert r['logZ'] == 0 and r['ge'] == 0
    # -1, 0, M - 1 and words far out of range at masked positions: the same bits
    mask = mixed_mask(B, T, np.random.RandomState(2))
    ref = gpu_pass(np.where(mask, y, 0), Pt, la0, lA, want=True, mask=mask)
    for fill in (-1, M - 1, M, 2 ** 31 - 1, -2 ** 31):
        got = gpu_pass(np.where(mask, y, fill), Pt, la0, lA, want=True, mask=mask)
        for k in ALL:
            np.testing.assert_array_equal(got[k], ref[k], err_msg='%s fill %d' % (k, fill))
    # a word out of range at an observed position indexes nothing: the step counts as masked
    pos = (0, T // 2)                               # chain 0 of mixed_mask is fully observed
    hole = mask.copy()
    hole[pos] = False
    assert mask[pos] and hole[0].any()
    want = gpu_pass(np.where(hole, y, -1), Pt, la0, lA, want=True, mask=hole)
    for bad in (M, -1, 10 ** 9):
        yb = np.where(mask, y, -1)
        yb[pos] = bad
        got = gpu_pass(yb, Pt, la0, lA, want=True, mask=mask)
        for k in ALL:
            np.testing.assert_array_equal(got[k], want[k], err_msg='%s word %d' % (k, bad))


def test_tables_below_the_underflow_of_exp():
    """Dirichlet(1e-3) rows: every <log A_ij> near -985 at K = 64 (exp of the table is 0: uniform
    xi is the answer without an emission term), and rows of <log P> near -700 with one used row of
    <log A> near 0 and the others near -670."""
    from scipy import special
    from hmm_cat_host import compare, pass_inputs, SUMS
    from bayespy_amd.inference.plans.hmm_cat import hmm_cat_limits
    K, M = hmm_cat_limits()[0], 3
    y, _, _, _ = pass_inputs(2, 5, M, K)
    al = np.full(K, 1e-3)
    la0 = special.digamma(al) - special.digamma(al.sum())
    lA = np.tile(la0, (K, 1))
    assert np.all(lA < -900) and np.all(np.exp(lA) == 0)
    got = gpu_pass(y, M, la0, lA, want=True)
    np.testing.assert_allclose(got['zz'], 1.0 / K ** 2, rtol=1e-12)
    assert compare(got, y, M, la0, lA, SUMS + ('zz',), label='flat') == []
    K, M = 3, 4
    y, _, _, _ = pass_inputs(3, 9, M, K)
    alA = np.full((K, K), 1e-3)
    alA[1] += [40.0, 25.0, 10.0]
    lA = special.digamma(alA) - special.digamma(alA.sum(-1, keepdims=True))
    assert lA[1].max() > -2 and lA[0].max() < -600
    la0 = special.digamma(np.full(K, 1e-3)) - special.digamma(3e-3)
    alP = np.full((K, M), 1e-3)
    alP[:, 0] += 30.0
    Pt = (special.digamma(alP) - special.digamma(alP.sum(-1, keepdims=True))).T.copy()
    assert Pt[1:].max() < -690 and np.all(np.exp(Pt[1:] + lA[0].max()) == 0)
    got = gpu_pass(y, Pt, la0, lA, want=True)
    assert np.all(np.isfinite(got['zz'])) and np.isfinite(got['logZ'])
    assert compare(got, y, Pt, la0, lA, SUMS + ('gamma', 'zz'), label='rows near -700') == []


def test_cabi_pass_checks_its_arguments_on_a_live_context():
    """Every refusal comes before a launch: null pointers, negative sizes, the limits."""
    import torch
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime, ptr
    rt = get_runtime()
    U, I = _lib.VMP_ERR_UNSUPPORTED, _lib.VMP_ERR_INVALID
    buf = rt.zeros(4096)
    p = ptr(buf)

    def call(B=4, T=3, M=2, K=3, y=p, Pt=p, a0=p, A=p, ws=p, z0sum=p, xisum=p, S=p, scal=p):
        return rt.lib.vmp_hmm_fused_pass_categorical(rt.ctx, B, T, M, K, y, Pt, a0, A, None, None,
                                                     ws, z0sum, xisum, S, scal, None, None, None)
    for name in ('a0', 'A', 'ws', 'z0sum', 'xisum', 'S', 'scal', 'y'):
        assert call(**{name: None}) == I, name
    for kw in (dict(B=-1), dict(T=1), dict(M=0), dict(K=0)):
        assert call(**kw) == I, kw
    assert call(K=65) == U and call(M=129) == U
    assert call(B=0, y=None) == _lib.VMP_OK            # no chains: zeros, y is not read
    rt.sync_stream()
    assert not torch.any(buf[:64] != 0)


def test_symbols_and_limits():
    """Fails without the feature: the library has no such symbols."""
    from bayespy_amd import _lib
    lib = _lib.load()
    for name in ('vmp_hmm_fused_cat_limits', 'vmp_hmm_fused_cat_plan',
                 'vmp_hmm_fused_pass_categorical'):
        assert name in _lib.header_symbols() and hasattr(lib, name)
    mk, mm = ctypes.c_int32(), ctypes.c_int32()
    assert lib.vmp_hmm_fused_cat_limits(ctypes.byref(mk), ctypes.byref(mm)) == _lib.VMP_OK
    assert (mk.value, mm.value) == (64, 128)
