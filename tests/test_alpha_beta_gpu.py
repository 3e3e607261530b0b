"""GPU: ``vmp_alpha_beta_recursion`` (csrc/vmp_hmm.hip, ``alpha_beta_kernel<KP>``) through the raw
C ABI on plain device buffers against the long-double restatement of the reference
(tests/alpha_beta_host.py ``restate``) under the rule of DESIGN 4.14 / 4.15: every instance
KP = 2 ... 64 at its edges, the register / LDS boundary K = 16 | 17, every stride form of the
ABI, the grid-stride loop with idle groups, impossible states, tables and emissions far outside
the range of ``exp``, determinism, the argument checks, and one model through engine='generic'.

Every output buffer (and the workspace) carries a tail of 64 sentinel doubles that must survive
the call: a store of an idle group or of a padded lane lands there.

Measured on MI355X (float64 deviation of the reference formulas, error of the kernel,
allowance): see DESIGN.md section 4.16."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

pytestmark = pytest.mark.gpu

TAIL = 64
SENTINEL = -7.25e77


def _kp(K):
    KP = 2
    while KP < K:
        KP *= 2
    return KP


def _groups(K):
    return 64 // _kp(K)


def _up(a):
    import torch
    from bayespy_amd.device import get_runtime
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(get_runtime().device)


def call(p0, p0_bs, P, P_bs, P_ts, B, N, K, ws_bytes=None, expect=0):
    """One call on device copies of ``p0`` / ``P`` (any shape; only the strides describe them);
    the status code and z0, zz, g as NumPy arrays.  Asserts the sentinel tails."""
    import torch
    from bayespy_amd.device import get_runtime, ptr
    rt = get_runtime()
    rt.sync_stream()
    sizes = dict(z0=B * K, zz=B * N * K * K, g=B, ws=B * N * K)
    buf = {k: torch.full((n + TAIL,), SENTINEL, dtype=torch.float64, device=rt.device)
           for k, n in sizes.items()}
    p0d, Pd = _up(p0), _up(P)
    rc = rt.lib.vmp_alpha_beta_recursion(
        rt.ctx, N, K, B, ptr(p0d), p0_bs, ptr(Pd), P_bs, P_ts, ptr(buf['z0']), ptr(buf['zz']),
        ptr(buf['g']), ptr(buf['ws']), sizes['ws'] * 8 if ws_bytes is None else ws_bytes)
    assert rc == expect, (rc, rt.lib.vmp_last_error(rt.ctx))
    for k, n in sizes.items():
        assert bool(torch.all(buf[k][n:] == SENTINEL)), 'the tail of %s was written' % k
    if rc != 0 or B == 0:
        for k, n in sizes.items():
            assert bool(torch.all(buf[k] == SENTINEL)), '%s was written' % k
        return None
    return dict(z0=buf['z0'][:B * K].cpu().numpy().reshape(B, K),
                zz=buf['zz'][:B * N * K * K].cpu().numpy().reshape(B, N, K, K),
                g=buf['g'][:B].cpu().numpy())


def dense(logp0, logP):
    B, N, K = logP.shape[0], logP.shape[1], logP.shape[-1]
    return call(logp0, K, logP, N * K * K, K * K, B, N, K)


def properties(got):
    """Size-independent: every pairwise marginal sums to one to 1e-13; z0 is the row sums of
    zz_0 (the kernel divides them by their total, which is that same sum in another order, so
    the two differ by no more than the total differs from one)."""
    np.testing.assert_allclose(got['zz'].sum(axis=(-1, -2)), 1.0, rtol=0, atol=1e-13)
    np.testing.assert_allclose(got['z0'], got['zz'][:, 0].sum(axis=-1), rtol=0, atol=1e-13)


@pytest.mark.parametrize('K', [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64])
def test_every_instance_at_its_edges(K):
    from alpha_beta_host import compare, inputs
    G = _groups(K)
    bad = []
    for N in (1, 2, 7):
        for B in (1, G + 1, 2 * G + 1):
            logp0, logP = inputs('random', B, N, K, seed=100 * N + B)
            got = dense(logp0, logP)
            bad += compare(got, logp0, logP, label=str((K, N, B)))
            properties(got)
    assert bad == []


@pytest.mark.parametrize('K', [5, 33])
@pytest.mark.parametrize('p0_shared', [False, True])
@pytest.mark.parametrize('form', ['dense', 'shared_b', 'shared_bt', 'shared_t'])
def test_stride_forms(form, p0_shared, K):
    """(P_bstride, P_tstride) = (N K^2, K^2), (0, K^2), (0, 0) and (K^2, 0): the last, one slice
    per chain shared over time, is legal in the ABI and never produced by the wrapper."""
    from alpha_beta_host import compare, inputs
    N, B = 4, 2 * _groups(K) + 1
    logp0, logP = inputs('random', B, N, K, seed=7)
    p0 = logp0[:1] if p0_shared else logp0
    P, P_bs, P_ts = {'dense': (logP, N * K * K, K * K), 'shared_b': (logP[:1], 0, K * K),
                     'shared_bt': (logP[:1, :1], 0, 0), 'shared_t': (logP[:, :1], K * K, 0)}[form]
    got = call(p0, 0 if p0_shared else K, P, P_bs, P_ts, B, N, K)
    assert compare(got, np.broadcast_to(p0, (B, K)), np.broadcast_to(P, (B, N, K, K)),
                   label='%s K=%d' % (form, K)) == []
    properties(got)


@pytest.mark.parametrize('K,N', [(2, 2), (33, 1)])
def test_grid_stride_loop_with_idle_groups(K, N):
    """num_cu * 32 blocks of G chains, then G + 1 more: block 0 and block 1 run a second round,
    block 1 with all groups but one idle."""
    from alpha_beta_host import compare, inputs
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    G = _groups(K)
    B = int(rt.lib.vmp_ctx_num_cu(rt.ctx)) * 32 * G + G + 1
    logp0, logP = inputs('random', B, N, K, seed=2)
    got = dense(logp0, logP)
    assert compare(got, logp0, logP, label='grid-stride K=%d B=%d' % (K, B)) == []
    properties(got)
    for sl in (slice(0, G + 1), slice(B - G - 1, B)):
        small = dense(logp0[sl], logP[sl])
        for k in small:
            np.testing.assert_array_equal(small[k], got[k][sl], err_msg=k)


@pytest.mark.parametrize('K', [3, 17])
@pytest.mark.parametrize('kind', ['inf_p0', 'inf_col', 'inf_row', 'left_to_right'])
def test_impossible_states(kind, K):
    from alpha_beta_host import compare, inputs, restate
    B, N = 2 * _groups(K) + 1, 4
    logp0, logP = inputs(kind, B, N, K, seed=3)
    z0, zz, g = restate(logp0, logP)
    assert np.all(np.isfinite(g)) and np.any(zz == 0)      # every chain keeps a possible path
    got = dense(logp0, logP)
    for k in got:
        assert np.all(np.isfinite(got[k])), k
    assert np.all(got['zz'][zz == 0] == 0) and np.all(got['z0'][z0 == 0] == 0)
    assert compare(got, logp0, logP, label='%s K=%d' % (kind, K)) == []
    properties(got)


def test_sparse_table_case():
    """Chain 0 is the counter-example of a shift by the joint maximum of a slice (tests/
    alpha_beta_host.py SPARSE: g = 803.18 and zz_1 on (1, 2); with a joint shift g = 903.75 and
    zz_1 on (0, 1)); the other 16 chains relabel its states."""
    from alpha_beta_host import SPARSE_G, compare, inputs
    from test_alpha_beta_host import SHAPES
    logp0, logP = inputs('sparse', *SHAPES['sparse'], seed=3)
    assert SHAPES['sparse'][0] == _groups(3) + 1
    got = dense(logp0, logP)
    print('sparse chain 0: g = %.6f  zz_1[1,2] = %.6f  zz_1[0,1] = %.6f'
          % (got['g'][0], got['zz'][0, 1, 1, 2], got['zz'][0, 1, 0, 1]))
    assert compare(got, logp0, logP, label='sparse') == []
    assert abs(got['g'][0] - SPARSE_G) < 5e-3 and got['zz'][0, 1, 1, 2] > 1 - 1e-9
    properties(got)


def test_tables_below_the_underflow_of_exp():
    """The unlearned Dirichlet(1e-3) table at K = 64: every entry below -900, zz = 1 / K^2."""
    from alpha_beta_host import compare, inputs
    from test_alpha_beta_host import SHAPES
    B, N, K = SHAPES['dirichlet_tiny']
    logp0, logP = inputs('dirichlet_tiny', B, N, K)
    assert logP.max() < -900
    got = dense(logp0, logP)
    assert compare(got, logp0, logP, label='dirichlet_tiny') == []
    np.testing.assert_allclose(got['zz'], 1.0 / K ** 2, rtol=1e-12)
    np.testing.assert_allclose(got['z0'], 1.0 / K, rtol=1e-12)


def test_one_used_row():
    """Row 0 near 0, the others in (-745, -600), partly below the normal range of exp(x); the
    odd chains leave their first state through such a row."""
    from alpha_beta_host import compare, inputs
    from test_alpha_beta_host import SHAPES
    logp0, logP = inputs('one_row', *SHAPES['one_row'], seed=3)
    got = dense(logp0, logP)
    assert compare(got, logp0, logP, label='one_row') == []
    assert np.all(np.argmax(got['z0'][1::2], axis=-1) == 1)
    properties(got)


def test_long_chain_of_separated_emissions():
    from alpha_beta_host import compare, inputs
    from test_alpha_beta_host import SHAPES
    logp0, logP = inputs('long', *SHAPES['long'], seed=3)
    got = dense(logp0, logP)
    for k in got:
        assert np.all(np.isfinite(got[k])), k
    assert np.all(np.abs(got['g']) > 5e3)
    assert compare(got, logp0, logP, label='long') == []
    properties(got)


@pytest.mark.parametrize('c', [1e4, -1e4])
def test_constant_added_to_every_slice(c):
    """logP + c: g moves by -N c and zz stays, each within the allowances of the two inputs."""
    from alpha_beta_host import allowances, compare, inputs
    B, N, K = 5, 7, 5
    logp0, logP = inputs('random', B, N, K, seed=3)
    base, moved = dense(logp0, logP), dense(logp0, logP + c)
    assert compare(base, logp0, logP, label='base') == []
    assert compare(moved, logp0, logP + c, label='c = %g' % c) == []
    a0, a1 = allowances(logp0, logP), allowances(logp0, logP + c)
    dg = float(np.max(np.abs((moved['g'] - base['g']) + N * c)))
    dzz = float(np.max(np.abs(moved['zz'] - base['zz'])))
    # the inputs logP + c are themselves rounded to the spacing of |c|: the reference moves by
    # that much too, so its own movement is part of the bound
    ref_g = float(np.max(np.abs((a1['g'][0] - a0['g'][0]) + N * c)))
    ref_zz = float(np.max(np.abs(a1['zz'][0] - a0['zz'][0])))
    print('c = %g: g moved by -N c to %.3e (reference %.3e, allowances %.3e + %.3e); zz moved '
          '%.3e (reference %.3e, allowances %.3e + %.3e)'
          % (c, dg, ref_g, a0['g'][2], a1['g'][2], dzz, ref_zz, a0['zz'][2], a1['zz'][2]))
    assert dg <= ref_g + a0['g'][2] + a1['g'][2]
    assert dzz <= ref_zz + a0['zz'][2] + a1['zz'][2]


def test_determinism_and_arguments():
    from alpha_beta_host import inputs
    from bayespy_amd import _lib
    B, N, K = 9, 5, 17
    logp0, logP = inputs('random', B, N, K, seed=9)
    a, b = dense(logp0, logP), dense(logp0, logP)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    args = (logp0, K, logP, N * K * K, K * K)
    exact = call(*args, B, N, K, ws_bytes=B * N * K * 8)              # exactly enough: accepted
    for k in a:
        np.testing.assert_array_equal(a[k], exact[k], err_msg=k)
    assert call(*args, B, N, K, ws_bytes=B * N * K * 8 - 8, expect=_lib.VMP_ERR_INVALID) is None
    assert call(*args, 0, N, K, expect=_lib.VMP_OK) is None           # nothing is written
    big = np.zeros(65 * 65)
    assert call(big, 65, big, 0, 0, 1, 1, 65, expect=_lib.VMP_ERR_UNSUPPORTED) is None


def test_model_through_the_generic_engine(monkeypatch):
    """A CategoricalMarkovChain under Dirichlet(1e-3) priors gating separated Gaussian means,
    engine='generic': zz of its first update against ``restate`` on the logp0 / logP the node
    formed -- the wrapper's choice of strides is on the path."""
    import bayespy_amd.nodes as N_
    from alpha_beta_host import compare
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.plans import families_extra
    seen = []
    real = families_extra.drandom.alpha_beta_recursion

    def spy(logp0, logP):
        out = real(logp0, logP)
        seen.append((np.array(logp0.numpy()), np.array(logP.numpy()), [np.array(o.numpy()) for o in out]))
        return out
    monkeypatch.setattr(families_extra.drandom, 'alpha_beta_recursion', spy)
    rs = np.random.RandomState(4)
    K, T = 3, 40
    z = np.repeat(rs.randint(K, size=T // 5), 5)
    mu = 4.0 * np.arange(K)[:, None] * np.ones(2)
    y = mu[z] + rs.randn(T, 2)
    a0 = N_.Dirichlet(1e-3 * np.ones(K), name='a0')
    A = N_.Dirichlet(1e-3 * np.ones((K, K)), name='A')
    Z = N_.CategoricalMarkovChain(a0, A, states=T, name='Z')
    Y = N_.Mixture(Z, N_.Gaussian, mu, np.identity(2), name='Y')
    Y.observe(y)
    Q = VB(Y, Z, A, a0, engine='generic')
    Q.update(Z, verbose=False)
    assert len(seen) >= 1                                   # the last call is the update of Z
    logp0, logP, (z0, zz, g) = seen[-1]
    assert logP.shape[-3:] == (T - 1, K, K) and logP.max() < -600
    logp0 = np.broadcast_to(logp0, logP.shape[:-3] + (K,))
    got = dict(z0=z0.reshape(logp0.shape), zz=zz.reshape(logP.shape), g=g.reshape(logP.shape[:-3]))
    assert compare(got, logp0, logP, label='model') == []
    np.testing.assert_array_equal(np.argmax(got['zz'].reshape(-1, T - 1, K * K), axis=-1)[0],
                                  z[:-1] * K + z[1:])
