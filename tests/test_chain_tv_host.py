"""CPU: GaussianMarkovChain with time-varying dynamics A_t / innovation precision nu_t -- the
constructor (accepted plate forms, inferred n, the reference's errors), the paths that decline such
a chain, the arithmetic of csrc/vmp_chain_tv.hip built with g++ (tests/host/chain_tv_host.cpp)
against a long-double sum, and the generic engine through the NumPy double of the entry points
against the live-reference fixtures (tests/golden/chain_tv.npz)."""
import os
import warnings

import numpy as np
import pytest

import chain_tv_host
from chain_tv_models import TAGS, run_chain_tv_case

U = 2.0 ** -53


def _chain(N_, A, nu, D=3, **kw):
    return N_.GaussianMarkovChain(np.zeros(D), np.identity(D), A, nu, **kw)


# -- the constructor -----------------------------------------------------------------------------
def test_accepted_plate_forms_and_inferred_n():
    import bayespy_amd.nodes as N_
    D, N = 3, 7
    al = N_.Gamma(1e-5, 1e-5, plates=(D,))
    # nodes with an N-1 plate; n inferred
    A = N_.GaussianARD(0, al, shape=(D,), plates=(N - 1, D))
    nu = N_.Gamma(1e-3, 1e-3, plates=(N - 1, D))
    X = _chain(N_, A, nu)
    assert (X.N, X.D, X.plates, X.time_varying) == (N, D, (), True)
    assert X.dims == ((N, D), (N, D, D), (N - 1, D, D))
    # constants with an N-1 plate, n given and matching, sequence plates from `plates`
    X = _chain(N_, np.ones((N - 1, D, D)), np.ones((N - 1, D)), n=N, plates=(5,))
    assert (X.N, X.plates, X.time_varying) == (N, (5,), True)
    # only one of the two varies; the other has a unit time plate or none
    for A_, nu_ in ((A, np.ones(D)), (A, N_.Gamma(1e-3, 1e-3, plates=(1, D))),
                    (np.ones((D, D)), nu), (N_.GaussianARD(0, al, shape=(D,), plates=(1, D)), nu)):
        X = _chain(N_, A_, nu_)
        assert (X.N, X.time_varying) == (N, True)
    # the dynamics carry a sequence plate before the time plate: it becomes a plate of the chain
    A6 = N_.GaussianARD(0, al, shape=(D,), plates=(6, N - 1, D))
    X = _chain(N_, A6, nu)
    assert (X.N, X.plates) == (N, (6,))
    # constant dynamics are what they were
    X = _chain(N_, np.ones((D, D)), np.ones(D), n=4)
    assert (X.N, X.time_varying) == (4, False)
    X = _chain(N_, np.ones((1, D, D)), np.ones((1, D)), n=2)
    assert (X.N, X.time_varying) == (2, False)


def test_wrong_time_plates_raise_the_references_errors():
    import bayespy_amd.nodes as N_
    D, N = 3, 7
    A = np.ones((N - 1, D, D))
    with pytest.raises(Exception, match='must match the number of last plates of parents: 5 != 6'):
        _chain(N_, A, np.ones(D), n=5)
    with pytest.raises(Exception, match='must match the number of last plates of parents'):
        _chain(N_, np.ones((D, D)), N_.Gamma(1e-3, 1e-3, plates=(N - 1, D)), n=N + 2)
    with pytest.raises(Exception, match='different number of time instances'):
        _chain(N_, A, np.ones((N, D)))
    with pytest.raises(Exception, match='could not be determined automatically'):
        _chain(N_, np.ones((1, D, D)), np.ones((1, D)))
    with pytest.raises(Exception, match='last plate equal to the dimensionality'):
        _chain(N_, A, np.ones((N - 1, D + 1)))
    with pytest.raises(NotImplementedError, match='input signals'):
        _chain(N_, A, np.ones(D), inputs=np.ones((N - 1, 2)))


def test_switching_and_varying_chains_keep_their_errors():
    import bayespy_amd.nodes as N_
    D, K, N = 2, 3, 6
    B = N_.GaussianARD(0, 1, shape=(D,), plates=(K, D))
    Z = N_.Categorical(np.ones(K) / K, plates=(N - 1,))
    with pytest.raises(NotImplementedError, match='time-dependent innovation precision is not built'):
        N_.SwitchingGaussianMarkovChain(np.zeros(D), np.identity(D), B, Z, np.ones((N - 1, D)), n=N)
    Bv = N_.GaussianARD(0, 1, shape=(D, K), plates=(D,))
    S = N_.GaussianARD(0, 1, shape=(K,), plates=(N - 1,))
    with pytest.raises(NotImplementedError, match='time-dependent innovation precision is not built'):
        N_.VaryingGaussianMarkovChain(np.zeros(D), np.identity(D), Bv, S, np.ones((N - 1, D)), n=N)


# -- paths that decline ----------------------------------------------------------------------------
def _lssm(N_, time_plate, B=None):
    D, T, M = 2, 6, 3
    pl = () if B is None else (B,)
    Apl = (T - 1, D) if time_plate else (D,)
    A = N_.GaussianARD(0, N_.Gamma(1e-5, 1e-5, plates=(D,), name='alpha'), shape=(D,), plates=Apl,
                       name='A')
    X = N_.GaussianMarkovChain(np.zeros(D), np.identity(D), A, np.ones(D), n=T, plates=pl, name='X')
    C = N_.GaussianARD(0, N_.Gamma(1e-5, 1e-5, plates=(D,), name='gamma'), shape=(D,),
                       plates=(M,) + (1,) * (len(pl) + 1), name='C')
    F = N_.SumMultiply('i,i', C, X, name='F')
    tau = N_.Gamma(1e-5, 1e-5, name='tau')
    Y = N_.GaussianARD(F, tau, name='Y')
    return dict(Y=Y, F=F, C=C, X=X, A=A, tau=tau, shape=(M,) + pl + (T,))


def test_fused_state_space_matchers_decline_a_time_plate_and_say_so():
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference.plans.lssm import LSSMPlan
    from bayespy_amd.inference.plans.lssm_masked import MaskedLSSMPlan
    r = _lssm(N_, True)
    r['Y'].observe(np.zeros(r['shape']))
    nodes = [r['Y'], r['F'], r['C'], r['C'].parents[1], r['X'], r['A'], r['A'].parents[1], r['tau']]
    for plan in (LSSMPlan, MaskedLSSMPlan):
        why = []
        assert plan.match(nodes, why) is None
        assert any('time plate' in w and 'dynamics A' in w for w in why), why
    # the same model without the time plate is still taken
    r = _lssm(N_, False)
    r['Y'].observe(np.zeros(r['shape']))
    nodes = [r['Y'], r['F'], r['C'], r['C'].parents[1], r['X'], r['A'], r['A'].parents[1], r['tau']]
    why = []
    LSSMPlan.match(nodes, why)
    assert not any('time plate' in w for w in why)


def test_rotation_of_a_time_varying_chain_is_refused():
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference.transformations import RotateGaussianARD, RotateGaussianMarkovChain
    r = _lssm(N_, True)
    with pytest.raises(NotImplementedError, match='time plate'):
        RotateGaussianMarkovChain(r['X'], RotateGaussianARD(r['A'], r['A'].parents[1]))


def test_sharded_models_with_a_time_varying_chain_are_refused():
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference.plans.generic import GenericPlan
    chain_tv_host.install()
    try:
        r = _lssm(N_, True, B=4)
        r['X'].shard(0)
        with pytest.raises(NotImplementedError, match='time-varying dynamics .* sharded'):
            GenericPlan([r['X'], r['A'], r['A'].parents[1]])
    finally:
        from host_generic import uninstall
        uninstall()


# -- the library interface ---------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    from bayespy_amd import _lib
    for s in ('vmp_chain_pair_stats', 'vmp_chain_pair_stats_limits'):
        assert s in _lib.header_symbols() and s in _lib.SIGNATURES


# -- the kernel's arithmetic on the host ---------------------------------------------------------------
@pytest.mark.parametrize('ny,N,D', [(0, 3, 2), (1, 2, 1), (5, 3, 3), (1000, 64, 4), (1000, 2, 16),
                                    (65537, 3, 2), (3000, 1001, 1), (300, 70, 7), (40, 17, 16)])
@pytest.mark.parametrize('scale', [1.0, 1e150, 1e-150])
def test_host_build_of_the_kernel_arithmetic(ny, N, D, scale):
    """Per element: |S - S_longdouble| <= (ny + 2) u sum_b |x_i x_j| -- the bound of recursive
    summation, which covers any fixed order (slices, then their partials)."""
    rs = np.random.RandomState(ny + 7 * N + D)
    x = scale * rs.normal(size=(ny, N, D)) * np.exp(rs.normal(size=(ny, 1, 1)))
    Sxx, Sxp = chain_tv_host.host_pair_stats(x)
    rxx, rxp, axx, axp = chain_tv_host.reference_pair_stats(x)
    assert Sxx.shape == (N, D, D) and Sxp.shape == (N - 1, D, D)
    assert np.all(np.abs(Sxx - rxx) <= (ny + 2) * U * axx)
    assert np.all(np.abs(Sxp - rxp) <= (ny + 2) * U * axp)
    if ny == 0:
        assert not Sxx.any() and not Sxp.any()
    again = chain_tv_host.host_pair_stats(x)
    assert np.array_equal(again[0], Sxx) and np.array_equal(again[1], Sxp)


def test_slices_fill_the_grid_and_the_workspace_covers_them():
    lib = chain_tv_host.chain_tv_host()
    assert lib.chain_tv_max_d() >= 16
    for ny, N, D in ((0, 2, 1), (1, 2, 16), (100000, 1000, 4), (100000, 2, 4), (65537, 1001, 16),
                     (7, 64, 3)):
        ns = lib.chain_tv_nslice(ny, N, D)
        TT = 256 // D
        ntile = (N + TT - 1) // TT
        assert 1 <= ns <= 1024
        assert lib.chain_tv_work_doubles(ny, N, D) == ns * (2 * N - 1) * D * D
        if ny >= 8 * 1024:
            assert ns * ntile >= 512, (ny, N, D, ns, ntile)     # two workgroups per CU at least


# -- the generic engine on the host against the live-reference fixtures -------------------------------
@pytest.mark.parametrize('on', [True, False])
@pytest.mark.parametrize('tag', TAGS)
def test_models_through_the_host_double_match_reference(golden_dir, tag, on):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    f = np.load(os.path.join(golden_dir, 'chain_tv.npz'))
    g = {k[3:]: f[k] for k in f.files if k.startswith('in_')}
    rt = chain_tv_host.install(enabled=on)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res = run_chain_tv_case(N_, VB, g, tag, engine='generic')
    finally:
        from host_generic import uninstall
        uninstall()
    # the plate sums come from the kernel's entry point exactly where the family says they do
    fast = on and tag in ('b2', 'b4', 'b12', 'cA', 'cnu')
    assert bool(rt.lib.calls.get('vmp_chain_pair_stats', 0)) == fast
    np.testing.assert_allclose(res[tag + '_L'], f[tag + '_L'], rtol=1e-9)
    for k, v in res.items():
        if k.endswith('_L'):
            np.testing.assert_allclose(v, f[k], rtol=1e-8, atol=1e-7, err_msg=k)
        else:
            np.testing.assert_allclose(np.broadcast_to(v, f[k].shape), f[k], rtol=1e-7, atol=1e-9,
                                       err_msg=k)


def test_a_state_above_the_kernel_limit_takes_the_general_operations(monkeypatch):
    """D = limit + 1 with the key on: no call of the entry point, and the bits of the key-off run."""
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    import chain_tv_models as m
    from chain_tv_models import build_chain_tv
    D, B, N, M = chain_tv_host.chain_tv_host().chain_tv_max_d() + 1, 5, 6, 20
    rs = np.random.RandomState(3)
    g = {'w_y': rs.normal(size=(M, B, N)), 'w_x0': rs.normal(size=(B, N, D)),
         'w_c0': rs.normal(size=(M, 1, 1, D))}
    monkeypatch.setattr(m, 'CASES', (('w', B, D, N, M),))
    out = []
    for on in (True, False):
        rt = chain_tv_host.install(enabled=on)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                Q, track = build_chain_tv(N_, VB, g, 'w', engine='generic')
                Q.update(repeat=3, verbose=False)
                out.append([Q.L[:3].copy()] + [np.array(u) for nd in track.values() for u in nd.u])
            X = Q['X']
            assert X._plan.family[id(X)].pair_stats_calls == 0
        finally:
            from host_generic import uninstall
            uninstall()
        assert not rt.lib.calls.get('vmp_chain_pair_stats', 0)
    assert np.all(np.isfinite(out[0][0]))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
