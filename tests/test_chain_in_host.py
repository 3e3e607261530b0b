"""CPU: GaussianMarkovChain with input signals -- the constructor (accepted forms, inferred n, the
reference's errors), the paths that decline such a chain, the arithmetic of csrc/vmp_chain_in.hip
built with g++ (tests/host/chain_in_host.cpp) against long-double sums, and the generic engine
through the NumPy double of the entry points against the live-reference fixtures
(tests/golden/chain_in.npz) with the tolerances of test_chain_tv_gpu.py::test_models_match_reference."""
import os
import warnings

import numpy as np
import pytest

import chain_in_host
from chain_in_models import CLOSED_FORM, TAGS, run_chain_in_case

FAST = ('b', 'c', 'd', 'e', 'g')      # shared [A | B] and nu, several sequences, D, K <= limits


def _chain(N_, A, nu, D=3, **kw):
    return N_.GaussianMarkovChain(np.zeros(D), np.identity(D), A, nu, **kw)


# -- the constructor -----------------------------------------------------------------------------
def test_accepted_forms_and_inferred_n():
    import bayespy_amd.nodes as N_
    D, K, N = 3, 2, 7
    al = N_.Gamma(1e-5, 1e-5, plates=(D + K,))
    A = N_.GaussianARD(0, al, shape=(D + K,), plates=(D,))
    # a constant array with an N-1 plate: n inferred, the inputs are the fifth parent
    X = _chain(N_, A, np.ones(D), inputs=np.ones((N - 1, K)))
    assert (X.N, X.D, X.K_inputs, X.plates, X.time_varying) == (N, D, K, (), False)
    assert len(X.parents) == 5
    assert X.dims == ((N, D), (N, D, D), (N - 1, D, D))
    # a node, with sequence plates; n given and matching
    U = N_.GaussianARD(0, 1, shape=(K,), plates=(4, N - 1))
    X = _chain(N_, A, np.ones(D), n=N, inputs=U, plates=(4,))
    assert (X.N, X.plates, X.parents[4]) == (N, (4,), U)
    # a unit time plate on the inputs, n from the time plate of [A | B]
    At = N_.GaussianARD(0, al, shape=(D + K,), plates=(N - 1, D))
    X = _chain(N_, At, np.ones(D), inputs=np.ones((1, K)))
    assert (X.N, X.time_varying) == (N, True)
    # constant [A | B] of shape (D, D + K)
    X = _chain(N_, np.ones((D, D + K)), np.ones(D), n=N, inputs=np.ones((N - 1, K)))
    assert (X.N, X.K_inputs) == (N, K)
    # no inputs: four parents, as before
    X = _chain(N_, np.ones((D, D)), np.ones(D), n=4)
    assert (len(X.parents), X.K_inputs) == (4, 0)


def test_wrong_plates_raise_the_references_errors():
    import bayespy_amd.nodes as N_
    D, K, N = 3, 2, 7
    AB = np.ones((D, D + K))
    with pytest.raises(Exception, match='Dynamics matrix has wrong dimensionality'):
        _chain(N_, np.ones((D, D)), np.ones(D), inputs=np.ones((N - 1, K)))
    with pytest.raises(Exception, match='Dynamics matrix has wrong dimensionality'):
        _chain(N_, N_.GaussianARD(0, 1, shape=(D,), plates=(D,)), np.ones(D),
               inputs=np.ones((N - 1, K)))
    # any other row length is the reference's plain error; the D-column matrix above (inputs
    # without their gain B) is refused as not built, with the reference's text first
    with pytest.raises(Exception, match='Dynamics matrix has wrong dimensionality') as e:
        _chain(N_, np.ones((D, D + K + 1)), np.ones(D), inputs=np.ones((N - 1, K)))
    assert type(e.value) is Exception
    with pytest.raises(NotImplementedError, match='wrong dimensionality: input signals .* gain'):
        _chain(N_, np.ones((D, D)), np.ones(D), inputs=np.ones((N - 1, K)))
    with pytest.raises(Exception, match='different number of time instances'):
        _chain(N_, np.ones((N - 1, D, D + K)), np.ones(D), inputs=np.ones((N, K)))
    with pytest.raises(Exception, match='must match the number of last plates of parents: 5 != 6'):
        _chain(N_, AB, np.ones(D), n=5, inputs=np.ones((N - 1, K)))
    with pytest.raises(Exception, match='could not be determined automatically'):
        _chain(N_, AB, np.ones(D), inputs=np.ones((1, K)))
    with pytest.raises(ValueError, match='Input signals have wrong dimensionality'):
        _chain(N_, AB, np.ones(D), n=N, inputs=N_.Gamma(1, 1, plates=(N - 1,)))
    with pytest.raises(ValueError, match='do not broadcast'):
        _chain(N_, AB, np.ones(D), n=N, inputs=np.ones((4, N - 1, K)), plates=(5,))


def test_family_of_the_fifth_parent():
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference.plans.families import make_family
    chain_in_host.install()
    try:
        D, K, N = 3, 2, 7
        X = _chain(N_, np.ones((D, D + K)), np.ones(D), n=N, inputs=np.ones((4, N - 1, K)),
                   plates=(4,))
        fam = make_family(X)
        assert fam.Kin == K
        assert fam.plates_to_parent(4) == (4, N - 1)
        assert fam.plates_to_parent(2) == (4, N - 1, D)
        assert fam.mask_to_parent(4, np.ones((4,), bool)).shape == (4, 1)
        z, zz = fam.constant_moments(4, np.arange(2.0 * K).reshape(2, K))
        assert np.array_equal(np.array(zz), np.einsum('ti,tj->tij', np.array(z), np.array(z)))
    finally:
        from host_generic import uninstall
        uninstall()


def test_a_chain_without_inputs_builds_the_family_state_it_did():
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference.plans.families import make_family
    chain_in_host.install()
    try:
        X = _chain(N_, np.ones((3, 3)), np.ones(3), n=5, plates=(2,))
        fam = make_family(X)
        assert (fam.Kin, fam.time_varying, fam.input_stats_calls, fam.pair_stats_calls) \
            == (0, False, 0, 0)
        assert fam._solve is None and fam._pair is None and fam._in is None
        assert [fam.plates_to_parent(i) for i in range(4)] == [(2,), (2,), (2, 4, 3), (2, 4, 3)]
        up = [fam.constant_moments(i, p.value) for i, p in enumerate(X.parents)]
        Am, AA, nu, _ = fam._dyn(up)
        assert (Am.shape, AA.shape, nu.shape) == ((1, 3, 3), (1, 3, 3, 3), (1, 3))
        phi = fam.phi_from_parents(up)
        assert [tuple(p.shape) for p in phi] == [(5, 3), (5, 3, 3), (1, 3, 3)]
        u, g = fam.moments_and_cgf(phi)
        assert fam._solve is None          # kept for the plate sums of the other chains only
    finally:
        from host_generic import uninstall
        uninstall()


# -- paths that decline ----------------------------------------------------------------------------
def _lssm(N_, inputs, B=None):
    D, K, T, M = 2, 2, 6, 3
    pl = () if B is None else (B,)
    R = D + (K if inputs else 0)
    A = N_.GaussianARD(0, N_.Gamma(1e-5, 1e-5, plates=(R,), name='alpha'), shape=(R,), plates=(D,),
                       name='A')
    X = N_.GaussianMarkovChain(np.zeros(D), np.identity(D), A, np.ones(D), n=T, plates=pl, name='X',
                               inputs=np.ones((T - 1, K)) if inputs else None)
    C = N_.GaussianARD(0, N_.Gamma(1e-5, 1e-5, plates=(D,), name='gamma'), shape=(D,),
                       plates=(M,) + (1,) * (len(pl) + 1), name='C')
    F = N_.SumMultiply('i,i', C, X, name='F')
    tau = N_.Gamma(1e-5, 1e-5, name='tau')
    Y = N_.GaussianARD(F, tau, name='Y')
    return dict(Y=Y, F=F, C=C, X=X, A=A, tau=tau, shape=(M,) + pl + (T,))


def _nodes(r):
    return [r['Y'], r['F'], r['C'], r['C'].parents[1], r['X'], r['A'], r['A'].parents[1], r['tau']]


def test_fused_state_space_matchers_decline_inputs_and_say_so():
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference.plans.lssm import LSSMPlan
    from bayespy_amd.inference.plans.lssm_masked import MaskedLSSMPlan
    r = _lssm(N_, True)
    r['Y'].observe(np.zeros(r['shape']))
    for plan in (LSSMPlan, MaskedLSSMPlan):
        why = []
        assert plan.match(_nodes(r), why) is None
        hits = [w for w in why if 'input signals go through the generic engine' in w]
        assert hits and all(w.startswith(plan._label) for w in hits), why
    # the same model without inputs is still taken
    r = _lssm(N_, False)
    r['Y'].observe(np.zeros(r['shape']))
    why = []
    LSSMPlan.match(_nodes(r), why)
    assert not any('input signals' in w for w in why)


def test_the_fused_engine_raises_that_reason():
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    chain_in_host.install()
    try:
        r = _lssm(N_, True)
        r['Y'].observe(np.zeros(r['shape']))
        with pytest.raises(Exception, match='input signals go through the generic engine'):
            Q = VB(*_nodes(r), engine='fused')
            Q.update(repeat=1, verbose=False)
    finally:
        from host_generic import uninstall
        uninstall()


def test_rotation_of_a_chain_with_inputs_is_refused_by_name():
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference.transformations import RotateGaussianARD, RotateGaussianMarkovChain
    r = _lssm(N_, True)
    with pytest.raises(NotImplementedError, match='chain X has input signals'):
        RotateGaussianMarkovChain(r['X'], RotateGaussianARD(r['A'], r['A'].parents[1]))


def test_sharded_models_with_inputs_are_refused():
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference.plans.generic import GenericPlan
    chain_in_host.install()
    try:
        r = _lssm(N_, True, B=4)
        r['X'].shard(0)
        with pytest.raises(NotImplementedError, match='input signals .* sharded'):
            GenericPlan([r['X'], r['A'], r['A'].parents[1]])
    finally:
        from host_generic import uninstall
        uninstall()


# -- the library interface ---------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    from bayespy_amd import _lib
    for s in ('vmp_chain_input_stats', 'vmp_chain_input_stats_limits'):
        assert s in _lib.header_symbols() and s in _lib.SIGNATURES


# -- the kernel's arithmetic on the host ---------------------------------------------------------------
@pytest.mark.parametrize('ny,N,D,K', [(0, 3, 2, 2), (1, 2, 1, 1), (5, 3, 3, 2), (9, 17, 7, 5),
                                      (1000, 17, 1, 16), (1000, 2, 16, 1), (1000, 33, 16, 16),
                                      (65537, 3, 2, 3), (300, 300, 1, 1)])
@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('scale', [1.0, 1e150, 1e-150])
def test_host_build_of_the_kernel_arithmetic(ny, N, D, K, shared, scale):
    """Per element: |S - S_longdouble| <= (ny + 2) u sum_b |terms| -- the bound of recursive
    summation, which covers any fixed order (slices, then their partials)."""
    x, z = chain_in_host.make_xz(ny, 1 if shared else ny, N, D, K, scale)
    S = chain_in_host.host_input_stats(x, z)
    chain_in_host.check_against_long_double(S, x, z)
    again = chain_in_host.host_input_stats(x, z, with_zz=False)
    assert again[2] is None
    assert np.array_equal(again[0], S[0]) and np.array_equal(again[1], S[1])


def test_slices_fill_the_grid_and_the_workspace_covers_them():
    lib = chain_in_host.chain_in_host()
    assert lib.chain_in_max_d() == 16 and lib.chain_in_max_k() == 16
    for ny, N, D, K in ((0, 2, 1, 1), (1, 2, 16, 16), (100000, 1000, 4, 2), (100000, 2, 4, 4),
                        (65537, 1001, 16, 3), (7, 64, 3, 9)):
        ns = lib.chain_in_nslice(ny, N, D, K)
        TT = 256 // max(D, K)
        assert lib.chain_in_tile(D, K) == TT
        ntile = (N - 1 + TT - 1) // TT
        assert 1 <= ns <= 1024
        assert lib.chain_in_work_doubles(ny, N, D, K) == ns * (N - 1) * (2 * D * K + K * K)
        if ny >= 8 * 1024:
            assert ns * ntile >= 512, (ny, N, D, K, ns, ntile)   # two workgroups per CU at least


# -- the generic engine on the host against the live-reference fixtures -------------------------------
def _golden(golden_dir):
    f = np.load(os.path.join(golden_dir, 'chain_in.npz'))
    return f, {k[3:]: f[k] for k in f.files if k.startswith('in_')}


def _joint_gaussian(mu, Lam, AB, nu, u):
    """Mean and covariance of all N D state elements of one driven chain, from the model's own
    definition: log p = -1/2 (x_0 - mu)^T Lam (x_0 - mu)
    - 1/2 sum_t (x_{t+1} - A x_t - B u_t)^T diag(nu) (x_{t+1} - A x_t - B u_t) + const, collected
    into a precision matrix P and a linear term h, transition by transition."""
    D = len(mu)
    T = len(u)
    A, B, W = AB[:, :D], AB[:, D:], np.diag(nu)
    P, h = np.zeros(((T + 1) * D,) * 2), np.zeros((T + 1) * D)
    P[:D, :D] += Lam
    h[:D] += Lam @ mu
    for t in range(T):
        prev, nxt = slice(t * D, (t + 1) * D), slice((t + 1) * D, (t + 2) * D)
        drive = B @ u[t]
        P[nxt, nxt] += W
        P[prev, prev] += A.T @ W @ A
        P[prev, nxt] -= A.T @ W
        P[nxt, prev] -= W @ A
        h[nxt] += W @ drive
        h[prev] -= A.T @ W @ drive
    S = np.linalg.inv(P)
    return S @ h, S


@pytest.mark.parametrize('case', ['reference', 'wide'])
def test_a_chain_without_children_is_the_joint_gaussian_of_its_definition(golden_dir, case):
    """One driven chain with constant parents and no children: its moments are those of the joint
    Gaussian the model defines.  'reference': the parameters of the reference's own case (D = K = 1,
    N = 3), also against the moments the reference recorded for it (cf_u0..2 of the fixture);
    'wide': D = 2, K = 3, N = 5."""
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    if case == 'reference':
        c = CLOSED_FORM
        mu, Lam = np.array([c['mu']]), np.array([[c['Lambda']]])
        AB, nu, u = np.array([[c['A'], c['B']]]), np.array([c['v']]), np.array(c['inputs'])
    else:
        rs = np.random.RandomState(11)
        D, K, T = 2, 3, 4
        mu, Lam = rs.normal(size=D), np.array([[2.0, 0.3], [0.3, 1.0]])
        AB = np.concatenate([0.6 * rs.normal(size=(D, D)), rs.normal(size=(D, K))], axis=-1)
        nu, u = np.array([1.5, 0.7]), rs.normal(size=(T, K))
    D = len(mu)
    mean, S = _joint_gaussian(mu, Lam, AB, nu, u)
    chain_in_host.install()
    try:
        X = N_.GaussianMarkovChain(mu, Lam, AB, nu, inputs=u)
        Q = VB(X, engine='generic')
        Q.update(X, repeat=1, verbose=False)
        got = [np.array(a) for a in X.u]
    finally:
        from host_generic import uninstall
        uninstall()
    N = len(u) + 1
    second = S + np.outer(mean, mean)
    want = [mean.reshape(N, D),
            np.array([second[t * D:(t + 1) * D, t * D:(t + 1) * D] for t in range(N)]),
            np.array([second[t * D:(t + 1) * D, (t + 1) * D:(t + 2) * D] for t in range(N - 1)])]
    for g_, w_ in zip(got, want):
        np.testing.assert_allclose(g_, w_, rtol=1e-9, atol=1e-12)
    if case == 'reference':
        f, _ = _golden(golden_dir)
        for i in range(3):
            np.testing.assert_allclose(got[i], f['cf_u%d' % i], rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize('on', [True, False])
@pytest.mark.parametrize('tag', TAGS)
def test_models_through_the_host_double_match_reference(golden_dir, tag, on):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    f, g = _golden(golden_dir)
    rt = chain_in_host.install(enabled=on)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res = run_chain_in_case(N_, VB, g, tag, engine='generic')
    finally:
        from host_generic import uninstall
        uninstall()
    # the plate sums come from the kernel's entry point exactly where the family says they do
    fast = on and tag in FAST
    assert bool(rt.lib.calls.get('vmp_chain_input_stats', 0)) == fast
    np.testing.assert_allclose(res[tag + '_L'], f[tag + '_L'], rtol=1e-9)
    for k, v in res.items():
        if k.endswith('_L'):
            np.testing.assert_allclose(v, f[k], rtol=1e-8, atol=1e-7, err_msg=k)
        else:
            np.testing.assert_allclose(np.broadcast_to(v, f[k].shape), f[k], rtol=1e-7, atol=1e-9,
                                       err_msg=k)


@pytest.mark.parametrize('D,K', [(17, 2), (2, 17)])
def test_dimensions_above_the_kernel_limits_take_the_general_operations(monkeypatch, D, K):
    """D or K = limit + 1 with the key on: no call of the entry point, and the bits of the key-off
    run."""
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    import chain_in_models as m
    B, N, M = 5, 5, 20
    rs = np.random.RandomState(3)
    g = {'b_y': rs.normal(size=(M, B, N)), 'b_x0': rs.normal(size=(B, N, D)),
         'b_c0': rs.normal(size=(M, 1, 1, D)), 'b_u': rs.normal(size=(B, N - 1, K))}
    monkeypatch.setattr(m, 'CASES', (('b', B, D, K, N, M),))
    out = []
    for on in (True, False):
        rt = chain_in_host.install(enabled=on)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                Q, track = m.build_chain_in(N_, VB, g, 'b', engine='generic')
                Q.update(repeat=3, verbose=False)
                out.append([Q.L[:3].copy()] + [np.array(u) for nd in track.values() for u in nd.u])
            X = Q['X']
            assert X._plan.family[id(X)].input_stats_calls == 0
        finally:
            from host_generic import uninstall
            uninstall()
        assert not rt.lib.calls.get('vmp_chain_input_stats', 0)
    assert np.all(np.isfinite(out[0][0]))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
