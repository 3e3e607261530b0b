"""TEST DOUBLE of the mixture block's kernels with the natural-gradient step of stochastic
variational inference: ``fake_kernels.CPUGMMKernels`` plus ``natural_init`` / ``natural_step`` of
``bayespy_amd.inference.plans.gmm.GMMKernels``, in NumPy float64 on the packed state.  Also the
restatement ``natural_step_reference`` that the GPU test of the kernel compares against."""
import numpy as np
from scipy import special

from fake_kernels import CPUGMMKernels

STEP_MU, STEP_LAMBDA, STEP_ALPHA = 1, 2, 4


def natural_step_reference(D, K, nodes, mult, scale, R, S1, S2, mu, Cmu, Lam, nk, Vk, alpha, phi,
                           beta0, n0, V0, alpha0):
    """phi <- phi + scale (phi* - phi) for the nodes of the bit set, every optimum from the
    arguments as given (the moments at entry).  ``phi`` is (K, D + D*D): h_k, then Lambda_mu,k.
    Returns a dict of the new parameters of the stepped nodes."""
    out = {}
    I = np.identity(D)

    def step(old, new):
        return new if scale == 1.0 else old + scale * (new - old)
    if nodes & STEP_MU:
        h_old, P_old = phi[:, :D], phi[:, D:].reshape(K, D, D)
        P = beta0 * I + (mult * R)[:, None, None] * Lam
        h = np.einsum('kij,kj->ki', Lam, mult * S1)
        out['Lmu'], out['h'] = step(P_old, P), step(h_old, h)
    if nodes & STEP_LAMBDA:
        mm = Cmu + mu[:, :, None] * mu[:, None, :]
        sm = (mult * S1)[:, :, None] * mu[:, None, :]
        V = V0 + mult * S2 - sm - np.swapaxes(sm, 1, 2) + (mult * R)[:, None, None] * mm
        out['nk'], out['Vk'] = step(nk, n0 + mult * R), step(Vk, V)
    if nodes & STEP_ALPHA:
        out['alpha'] = step(alpha, alpha0 + mult * R)
    return out


class CPUGMMSVIKernels(CPUGMMKernels):

    def natural_init(self, D, K, state, phi_mu):
        self.calls.append('natural_init')
        v = self._v(state, D, K)
        p = phi_mu.numpy().reshape(K, D + D * D)
        p[:, :D] = 0.0
        p[:, D:] = (v['hdr'][0] * np.identity(D)).reshape(-1)

    def natural_step(self, D, K, nodes, mult, scale, state, phi_mu):
        self.calls.append('natural_step:%d' % nodes)
        v = self._v(state, D, K)
        p = phi_mu.numpy().reshape(K, D + D * D)
        new = natural_step_reference(
            D, K, nodes, float(mult), float(scale), v['R'].copy(), v['S1'].copy(), v['S2'].copy(),
            v['mu'].copy(), v['Cmu'].copy(), v['Lam'].copy(), v['nk'].copy(), v['Vk'].copy(),
            v['alpha'].copy(), p.copy(), v['hdr'][0], v['hdr'][1], v['V0'].copy(),
            v['alpha0'].copy())
        if nodes & STEP_MU:
            p[:, :D], p[:, D:] = new['h'], new['Lmu'].reshape(K, -1)
            v['Cmu'][:] = np.linalg.inv(new['Lmu'])
            v['ldLmu'][:] = np.linalg.slogdet(new['Lmu'])[1]
            v['mu'][:] = np.einsum('kij,kj->ki', v['Cmu'], new['h'])
        if nodes & STEP_LAMBDA:
            v['nk'][:], v['Vk'][:] = new['nk'], new['Vk']
            self._lambda_moments(v, D)
        if nodes & STEP_ALPHA:
            v['alpha'][:] = new['alpha']
            v['logpi'][:] = special.digamma(v['alpha']) - special.digamma(v['alpha'].sum())


def attach(Q):
    """Give the plan of a VB object this double and a CPU runtime."""
    from bayespy_amd.device import Runtime
    rt = Runtime(device='cpu')
    for p in Q.plans:
        assert type(p).__name__ == 'GMMSVIPlan', type(p).__name__
        p._rt, p._kernels = rt, CPUGMMSVIKernels(rt)
    return Q
