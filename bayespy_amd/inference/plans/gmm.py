"""
Execution plan of the full-covariance Gaussian-mixture block

    alpha = Dirichlet(a0); z = Categorical(alpha, plates=(N,));
    mu = GaussianARD(0, beta0, shape=(D,), plates=(K,)); Lambda = Wishart(n0, V0, plates=(K,));
    Y = Mixture(z, Gaussian, mu, Lambda)                     (bayespy/demos/mog.py:17-64)

with a fully observed Y, D <= 32, K <= 64.  The plan owns, in HBM: ``Y`` (N, D), the
responsibilities ``R`` (N, K) (= z.u[0]) and one state block (``vmp_gmm_layout``)
holding the statistics T = r^T [1, y, y y^T] that ranks all-reduce and every
replicated quantity.  The only plate-sized work per VB iteration is ONE pass over
Y, issued by ``z.update()`` (``vmp_gmm_pass``).
"""
import ctypes

import numpy as np

from . import _delta

from ... import _lib
from ...device import get_runtime, ptr
from ...nodes.node import Constant
from ...nodes.gaussian import GaussianARD, Gaussian
from ...nodes.wishart import Wishart
from ...nodes.dirichlet import Dirichlet
from ...nodes.categorical import Categorical
from ...nodes.mixture import Mixture


# the bit set of vmp_gmm_natural_step; one of them selects the node of vmp_gmm_update_annealed
STEP_MU, STEP_LAMBDA, STEP_ALPHA = 1, 2, 4


class GMMKernels:

    def __init__(self, rt):
        self.rt, self.lib, self.ctx = rt, rt.lib, rt.ctx

    def layout(self, D, K):
        L = _lib.GMMLayout()
        rc = self.lib.vmp_gmm_get_layout(D, K, ctypes.byref(L))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'fused GMM block supports D <= 32 and K <= 64')
        return L

    def workspace_doubles(self, D, K):
        n = ctypes.c_size_t()
        self.rt.check(self.lib.vmp_gmm_workspace_bytes(self.ctx, D, K, ctypes.byref(n)))
        return (n.value + 7) // 8

    def init_state(self, D, K, alpha0, beta0, n0, V0, state):
        a = np.ascontiguousarray(alpha0, dtype=np.float64)
        v = np.ascontiguousarray(V0, dtype=np.float64)
        self.rt.check(self.lib.vmp_gmm_init_state(
            self.ctx, D, K, a.ctypes.data_as(ctypes.c_void_p), float(beta0), float(n0),
            v.ctypes.data_as(ctypes.c_void_p), ptr(state)))

    def stats_from_labels(self, Y, N, D, K, labels, R, state, ws):
        self.rt.check(self.lib.vmp_gmm_stats_from_labels(self.ctx, ptr(Y), N, D, K, ptr(labels),
                                                         ptr(R), ptr(state), ptr(ws)))

    def update_mu(self, D, K, state):
        self.rt.check(self.lib.vmp_gmm_update_mu(self.ctx, D, K, ptr(state)))

    def update_lambda(self, D, K, state):
        self.rt.check(self.lib.vmp_gmm_update_lambda(self.ctx, D, K, ptr(state)))

    def prepare_z(self, D, K, prior_only, state):
        self.rt.check(self.lib.vmp_gmm_prepare_z(self.ctx, D, K, 1 if prior_only else 0,
                                                 ptr(state)))

    def pass_(self, Y, N, D, K, R, state, ws):
        self.rt.check(self.lib.vmp_gmm_pass(self.ctx, ptr(Y), N, D, K, ptr(R), ptr(state),
                                            ptr(ws)))

    def update_alpha(self, D, K, state):
        self.rt.check(self.lib.vmp_gmm_update_alpha(self.ctx, D, K, ptr(state)))

    def lower_bound(self, D, K, state):
        self.rt.check(self.lib.vmp_gmm_lower_bound(self.ctx, D, K, ptr(state)))

    # deterministic annealing: the forms with a coefficient (update) or temperatures (bound)
    def prepare_z_annealed(self, D, K, prior_only, annealing, state):
        self.rt.check(self.lib.vmp_gmm_prepare_z_annealed(self.ctx, D, K, 1 if prior_only else 0,
                                                          float(annealing), ptr(state)))

    def update_annealed(self, D, K, node, annealing, state):
        self.rt.check(self.lib.vmp_gmm_update_annealed(self.ctx, D, K, int(node), float(annealing),
                                                       ptr(state)))

    def lower_bound_annealed(self, D, K, temperatures, state):
        tz, ta, tm, tl = (float(t) for t in temperatures)
        self.rt.check(self.lib.vmp_gmm_lower_bound_annealed(self.ctx, D, K, tz, ta, tm, tl,
                                                            ptr(state)))

    def natural_init(self, D, K, state, phi_mu):
        self.rt.check(self.lib.vmp_gmm_natural_init(self.ctx, D, K, ptr(state), ptr(phi_mu)))

    def natural_step(self, D, K, nodes, mult, scale, state, phi_mu):
        self.rt.check(self.lib.vmp_gmm_natural_step(self.ctx, D, K, int(nodes), float(mult),
                                                    float(scale), ptr(state), ptr(phi_mu)))

    def set_timing(self, on):
        self.rt.check(self.lib.vmp_ctx_set_timing(self.ctx, 1 if on else 0))

    def last_pass_ms(self):
        a, b = ctypes.c_double(), ctypes.c_double()
        self.rt.check(self.lib.vmp_pca_last_pass_ms(self.ctx, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def pass_times_ms(self, cap=64):
        """(pass_ms, reduce_ms) of the most recent timed plate passes, oldest first."""
        a = (ctypes.c_double * cap)()
        b = (ctypes.c_double * cap)()
        n = ctypes.c_int32()
        self.rt.check(self.lib.vmp_pass_times_ms(self.ctx, a, b, cap, ctypes.byref(n)))
        return [(a[i], b[i]) for i in range(n.value)]


class GMMPlan:

    KIND = 'gmm'            # of its checkpoints
    ANNEALING = True        # VB.set_annealing: the updates and the bound read node.annealing

    @staticmethod
    def describe():
        return ("Mixture(Categorical(Dirichlet(const)), Gaussian, GaussianARD(0, const, "
                "shape=(D,), plates=(K,)), Wishart(const, const, plates=(K,))), fully observed, "
                "D <= 32, K <= 64")

    @staticmethod
    def match(nodes, why=None):
        def no(Y, msg):
            if why is not None:
                why.append('fused Gaussian-mixture block, observed node %s: %s'
                           % (Y.name or '<unnamed>', msg))
        # mini-batch multipliers (stochastic VI) go through the generic engine
        if any(any(m != 1 for m in n.plates_multiplier) for n in nodes):
            return None
        for Y in nodes:
            if not isinstance(Y, Mixture) or Y.node_class is not Gaussian:
                continue
            if len(Y.parents) != 3 or len(Y.plates) != 1:
                no(Y, 'it needs plates (N,) and parents (z, mu, Lambda)')
                continue
            if Y._mask is not True:
                no(Y, 'it has missing values')
                continue
            z, mu, Lam = Y.parents
            if not (isinstance(z, Categorical) and isinstance(mu, GaussianARD)
                    and isinstance(Lam, Wishart)):
                no(Y, 'its parents are not (Categorical, GaussianARD, Wishart)')
                continue
            alpha = z.parents[0]
            if not (isinstance(alpha, Dirichlet) and all(p == 1 for p in alpha.plates)):
                no(Y, 'the assignment prior is not one Dirichlet node')
                continue
            if not isinstance(alpha.parents[0], Constant):
                no(Y, 'the concentration of the assignment prior is a node (%s), not a constant'
                      % type(alpha.parents[0]).__name__)
                continue
            N = Y.plates[0]
            K, D = Y.clusters, Y.dims[0][0]
            if D > 32 or K > 64:
                no(Y, 'D = %d, K = %d exceed the limits of the block (D <= 32, K <= 64)' % (D, K))
                continue
            if z.plates != (N,) or mu.plates != (K,) or Lam.plates != (K,) or mu.shape != (D,):
                no(Y, 'plates of z / mu / Lambda are not (N,), (K,), (K,)')
                continue
            m0, b0 = mu.parents
            if not (isinstance(m0, Constant) and not np.any(m0.value)
                    and isinstance(b0, Constant) and b0.is_scalar()):
                no(Y, 'the prior of the means is not N(0, c I) with constants')
                continue
            n0, V0 = Lam.parents
            if not (n0.is_scalar() and V0.value.shape == (D, D)):
                no(Y, 'the Wishart prior is not (scalar degrees, one D x D scale)')
                continue
            if any(len(n.children) != 1 for n in (z, mu, Lam, alpha)) or Y.children:
                no(Y, 'one of its roles has other children as well')
                continue
            return dict(Y=Y, z=z, mu=mu, Lambda=Lam, alpha=alpha)
        return None

    def __init__(self, roles, runtime=None, kernels=None):
        self.roles = roles
        self.Y, self.z, self.mu = roles['Y'], roles['z'], roles['mu']
        self.Lam, self.alpha = roles.get('Lambda'), roles['alpha']
        self.N = self.Y.plates[0]
        self.K, self.D = self.Y.clusters, self.Y.dims[0][0]
        self.alpha0 = np.broadcast_to(self.alpha.parents[0].value, (self.K,)).astype(np.float64)
        self._read_priors()
        self._rt, self._kernels = runtime, kernels
        self._ready = False
        self._version = 0
        self._L_version = -1
        self._L_annealing = None
        self._L = None
        for n in roles.values():
            n._plan = self

    def _read_priors(self):
        self.beta0 = self.mu.parents[1].scalar()
        self.n0 = self.Lam.parents[0].scalar()
        self.V0 = np.array(self.Lam.parents[1].value, dtype=np.float64)

    @property
    def rt(self):
        if self._rt is None:
            self._rt = get_runtime()
        return self._rt

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = GMMKernels(self.rt)
        return self._kernels

    def nodes(self):
        return list(self.roles.values())

    def has_state(self):
        """Device state exists (a recompilation would discard it)."""
        return bool(self._ready)

    def invalidate(self, node):
        _delta.warn_state_discarded(self, node)
        self._ready = False
        self._version += 1
        if node is self.Y and node._mask is not True:
            from .generic import GenericPlan
            GenericPlan(self.nodes())

    def _all_reduce_stats(self):
        """Plate sums over the ranks (node.py:650) -- only when the observation plate was
        declared sharded with Node.shard() on z or Y (the same contract as every other plan)."""
        if not any(getattr(n, '_shard_axis', None) is not None for n in (self.z, self.Y)):
            return
        L = self.layout
        self.rt.all_reduce_sum_(self.state[L.off_T:L.off_T + L.len_T])
        self.rt.all_reduce_sum_(self.state[L.off_zs:L.off_zs + 2])

    def _check_initialisations(self):
        for n in (self.mu, self.Lam, self.alpha):
            if n._init is not None or n.observed:
                raise NotImplementedError('the fused GMM block initialises mu, Lambda and alpha '
                                          'from their priors')

    def _initialise_globals(self):
        """After ``init_state``: what a form of the block sets besides the priors."""

    def _materialize(self):
        if self._ready:
            return
        self._delta = _delta.delta_roles(self.roles)    # point masses until their first update
        rt, k = self.rt, self.kernels
        torch = rt.torch
        N, D, K = self.N, self.D, self.K
        if self.Y._data is None:
            raise ValueError('Node %s has not been observed' % self.Y.name)
        self._check_initialisations()
        rt.sync_stream()
        self.layout = L = k.layout(D, K)
        y = self.Y._data
        if isinstance(y, torch.Tensor) and y.device == rt.device and y.dtype == torch.float64 \
                and tuple(y.shape) == (N, D) and y.is_contiguous():
            self.Yd = y
        else:
            ya = np.array(np.broadcast_to(np.asarray(y, dtype=np.float64), (N, D)), order='C')
            self.Yd = torch.from_numpy(ya).to(rt.device)
        self.Rd = rt.empty(N, K)
        self.state = rt.zeros(int(L.total))
        self.ws = rt.empty(int(k.workspace_doubles(D, K)))
        k.init_state(D, K, self.alpha0, self.beta0, self.n0, self.V0, self.state)
        self._initialise_globals()
        init = self.z._init
        if init is None:
            k.prepare_z(D, K, True, self.state)
            k.pass_(self.Yd, N, D, K, self.Rd, self.state, self.ws)
        else:
            if init[0] == 'value':
                lab = np.asarray(init[1])
                if not np.issubdtype(lab.dtype, np.integer):
                    raise ValueError("Class indices must be integers")
                lab = np.broadcast_to(lab, (N,)).astype(np.int64)
                if lab.size and (lab.min() < 0 or lab.max() >= K):
                    raise ValueError("Class indices out of range [0, %d)" % K)
            else:
                lab = np.random.randint(K, size=N).astype(np.int64)
            self.labels = torch.from_numpy(np.ascontiguousarray(lab)).to(rt.device)
            k.stats_from_labels(self.Yd, N, D, K, self.labels, self.Rd, self.state, self.ws)
        self._all_reduce_stats()
        self._ready = True
        self._version += 1

    def update(self, node):
        self._materialize()
        _delta.updated(self._delta, self.roles, node)
        rt, k = self.rt, self.kernels
        rt.sync_stream()
        D, K = self.D, self.K
        # the coefficient of deterministic annealing (VB.set_annealing); 1.0 runs the plain kernels
        b = self._annealing(node)
        if node is self.mu:
            if b == 1.0:
                k.update_mu(D, K, self.state)
            else:
                k.update_annealed(D, K, STEP_MU, b, self.state)
        elif node is self.Lam:
            if b == 1.0:
                k.update_lambda(D, K, self.state)
            else:
                k.update_annealed(D, K, STEP_LAMBDA, b, self.state)
        elif node is self.z:
            # the factor sits in the C table; the pass is the same launch.  The statistics are
            # sums of r alone, so the all-reduce over a sharded plate is as at 1.0
            if b == 1.0:
                k.prepare_z(D, K, False, self.state)
            else:
                k.prepare_z_annealed(D, K, False, b, self.state)
            k.pass_(self.Yd, self.N, D, K, self.Rd, self.state, self.ws)
            # child -> parent message sums over the sharded plate (node.py:650)
            self._all_reduce_stats()
        elif node is self.alpha:
            if b == 1.0:
                k.update_alpha(D, K, self.state)
            else:
                k.update_annealed(D, K, STEP_ALPHA, b, self.state)
        else:
            return
        self._version += 1

    @staticmethod
    def _annealing(node):
        return float(getattr(node, 'annealing', 1.0))

    def _bound_annealing(self):
        """The coefficients of (z, alpha, mu, Lambda) as the nodes carry them NOW: the temperature
        of a bound term is the node's at the request, not that of its last update."""
        return tuple(self._annealing(n) for n in (self.z, self.alpha, self.mu, self.Lam))

    def _lower_bound_terms(self):
        self._materialize()
        ann = self._bound_annealing()
        if self._L_version != self._version or self._L_annealing != ann:
            rt, k, L = self.rt, self.kernels, self.layout
            rt.sync_stream()
            if all(b == 1.0 for b in ann):
                k.lower_bound(self.D, self.K, self.state)
            else:
                k.lower_bound_annealed(self.D, self.K, [1.0 / b for b in ann], self.state)
            host = self.state[L.off_scal:L.off_L + 8].cpu().numpy()
            status = int(host[3])
            if status == _lib.VMP_ERR_INVALID:
                _lib.raise_for_status(status, 'annealing leaves a Wishart node of the fused '
                                      'Gaussian-mixture block with annealing * (n0 + R_k) <= D - 1 '
                                      'degrees of freedom: raise n0 or the coefficient')
            if status != 0:
                _lib.raise_for_status(status)
            t = host[8:]
            self._L = dict(Y=float(t[0]), z=float(t[1]), alpha=float(t[2]), mu=float(t[3]),
                           Lambda=float(t[4]), total=float(t[5]))
            self._L_version = self._version
            self._L_annealing = ann
        return _delta.bound_terms(self._L, self._delta)

    def lower_bound_contribution(self, node):
        terms = self._lower_bound_terms()
        for key in ('Y', 'z', 'alpha', 'mu', 'Lambda'):
            if node is self.roles.get(key):
                return terms[key]
        return 0.0

    def _blk(self, off, shape):
        n = int(np.prod(shape))
        return self.state[off:off + n].cpu().numpy().reshape(shape).copy()

    # -- persistence: the packed device state + responsibilities ------------------------------------
    def save_state(self, put, nodes, index):
        self._materialize()
        base = 'plans/%d/' % index
        _delta.save(put, base, self._delta)
        put(base + 'kind', np.array([ord(c) for c in self.KIND], dtype=np.uint8))
        put(base + 'dims', np.array([self.N, self.D, self.K], dtype=np.int64))
        put(base + 'state', self.state.cpu().numpy())
        put(base + 'R', self.Rd.cpu().numpy())

    def load_state(self, reader, nodes, index):
        self._materialize()
        base = 'plans/%d/' % index
        self._delta = _delta.load(reader, base)
        if not reader.has(base + 'state'):
            raise Exception("File does not contain the state of the fused mixture block")
        if reader.has(base + 'kind'):
            kind = ''.join(chr(int(c)) for c in np.asarray(reader.get(base + 'kind')).ravel())
            if kind != self.KIND:
                raise ValueError("the checkpoint holds the state of a fused block of kind '%s'; this "
                                 "model runs on %s (kind '%s') -- load it into a model built the "
                                 "same way" % (kind, type(self).__name__, self.KIND))
        dims = tuple(int(v) for v in reader.get(base + 'dims'))
        if dims != (self.N, self.D, self.K):
            raise ValueError('checkpoint is for (N, D, K) = %s, the model has %s'
                             % (dims, (self.N, self.D, self.K)))
        torch = self.rt.torch
        self.state.copy_(torch.from_numpy(np.array(reader.get(base + 'state'), dtype=np.float64)))
        self.Rd.copy_(torch.from_numpy(np.array(reader.get(base + 'R'), dtype=np.float64)))
        self._version += 1

    def get_moments(self, node):
        self._materialize()
        L, D, K = self.layout, self.D, self.K
        if node is self.z:
            return [self.Rd.cpu().numpy()]
        if node is self.mu:
            m = self._blk(L.off_mu, (K, D))
            C = self._blk(L.off_Cmu, (K, D, D))
            return [m, C + m[:, :, None] * m[:, None, :]]
        if node is self.Lam:
            return [self._blk(L.off_Lam, (K, D, D)), self._blk(L.off_logdetLam, (K,))]
        if node is self.alpha:
            return [self._blk(L.off_alpha + L.KP, (K,)).reshape(self.alpha.plates + (K,))]
        if node is self.Y:
            y = self.Yd.cpu().numpy()
            return [y, y[:, :, None] * y[:, None, :]]
        raise NotImplementedError

    def statistics(self):
        """(R_k, sum r y, sum r y y^T) -- host copies of the all-reduced statistics."""
        self._materialize()
        L, D, K = self.layout, self.D, self.K
        T = self._blk(L.off_T, (int(L.KP), int(L.FS)))[:K]
        return T[:, 0], T[:, 1:1 + D], T[:, 1 + D:].reshape(K, D, D)

    def enable_timing(self, on=True):
        self._materialize()
        self.kernels.set_timing(on)

    def last_pass_ms(self):
        return self.kernels.last_pass_ms()

    def pass_times_ms(self, cap=64):
        return self.kernels.pass_times_ms(cap)


# ---- stochastic variational inference -----------------------------------------------------------


def _scalar_multiplier(node):
    """The one factor of a node with at most one plate axis, or None."""
    m = tuple(np.ravel(node.plates_multiplier))
    if len(m) > 1:
        return None
    return float(m[0]) if m else 1.0


def _batch_multiplier(Y, z, globals_):
    """What is wrong with the plate multipliers of the block's nodes (a reason), or None."""
    if any(any(m != 1 for m in n.plates_multiplier) for n in globals_):
        return ('a global node (mu, Lambda or alpha) carries a plates_multiplier; only the '
                'mini-batch plate of z and Y may')
    mz, my = _scalar_multiplier(z), _scalar_multiplier(Y)
    if mz is None or my is None or not (mz > 0 and my > 0) or mz != my:
        return ('the plates_multiplier of z / Y is not one positive factor: %s, %s'
                % (tuple(z.plates_multiplier), tuple(Y.plates_multiplier)))
    return None


def _mean_prior(mu, D):
    """beta0 of a prior N(0, beta0 I) with constants on the means, or a reason (str)."""
    m0, b0 = mu.parents
    if not (isinstance(m0, Constant) and isinstance(b0, Constant)):
        return 'the prior of the means has parents that are nodes, not constants'
    if np.any(m0.value):
        return 'the prior mean of the means is not zero'
    if isinstance(mu, GaussianARD):
        b = np.asarray(b0.value, dtype=np.float64)
        if b.size == 0 or np.any(b != b.reshape(-1)[0]):
            return 'the prior precision of the means is not a scalar multiple of the identity'
        return float(b.reshape(-1)[0])
    P = np.asarray(b0.value, dtype=np.float64)
    if P.ndim < 2 or P.shape[-2:] != (D, D):
        return 'the prior precision of the means is not (D, D)'
    c = float(P.reshape(-1)[0])
    if not np.array_equal(P, np.broadcast_to(c * np.identity(D), P.shape)):
        return 'the prior precision of the means is not a scalar multiple of the identity'
    return c


class GMMSVIPlan(GMMPlan):
    """The block under stochastic variational inference (bayespy/demos/stochastic_inference.py):
    ``z`` and ``Y`` hold a mini-batch of N rows that stands for ``m`` times as many
    (``plates_multiplier``), every step re-observes ``Y`` -- the device state stays -- and updates
    ``z`` (one pass over the batch), and ``gradient_step`` moves mu, Lambda and alpha along their
    natural gradients in one launch (``vmp_gmm_natural_step``).  The means may be written
    ``Gaussian(zeros(D), c I)`` and start from a value or a random draw, the precision may be a
    constant.  Opt-in: ``VB(..., engine='fused')``, tried after ``GMMPlan``."""

    KIND = 'gmm_svi'
    ANNEALING = False       # the natural-gradient step has no annealed form

    @staticmethod
    def _annealing(node):
        """No node of this plan may carry a coefficient other than 1, however it was set."""
        b = float(getattr(node, 'annealing', 1.0))
        if b != 1.0:
            raise NotImplementedError(
                "annealing is not built into the fused GMMSVIPlan plan; build the engine with "
                "VB(..., engine='generic')")
        return b

    @staticmethod
    def describe():
        return ("Mixture(Categorical(Dirichlet(const), plates_multiplier=(m,)), Gaussian, "
                "GaussianARD(0, c, shape=(D,), plates=(K,)) or Gaussian(zeros(D), c I, plates=(K,)), "
                "Wishart(const, const, plates=(K,)) or a constant SPD (D, D) / (K, D, D) array), "
                "fully observed mini-batches, D <= 32, K <= 64")

    @staticmethod
    def match(nodes, why=None):
        def no(Y, msg):
            if why is not None:
                why.append('fused Gaussian-mixture block (stochastic VI), observed node %s: %s'
                           % (Y.name or '<unnamed>', msg))
        for Y in nodes:
            if not isinstance(Y, Mixture) or Y.node_class is not Gaussian:
                continue
            if len(Y.parents) != 3 or len(Y.plates) != 1:
                no(Y, 'it needs plates (N,) and parents (z, mu, Lambda)')
                continue
            if Y._mask is not True:
                no(Y, 'it has missing values (a mask)')
                continue
            z, mu, Lam = Y.parents
            const_lam = isinstance(Lam, Constant)
            if not (isinstance(z, Categorical) and type(mu) in (GaussianARD, Gaussian)
                    and (const_lam or isinstance(Lam, Wishart))):
                no(Y, 'its parents are not (Categorical, GaussianARD or Gaussian, Wishart or a '
                      'constant array)')
                continue
            alpha = z.parents[0]
            if not (isinstance(alpha, Dirichlet) and all(p == 1 for p in alpha.plates)):
                no(Y, 'the assignment prior is not one Dirichlet node')
                continue
            if not isinstance(alpha.parents[0], Constant):
                no(Y, 'the concentration of the assignment prior is a node (%s), not a constant'
                      % type(alpha.parents[0]).__name__)
                continue
            latent = [z, mu, alpha] + ([] if const_lam else [Lam])
            if not all(any(n is m for m in nodes) for n in latent):
                continue
            if any(getattr(n, '_shard_axis', None) is not None for n in latent + [Y]):
                no(Y, 'its plates are sharded over ranks (Node.shard)')
                continue
            N = Y.plates[0]
            K, D = Y.clusters, Y.dims[0][0]
            if D > 32 or K > 64:
                no(Y, 'D = %d, K = %d exceed the limits of the block (D <= 32, K <= 64)' % (D, K))
                continue
            if z.plates != (N,) or mu.plates != (K,) or tuple(mu.dims[0]) != (D,) \
                    or (not const_lam and Lam.plates != (K,)):
                no(Y, 'plates of z / mu / Lambda are not (N,), (K,), (K,)')
                continue
            bad = _batch_multiplier(Y, z, latent[1:])
            if bad:
                no(Y, bad)
                continue
            beta0 = _mean_prior(mu, D)
            if isinstance(beta0, str):
                no(Y, beta0)
                continue
            if const_lam:
                P = np.asarray(Lam.value, dtype=np.float64)
                if P.shape not in ((D, D), (K, D, D)):
                    no(Y, 'the constant precision is not a (D, D) or (K, D, D) array')
                    continue
                spd = np.array_equal(P, np.swapaxes(P, -1, -2))
                if spd:
                    try:
                        np.linalg.cholesky(P)
                    except np.linalg.LinAlgError:
                        spd = False
                if not spd:
                    no(Y, 'the constant precision is not symmetric positive definite')
                    continue
            else:
                n0, V0 = Lam.parents
                if not (isinstance(n0, Constant) and isinstance(V0, Constant) and n0.is_scalar()
                        and V0.value.shape == (D, D)):
                    no(Y, 'the Wishart prior is not (scalar degrees, one D x D scale)')
                    continue
            if any(len(n.children) != 1 for n in latent) or Y.children:
                no(Y, 'one of its roles has other children as well')
                continue
            roles = dict(Y=Y, z=z, mu=mu, alpha=alpha)
            if not const_lam:
                roles['Lambda'] = Lam
            return roles
        return None

    def __init__(self, roles, runtime=None, kernels=None):
        super().__init__(roles, runtime=runtime, kernels=kernels)
        self._m_seen = _scalar_multiplier(self.z)
        self._z_init_seen = None
        self._Ybuf = None

    def _read_priors(self):
        D = self.D
        self.beta0 = _mean_prior(self.mu, D)
        if self.Lam is not None:
            self.n0 = self.Lam.parents[0].scalar()
            self.V0 = np.array(self.Lam.parents[1].value, dtype=np.float64)
            self.Lam_const = None
        else:
            # a constant precision sits in the slots of <Lambda>, <log|Lambda|>; the Wishart slots
            # hold a placeholder that nothing steps and whose bound term is not read
            self.n0, self.V0 = float(D), np.identity(D)
            P = np.asarray(self.Y.parents[2].value, dtype=np.float64)
            self.Lam_const = np.array(np.broadcast_to(P, (self.K, D, D)), order='C')

    # -- state -----------------------------------------------------------------------------------
    def _multiplier(self):
        """The multiplier of the mini-batch plate as the nodes carry it now (it has a setter)."""
        bad = _batch_multiplier(self.Y, self.z, [n for n in (self.mu, self.Lam, self.alpha)
                                                 if n is not None])
        if bad:
            raise ValueError('fused Gaussian-mixture block: ' + bad)
        return _scalar_multiplier(self.z)

    def _is_device_batch(self, y):
        torch = self.rt.torch
        return isinstance(y, torch.Tensor) and y.device == self.rt.device \
            and y.dtype == torch.float64 and tuple(y.shape) == (self.N, self.D) \
            and y.is_contiguous()

    def invalidate(self, node):
        Y, z = self.Y, self.z
        live = self._ready and Y.observed and Y._mask is True \
            and tuple(np.shape(Y._data)) == (self.N, self.D)
        if live and (node is z or node is Y) and _scalar_multiplier(z) != self._m_seen \
                and GMMSVIPlan.match(self.nodes()) is not None:
            # the setter of plates_multiplier: the state stays, the next operation reads the factor
            self._m_seen = _scalar_multiplier(z)
            self._version += 1
            if node is z:
                return
        if live and node is Y:
            # the next mini-batch -- a new array, or the same one filled again: the data changes,
            # the state stays
            y, torch = Y._data, self.rt.torch
            if self._is_device_batch(y):
                self.Yd = y
            else:
                if self._Ybuf is None:
                    self._Ybuf = self.rt.empty(self.N, self.D)
                src = y if isinstance(y, torch.Tensor) else \
                    torch.from_numpy(np.array(y, dtype=np.float64, order='C'))
                self._Ybuf.copy_(src)
                self.Yd = self._Ybuf
            self._version += 1
            return
        if live and node is z and z._init is self._z_init_seen:
            return                  # the setter wrote the factor that was there: nothing changed
        _delta.warn_state_discarded(self, node)
        self._ready = False
        self._version += 1
        if GMMSVIPlan.match(self.nodes()) is None:
            from .generic import GenericPlan
            GenericPlan(self.nodes())

    def _check_initialisations(self):
        for n in (self.Lam, self.alpha):
            if n is not None and (n._init is not None or n.observed):
                raise NotImplementedError('the fused GMM block initialises Lambda and alpha from '
                                          'their priors')
        init = self.mu._init
        if self.mu.observed or (init is not None and init[0] not in ('value', 'random')):
            raise NotImplementedError('the fused GMM block initialises mu from its prior, from a '
                                      'value or from a random draw')

    def _initialise_globals(self):
        rt, k, L = self.rt, self.kernels, self.layout
        torch = rt.torch
        D, K = self.D, self.K
        self._m_seen = _scalar_multiplier(self.z)
        self._z_init_seen = self.z._init
        if self._Ybuf is None and not self._is_device_batch(self.Y._data):
            self._Ybuf = self.Yd                    # the plan's own copy of a host array
        # q(mu) in natural parameters: the prior's until the first update or step, also under a
        # point mass (initialize_from_value leaves phi alone, expfamily.py:193-212)
        self.phi_mu = rt.empty(K * (D + D * D))
        k.natural_init(D, K, self.state, self.phi_mu)
        if self.Lam_const is not None:
            self.state[L.off_Lam:L.off_Lam + K * D * D].copy_(
                torch.from_numpy(self.Lam_const.reshape(-1)))
            self.state[L.off_logdetLam:L.off_logdetLam + K].copy_(
                torch.from_numpy(np.ascontiguousarray(np.linalg.slogdet(self.Lam_const)[1])))
        init = self.mu._init
        if init is not None:
            if init[0] == 'value':
                x = np.array(np.broadcast_to(np.asarray(init[1], dtype=np.float64), (K, D)))
            else:
                # a draw from the prior N(0, I / beta0), as the generic engine draws it
                Lc = np.linalg.cholesky(np.identity(D) / self.beta0 + 1e-12 * np.eye(D))
                x = np.random.randn(K, D) @ Lc.T
            self.state[L.off_mu:L.off_mu + K * D].copy_(
                torch.from_numpy(np.ascontiguousarray(x).reshape(-1)))
            self.state[L.off_Cmu:L.off_Cmu + K * D * D].zero_()

    # -- operations ------------------------------------------------------------------------------
    def _bit(self, node):
        if node is self.mu:
            return STEP_MU
        if self.Lam is not None and node is self.Lam:
            return STEP_LAMBDA
        if node is self.alpha:
            return STEP_ALPHA
        return 0

    def update(self, node):
        if node is self.z:
            return super().update(node)
        bit = self._bit(node)
        if not bit:
            return
        self._materialize()
        m = self._multiplier()
        _delta.updated(self._delta, self.roles, node)
        self.rt.sync_stream()
        self.kernels.natural_step(self.D, self.K, bit, m, 1.0, self.state, self.phi_mu)
        self._version += 1

    def gradient_step(self, nodes, scale=1.0):
        """phi <- phi + scale * (phi* - phi) for mu, Lambda and alpha among ``nodes``, in one
        launch: every optimum phi* is taken from the moments and statistics present before any
        node moves (vmp.py:432-440).  A mean that is still a point mass steps from its prior's
        parameters, as on the generic engine."""
        from ...nodes.node import Stochastic
        bits, todo = 0, []
        for node in nodes:
            if not isinstance(node, Stochastic) or node.observed:
                continue
            if node is self.z:
                raise NotImplementedError(
                    'gradient step of %s: the fused Gaussian-mixture block keeps no natural '
                    'parameters of the responsibilities to step from; update it (Q.update(%r)), or '
                    'use VB(..., engine="generic")' % (node.name, node.name))
            if self._bit(node):
                bits |= self._bit(node)
                todo.append(node)
        if not bits:
            return
        self._materialize()
        m = self._multiplier()
        for node in todo:
            _delta.updated(self._delta, self.roles, node)
        self.rt.sync_stream()
        self.kernels.natural_step(self.D, self.K, bits, m, scale, self.state, self.phi_mu)
        self._version += 1

    def _lower_bound_terms(self):
        self._materialize()
        if self._L_version != self._version:
            super()._lower_bound_terms()
            # the mini-batch stands for m times as many rows (expfamily.py:470-480); a constant
            # precision has no term; the total is formed again from the terms
            m = self._multiplier()
            t = self._L
            t['Y'], t['z'] = m * t['Y'], m * t['z']
            if self.Lam is None:
                t['Lambda'] = 0.0
            t['total'] = t['Y'] + t['z'] + t['alpha'] + t['mu'] + t['Lambda']
        return _delta.bound_terms(self._L, self._delta)

    # -- persistence: + the natural parameters of the means --------------------------------------
    def save_state(self, put, nodes, index):
        super().save_state(put, nodes, index)
        put('plans/%d/phi_mu' % index, self.phi_mu.cpu().numpy())

    def load_state(self, reader, nodes, index):
        super().load_state(reader, nodes, index)
        self.phi_mu.copy_(self.rt.torch.from_numpy(
            np.array(reader.get('plans/%d/phi_mu' % index), dtype=np.float64)))
