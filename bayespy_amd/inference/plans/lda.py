"""
Execution plan of the latent-Dirichlet-allocation block (doc/source/examples/lda.rst)

    p_topic = Dirichlet(a, plates=(D,));  p_word = Dirichlet(b, plates=(K,))
    topics  = Categorical(Gate(document_indices, p_topic), plates=(n,))
    words   = Categorical(Gate(topics, p_word));  words.observe(corpus)

with constant concentrations, a fully observed ``words`` and K <= 64.  The plan owns, in HBM: the
Dirichlet parameters and <log> tables of ``p_topic`` (D x K) and ``p_word`` (kept transposed,
V x K), the tables the last ``topics`` update used, the counts N_dk and N_vk, and the tokens as
int32 indices in two sorted layouts (by document and by word, with offsets).  Nothing of size
tokens x K, tokens x V or tokens x D exists: the responsibilities of ``topics`` are formed inside
``vmp_lda_token_pass`` and only on request written out (``topics.get_moments()``).

All token terms of the lower bound follow from the counts, sum_n lse_n and the tables:
    <log p(words)>            = sum_vk N_vk <log beta>[k, v]
    <log p(topics)> + entropy = sum_dk N_dk <log theta>[d, k]
                                + sum_n lse_n - sum_dk N_dk <log theta>_used - sum_vk N_vk <log beta>_used
"""
import ctypes

import numpy as np

from . import _delta
from ._dirichlet import DirichletKernels, prior_table

from ... import _lib
from ...device import get_runtime, ptr
from ...nodes.node import Constant
from ...nodes.dirichlet import Dirichlet
from ...nodes.categorical import Categorical
from ...nodes.take import Gate

LDA_MAX_K = 64          # vmp_lda_limits


class LDAKernels(DirichletKernels):

    def __init__(self, rt):
        self.rt, self.lib, self.ctx = rt, rt.lib, rt.ctx

    def plan(self, n, K):
        """(lane group, tokens per chunk, workspace doubles) of the token pass."""
        g, c, w = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        rc = self.lib.vmp_lda_plan(n, K, ctypes.byref(g), ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the fused LDA block supports K <= %d and fewer than 2^31 '
                                      'tokens' % LDA_MAX_K)
        return g.value, c.value, w.value

    def token_pass(self, n, D, V, K, lay, labels, elog_theta, elog_beta_t, phases, lse, ws, Ndk,
                   Nvk, scal, orig=None, phi=None):
        def p(t):
            return ptr(t) if t is not None else None
        self.rt.check(self.lib.vmp_lda_token_pass(
            self.ctx, n, D, V, K, p(lay['doc_d']), p(lay['word_d']), p(lay['doc_off']),
            p(lay['word_w']), p(lay['doc_w']), p(lay['pos_w']), p(lay['word_off']), p(labels),
            p(elog_theta), p(elog_beta_t), phases, p(lse), p(ws), p(Ndk), p(Nvk), p(scal),
            p(orig), p(phi)))

    def dirichlet_step_ws(self, rows, cols, rs, cs):
        """Doubles of the workspace of ``dirichlet_step`` for this table."""
        w = ctypes.c_int64()
        rc = self.lib.vmp_lda_dirichlet_step_workspace(rows, cols, rs, cs, ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'vmp_lda_dirichlet_step_workspace')
        return w.value

    def dirichlet_step(self, rows, cols, rs, cs, prior, counts, mult, scale, alpha, elog, ws,
                       bound):
        self.rt.check(self.lib.vmp_lda_dirichlet_step(
            self.ctx, rows, cols, rs, cs, ptr(prior), ptr(counts) if counts is not None else None,
            float(mult), float(scale), ptr(alpha), ptr(elog), ptr(ws), ptr(bound)))


def _structure(words):
    """The nodes of the two-level structure under the observed Categorical ``words``, or None."""
    if not isinstance(words, Categorical) or type(words) is not Categorical:
        return None
    g2 = words.parents[0]
    if not isinstance(g2, Gate):
        return None
    topics, p_word = g2.parents
    if type(topics) is not Categorical or not isinstance(p_word, Dirichlet):
        return None
    g1 = topics.parents[0]
    if not isinstance(g1, Gate):
        return None
    idx, p_topic = g1.parents
    if not isinstance(idx, Constant) or not isinstance(p_topic, Dirichlet):
        return None
    return dict(words=words, topics=topics, p_word=p_word, p_topic=p_topic, gate_word=g2,
                gate_topic=g1, document_indices=idx)


def _no_multiplier(words, topics, p_word, p_topic):
    if any(any(m != 1 for m in n.plates_multiplier) for n in (words, topics, p_word, p_topic)):
        return ('plates_multiplier (mini-batches) goes through the generic engine '
                '(VB(..., engine="fused") runs mini-batches of tokens on the block)')
    return None


def _scalar_multiplier(node):
    """The one factor of a node with at most one plate axis, or None."""
    m = tuple(np.ravel(node.plates_multiplier))
    if len(m) > 1:
        return None
    return float(m[0]) if m else 1.0


def _batch_multiplier(words, topics, p_word, p_topic):
    if any(any(m != 1 for m in n.plates_multiplier) for n in (p_word, p_topic)):
        return 'a Dirichlet carries a plates_multiplier'
    mw, mt = _scalar_multiplier(words), _scalar_multiplier(topics)
    if mw is None or mt is None or not (mw > 0 and mt > 0):
        return ('the plates_multiplier of words / topics is not one positive factor: %s, %s'
                % (tuple(words.plates_multiplier), tuple(topics.plates_multiplier)))
    if mw != mt:
        return ('words and topics carry unequal plates_multiplier (%r and %r)' % (mw, mt))
    return None


def _narrow_topics(K):
    if K > LDA_MAX_K:
        return 'n_topics = %d exceeds the limit of the block (K <= %d)' % (K, LDA_MAX_K)
    return None


def _constant_parents(p_topic, p_word, nodes):
    """(reason or None, further roles): both concentrations are constants."""
    bad = [n for n in (p_topic, p_word) if not isinstance(n.parents[0], Constant)]
    if bad:
        return ('the concentration of %s is a node (%s), not a constant'
                % (bad[0].name, type(bad[0].parents[0]).__name__)), None
    return None, {}


def _match(nodes, why, multiplier_rule, label='fused LDA block', topics_rule=_narrow_topics,
           parent_rule=_constant_parents):
    """The roles of the first latent-Dirichlet-allocation structure among ``nodes`` that meets
    every condition of the block, or None; ``multiplier_rule`` says what plate multipliers may
    be there, ``topics_rule`` what numbers of topics (a reason, or None) and ``parent_rule`` what
    parents the Dirichlets may have (a reason or None, and the roles it adds); ``label`` opens
    every reason."""
    for words in nodes:
        r = _structure(words)
        if r is None:
            continue

        def no(msg, words=words):
            if why is not None:
                why.append('%s, observed node %s: %s' % (label, words.name or '<unnamed>', msg))
        topics, p_word, p_topic = r['topics'], r['p_word'], r['p_topic']
        g1, g2, idx = r['gate_topic'], r['gate_word'], r['document_indices']
        four = (words, topics, p_word, p_topic)
        if not all(any(n is m for m in nodes) for n in four):
            continue
        bad = multiplier_rule(words, topics, p_word, p_topic)
        if bad:
            no(bad)
            continue
        if any(getattr(n, '_shard_axis', None) is not None for n in r.values()):
            no('a plate is sharded over ranks')
            continue
        if not words.observed:
            no('it is not observed')
            continue
        if words._mask is not True:
            no('it has a mask')
            continue
        bad, extra = parent_rule(p_topic, p_word, nodes)
        if bad:
            no(bad)
            continue
        if len(topics.plates) != 1 or idx.value.ndim != 1:
            no('it needs one token plate axis, topics has plates %s and the indices have '
               'shape %s' % (topics.plates, idx.value.shape))
            continue
        n, K = topics.plates[0], topics.categories
        if g1.gated_plate != -1 or g2.gated_plate != -1 or len(p_topic.plates) != 1 \
                or p_word.plates != (K,) or idx.value.shape != (n,) or words.plates != (n,):
            no('plates of p_topic / p_word / indices are not (D,), (K,), (n,)')
            continue
        bad = topics_rule(K)
        if bad:
            no(bad)
            continue
        kids = ((p_topic, [g1]), (g1, [topics]), (topics, [g2]), (p_word, [g2]),
                (g2, [words]), (words, []))
        if any([c for c, _ in n.children] != want for n, want in kids) \
                or any(c is not g1 for c, _ in idx.children):
            no('one of its roles has other children as well')
            continue
        if topics.observed or p_topic.observed or p_word.observed:
            no('topics or a Dirichlet is observed')
            continue
        if topics._init is not None and topics._init[0] != 'value':
            no('topics is initialised by %s' % topics._init[0])
            continue
        if any(n._init is not None and n._init[0] not in ('value', 'random')
               for n in (p_topic, p_word)):
            no('a Dirichlet is initialised from parameters')
            continue
        return dict(r, **extra)
    return None


class LDAPlan:

    @staticmethod
    def describe():
        return ("Categorical(Gate(Categorical(Gate(indices, Dirichlet(const, plates=(D,))), "
                "plates=(n,)), Dirichlet(const, plates=(K,)))), fully observed, K <= %d"
                % LDA_MAX_K)

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why, _no_multiplier)

    def _token_multiplier(self):
        return 1.0

    def __init__(self, roles, runtime=None, kernels=None):
        self.roles = roles
        self.words, self.topics = roles['words'], roles['topics']
        self.p_word, self.p_topic = roles['p_word'], roles['p_topic']
        self.index = roles['document_indices']
        self.n = self.topics.plates[0]
        self.K = self.topics.categories
        self.D = self.p_topic.plates[0]
        self.V = self.p_word.dims[0][0]
        self._rt, self._kernels = runtime, kernels
        self._ready = False
        self._layout_stale = False
        self._lazy_recount = False
        self._version = 0
        self._L_version = -1
        self._L = None
        for nd in roles.values():
            nd._plan = self

    @property
    def rt(self):
        if self._rt is None:
            self._rt = get_runtime()
        return self._rt

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = LDAKernels(self.rt)
        return self._kernels

    def nodes(self):
        return list(self.roles.values())

    def has_state(self):
        return bool(self._ready)

    def invalidate(self, node):
        if node is self.words and node.observed and node._mask is True:
            # new tokens of the same count: the layouts are built again, the Dirichlets stay
            self._layout_stale = True
            self._version += 1
            return
        _delta.warn_state_discarded(self, node)
        self._ready = False
        self._version += 1
        if node is self.words or any(any(m != 1 for m in nd.plates_multiplier)
                                     for nd in (self.words, self.topics)):
            from .generic import GenericPlan
            GenericPlan(self.nodes())

    def constant_changed(self, const):
        """``document_indices.set_value``: the layouts are built again, the Dirichlets stay."""
        self._layout_stale = True
        self._version += 1

    # -- set-up ------------------------------------------------------------------------------------
    def _index_tensor(self, x):
        """(int64 device tensor of the n indices ``x``, device flag "a value is no integer" or
        None): a host array is checked on the host, a tensor stays where it is."""
        torch = self.rt.torch
        frac = None
        if isinstance(x, torch.Tensor):
            t = x.to(self.rt.device)
            if t.dtype.is_floating_point:
                frac = (t != t.round()).any()
            t = t.to(torch.int64)
        else:
            a = np.asarray(x)
            if a.dtype.kind == 'f':
                if np.any(a != np.round(a)):
                    raise ValueError("Values must be integers")
            elif a.dtype.kind not in 'iub':
                raise ValueError("Values must be integers")
            a = np.array(np.broadcast_to(a, (self.n,)), dtype=np.int64, order='C')
            t = torch.from_numpy(a).to(self.rt.device)
        t = t.reshape(-1)
        if t.numel() != self.n:
            t = t.expand(self.n).contiguous()
        return t, frac

    def _indices(self, x, upper):
        """int64 device tensor of the indices ``x`` after the reference's checks
        (categorical.py:35-40)."""
        t, frac = self._index_tensor(x)
        if frac is not None and bool(frac.item()):
            raise ValueError("Values must be integers")
        if t.numel() and (int(t.min().item()) < 0 or int(t.max().item()) >= upper):
            raise ValueError("Invalid category index")
        return t

    def _token_indices(self):
        """(documents, words) of the tokens as checked int64 device tensors."""
        return self._indices(self.index.value, self.D), self._indices(self.words._data, self.V)

    def _build_layouts(self):
        """Tokens sorted by (document, word) with document offsets, and sorted by (word, document)
        with word offsets: both depend on the multiset of tokens only, not on their order."""
        rt = self.rt
        torch = rt.torch
        if self.words._data is None:
            raise ValueError('Node %s has not been observed' % self.words.name)
        doc, word = self._token_indices()
        n, D, V = self.n, self.D, self.V
        order = torch.argsort(doc * V + word, stable=True)
        doc_d, word_d = doc[order], word[order]
        order_w = torch.argsort(word_d * D + doc_d, stable=True)

        def offsets(ix, m):
            off = torch.zeros(m + 1, dtype=torch.int64, device=rt.device)
            if n:
                off[1:] = torch.cumsum(torch.bincount(ix, minlength=m), 0)
            return off
        i32 = torch.int32
        self.lay = dict(doc_d=doc_d.to(i32), word_d=word_d.to(i32), doc_off=offsets(doc, D),
                        word_w=word_d[order_w].to(i32), doc_w=doc_d[order_w].to(i32),
                        pos_w=order_w.to(i32), word_off=offsets(word, V))
        self.orig = order.to(i32)
        self._layout_stale = False

    def _prior_table(self, node, shape):
        """The concentration of a Dirichlet at set-up, broadcast to ``shape`` (host)."""
        return prior_table(node, shape)

    def _init_dirichlet(self, node, prior):
        """Initial <log> table of a Dirichlet: from the prior (device), or the log of a value /
        of a draw from the prior (host, set-up only)."""
        init = node._init
        if init is None:
            return None
        if init[0] == 'value':
            x = np.broadcast_to(np.asarray(init[1], dtype=np.float64), prior.shape)
        else:
            x = np.random.gamma(prior)
            x = x / x.sum(axis=-1, keepdims=True)
        with np.errstate(divide='ignore'):
            return np.log(x)

    def _materialize(self, recount=True):
        """``recount=False``: the caller forms the counts on the new layouts itself."""
        if self._ready:
            if self._layout_stale:
                self._build_layouts()
                if recount:
                    self._recount()
            return
        self._delta = _delta.delta_roles(self.roles)
        rt, k = self.rt, self.kernels
        torch = rt.torch
        n, D, V, K = self.n, self.D, self.V, self.K
        rt.sync_stream()
        self.group, self.chunk, wsd = k.plan(n, K)
        self._build_layouts()
        pt = self._prior_table(self.p_topic, (D, K))
        pw = self._prior_table(self.p_word, (K, V))
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order='C')).to(rt.device)  # noqa: E731
        self.prior_theta, self.prior_beta_t = up(pt), up(pw.T)
        self.alpha_theta, self.alpha_beta_t = rt.empty(D, K), rt.empty(V, K)
        self.elog_theta, self.elog_beta_t = rt.empty(D, K), rt.empty(V, K)
        self.used_theta, self.used_beta_t = rt.empty(D, K), rt.empty(V, K)
        self.Ndk, self.Nvk = rt.zeros(D, K), rt.zeros(V, K)
        self.lse = rt.empty(max(n, 1))
        self.ws = rt.empty(int(wsd))
        self.ws_small = rt.empty(max(D, K, 1024))
        # [0] sum lse, [1] N_dk . used theta, [2] N_vk . used beta, [3] bound of p_topic,
        # [4] bound of p_word, [5] N_dk . theta, [6] N_vk . beta
        self.scal = rt.zeros(8)
        k.dirichlet(D, K, K, 1, self.prior_theta, None, self.alpha_theta, self.elog_theta,
                    self.ws_small, self.scal[3:4])
        k.dirichlet(K, V, 1, K, self.prior_beta_t, None, self.alpha_beta_t, self.elog_beta_t,
                    self.ws_small, self.scal[4:5])
        e = self._init_dirichlet(self.p_topic, pt)
        if e is not None:
            self.elog_theta.copy_(up(e))
            self.alpha_theta.fill_(float('nan'))         # a point mass has no parameters
        e = self._init_dirichlet(self.p_word, pw)
        if e is not None:
            self.elog_beta_t.copy_(up(e.T))
            self.alpha_beta_t.fill_(float('nan'))
        # topics: fixed labels, or its moments under the prior (no word term)
        self.labels = self.labels_orig = None
        self.has_word_term = False
        init = self.topics._init
        if init is not None:
            lab = self._indices(init[1], K)
            self.labels_orig = lab
            self.labels = lab[self.orig.to(torch.int64)].to(torch.int32)
        self._ready = True
        self.used_theta.copy_(self.elog_theta)
        self._recount()

    def _recount(self):
        """The counts and sums of the present ``topics`` state on the present layouts."""
        k = self.kernels
        if self.labels_orig is not None:
            torch = self.rt.torch
            self.labels = self.labels_orig[self.orig.to(torch.int64)].to(torch.int32)
        k.token_pass(self.n, self.D, self.V, self.K, self.lay, self.labels, self.used_theta,
                     self.used_beta_t if self.has_word_term else None, 7, self.lse, self.ws,
                     self.Ndk, self.Nvk, self.scal)
        self._version += 1

    # -- operations ----------------------------------------------------------------------------------
    def update(self, node):
        self._materialize(recount=not (self._lazy_recount and node is self.topics))
        _delta.updated(self._delta, self.roles, node)
        rt, k = self.rt, self.kernels
        rt.sync_stream()
        D, V, K = self.D, self.V, self.K
        if node is self.topics:
            self.used_theta.copy_(self.elog_theta)
            self.used_beta_t.copy_(self.elog_beta_t)
            self.labels = None
            self.labels_orig = None
            self.has_word_term = True
            k.token_pass(self.n, D, V, K, self.lay, None, self.used_theta, self.used_beta_t, 7,
                         self.lse, self.ws, self.Ndk, self.Nvk, self.scal)
        elif node is self.p_topic or node is self.p_word:
            self._update_dirichlet(node)
        else:
            return
        self._version += 1

    def _update_dirichlet(self, node):
        k = self.kernels
        D, V, K = self.D, self.V, self.K
        if node is self.p_topic:
            k.dirichlet(D, K, K, 1, self.prior_theta, self.Ndk, self.alpha_theta, self.elog_theta,
                        self.ws_small, self.scal[3:4])
        else:
            k.dirichlet(K, V, 1, K, self.prior_beta_t, self.Nvk, self.alpha_beta_t,
                        self.elog_beta_t, self.ws_small, self.scal[4:5])

    def _lower_bound_terms(self):
        self._materialize()
        if self._L_version != self._version:
            rt, k = self.rt, self.kernels
            rt.sync_stream()
            k.dot(self.D * self.K, self.Ndk, self.elog_theta, self.ws_small, self.scal[5:6])
            k.dot(self.V * self.K, self.Nvk, self.elog_beta_t, self.ws_small, self.scal[6:7])
            s = self.scal.cpu().numpy()
            entropy = 0.0 if self.labels is not None else float(s[0] - s[1] - s[2])
            m = self._token_multiplier()
            t = dict(words=m * float(s[6]), topics=m * (float(s[5]) + entropy),
                     p_topic=float(s[3]), p_word=float(s[4]))
            t['total'] = t['words'] + t['topics'] + t['p_topic'] + t['p_word']
            self._L = t
            self._L_version = self._version
        return _delta.bound_terms(self._L, self._delta)

    def lower_bound_contribution(self, node):
        terms = self._lower_bound_terms()
        for key in ('words', 'topics', 'p_topic', 'p_word'):
            if node is self.roles[key]:
                return terms[key]
        return 0.0

    def responsibilities(self):
        """tokens x K responsibilities of ``topics`` as a device array in the caller's token order:
        formed by the token pass in its write mode from the tables of the last ``topics`` update;
        not kept."""
        self._materialize()
        rt = self.rt
        rt.sync_stream()
        phi = rt.empty(self.n, self.K)
        if self.n:
            self.kernels.token_pass(self.n, self.D, self.V, self.K, self.lay, self.labels,
                                    self.used_theta,
                                    self.used_beta_t if self.has_word_term else None, 1, self.lse,
                                    self.ws, self.Ndk, self.Nvk, self.scal, self.orig, phi)
        return phi

    def get_moments(self, node):
        self._materialize()
        if node is self.p_topic:
            return [self.elog_theta.cpu().numpy().copy()]
        if node is self.p_word:
            return [self.elog_beta_t.cpu().numpy().T.copy()]
        if node is self.topics:
            return [self.responsibilities().cpu().numpy()]
        if node is self.index:
            return [self.index.value]
        if node is self.words:
            raise NotImplementedError(
                'the fused LDA block never forms the tokens x vocabulary one-hot moments of %s '
                '(the observed indices are words._data); use VB(..., engine="generic") to get the '
                'dense array' % self.words.name)
        raise NotImplementedError('the fused LDA block does not form the moments of the gate %s; '
                                  'use VB(..., engine="generic")' % node.name)

    # -- persistence -----------------------------------------------------------------------------------
    _SAVED = ('alpha_theta', 'alpha_beta_t', 'elog_theta', 'elog_beta_t', 'used_theta',
              'used_beta_t', 'Ndk', 'Nvk', 'scal')
    _KIND = 'lda'           # names the form in a checkpoint
    _OTHER_KINDS = {'lda': 'the fused LDA block (K <= %d)' % LDA_MAX_K,
                    'lda_wide': "the wide-topic form of the fused LDA block "
                                "(engine='fused+topics', K > %d)" % LDA_MAX_K,
                    'lda_hyper': "the fused LDA block with learnt concentrations "
                                 "(engine='fused+hyper', K <= %d)" % LDA_MAX_K,
                    'lda_wide_hyper': "the wide-topic form of the fused LDA block with learnt "
                                      "concentrations (engine='fused+topics+hyper', K > %d)"
                                      % LDA_MAX_K}

    def save_state(self, put, nodes, index):
        self._materialize()
        base = 'plans/%d/' % index
        _delta.save(put, base, self._delta)
        put(base + 'kind', np.array([ord(c) for c in self._KIND], dtype=np.uint8))
        put(base + 'dims', np.array([self.n, self.D, self.V, self.K], dtype=np.int64))
        put(base + 'flags', np.array([1 if self.has_word_term else 0,
                                      1 if self.labels is not None else 0], dtype=np.int64))
        if self.labels is not None:
            put(base + 'labels', self.labels_orig.cpu().numpy())
        for name in self._SAVED:
            put(base + name, getattr(self, name).cpu().numpy())

    def load_state(self, reader, nodes, index):
        self._materialize()
        base = 'plans/%d/' % index
        kind = bytes(np.asarray(reader.get(base + 'kind'), dtype=np.uint8)).decode() \
            if reader.has(base + 'kind') else None
        if kind != self._KIND:
            if kind in self._OTHER_KINDS:
                raise Exception("File holds the state of %s, this model runs on %s"
                                % (self._OTHER_KINDS[kind], self._OTHER_KINDS[self._KIND]))
            raise Exception("File does not contain the state of the fused LDA block")
        dims = tuple(int(v) for v in reader.get(base + 'dims'))
        if dims != (self.n, self.D, self.V, self.K):
            raise ValueError('checkpoint is for (n, D, V, K) = %s, the model has %s'
                             % (dims, (self.n, self.D, self.V, self.K)))
        torch = self.rt.torch
        self._delta = _delta.load(reader, base)
        flags = [int(v) for v in reader.get(base + 'flags')]
        self.has_word_term = bool(flags[0])
        if flags[1]:
            self.labels_orig = torch.from_numpy(
                np.array(reader.get(base + 'labels'), dtype=np.int64)).to(self.rt.device)
            self.labels = self.labels_orig[self.orig.to(torch.int64)].to(torch.int32)
        else:
            self.labels = self.labels_orig = None
        for name in self._SAVED:
            getattr(self, name).copy_(torch.from_numpy(
                np.array(reader.get(base + name), dtype=np.float64)).to(self.rt.device))
        self._version += 1


class LDASVIPlan(LDAPlan):
    """The block under stochastic variational inference (lda.rst, second half): ``words`` and
    ``topics`` hold a mini-batch of n tokens that stands for ``m`` times as many
    (``plates_multiplier``), every step re-observes ``words``, sets the document indices and updates
    ``topics`` -- one token pass over the batch -- and ``gradient_step`` moves the two corpus-sized
    Dirichlet tables along their natural gradients (``vmp_lda_dirichlet_step``).  Opt-in:
    ``VB(..., engine='fused')``."""

    @staticmethod
    def describe():
        return LDAPlan.describe() + ('; words and topics may carry one equal plates_multiplier '
                                     '(mini-batches of tokens)')

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why, _batch_multiplier)

    def __init__(self, roles, runtime=None, kernels=None):
        super().__init__(roles, runtime=runtime, kernels=kernels)
        self._lazy_recount = True
        self._ws_step = None
        self._m_seen = _scalar_multiplier(self.topics)

    def _token_multiplier(self):
        """The multiplier of the token plate as the nodes carry it now (it has a setter)."""
        bad = _batch_multiplier(self.words, self.topics, self.p_word, self.p_topic)
        if bad:
            raise ValueError('fused LDA block: ' + bad)
        return _scalar_multiplier(self.topics)

    def invalidate(self, node):
        if node is self.words and node.observed and node._mask is True:
            self._layout_stale = True
            self._version += 1
            return
        if (node is self.words or node is self.topics) \
                and LDASVIPlan.match(self.nodes()) is not None \
                and _scalar_multiplier(self.topics) != self._m_seen:
            # the setter of plates_multiplier: the state stays, the next operation reads the factor
            self._m_seen = _scalar_multiplier(self.topics)
            self._version += 1
            return
        _delta.warn_state_discarded(self, node)
        self._ready = False
        self._version += 1
        if LDASVIPlan.match(self.nodes()) is None:
            from .generic import GenericPlan
            GenericPlan(self.nodes())

    def _token_indices(self):
        """Both index arrays with ONE device -> host read for all of the reference's checks."""
        torch = self.rt.torch
        index = getattr(self.index, 'device_value', None)
        doc, f1 = self._index_tensor(self.index.value if index is None else index)
        word, f2 = self._index_tensor(self.words._data)
        if self.n:
            no = torch.zeros((), dtype=torch.bool, device=doc.device)
            flags = torch.stack([f1 if f1 is not None else no, f2 if f2 is not None else no,
                                 (doc.min() < 0) | (doc.max() >= self.D),
                                 (word.min() < 0) | (word.max() >= self.V)]).cpu().numpy()
            if flags[0] or flags[1]:
                raise ValueError("Values must be integers")
            if flags[2] or flags[3]:
                raise ValueError("Invalid category index")
        return doc, word

    def _step_ws(self):
        if self._ws_step is None:
            k = self.kernels
            self._ws_step = self.rt.empty(max(
                k.dirichlet_step_ws(self.D, self.K, self.K, 1),
                k.dirichlet_step_ws(self.K, self.V, 1, self.K), 1))
        return self._ws_step

    def _step(self, node, mult, scale):
        k, ws = self.kernels, self._step_ws()
        D, V, K = self.D, self.V, self.K
        if node is self.p_topic:
            k.dirichlet_step(D, K, K, 1, self.prior_theta, self.Ndk, mult, scale, self.alpha_theta,
                             self.elog_theta, ws, self.scal[3:4])
        else:
            k.dirichlet_step(K, V, 1, K, self.prior_beta_t, self.Nvk, mult, scale,
                             self.alpha_beta_t, self.elog_beta_t, ws, self.scal[4:5])

    def _update_dirichlet(self, node):
        self._step(node, self._token_multiplier(), 1.0)

    def gradient_step(self, nodes, scale=1.0):
        """alpha <- alpha + scale * (prior + m * counts - alpha) for the Dirichlets among ``nodes``:
        the counts are those of the present ``topics`` state, so every optimum is taken before
        any node moves.  A Dirichlet that is still a point mass steps from its prior, as on the
        generic engine (its parameters there are the prior's until the first update)."""
        from ...nodes.node import Stochastic
        todo = []
        for node in nodes:
            if not isinstance(node, Stochastic) or node.observed:
                continue
            if node is self.topics:
                raise NotImplementedError(
                    'gradient step of %s: the fused LDA block keeps no responsibilities to step '
                    'from; update it (Q.update(%r)), or use VB(..., engine="generic")'
                    % (node.name, node.name))
            if node is self.p_topic or node is self.p_word:
                todo.append(node)
        if not todo:
            return
        self._materialize()
        m = self._token_multiplier()
        self.rt.sync_stream()
        for node in todo:
            key = 'p_topic' if node is self.p_topic else 'p_word'
            if key in self._delta and float(scale) != 1.0:
                (self.alpha_theta if node is self.p_topic else self.alpha_beta_t).copy_(
                    self.prior_theta if node is self.p_topic else self.prior_beta_t)
            _delta.updated(self._delta, self.roles, node)
            self._step(node, m, scale)
        self._version += 1
