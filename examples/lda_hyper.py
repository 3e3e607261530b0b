"""Latent Dirichlet allocation (doc/source/examples/lda.rst) with both concentrations learnt: the
corpus of examples/lda.py -- 2 million tokens, 20 000 documents, a vocabulary of 20 000 words -- with
a ``DirichletConcentration`` parent on the topic proportions and on the word distributions.
``engine='fused+topics+hyper'`` runs it on the fused block (up to 1024 topics); the generic engine
would hold tokens x topics and tokens x vocabulary arrays and cannot run this corpus.

    python examples/lda_hyper.py [tokens [topics]]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayespy_amd import nodes                                                          # noqa: E402
from bayespy_amd.inference import VB                                                   # noqa: E402
from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments             # noqa: E402

n_words = int(sys.argv[1]) if len(sys.argv) > 1 else 2000000
n_topics = int(sys.argv[2]) if len(sys.argv) > 2 else 20
n_documents, n_vocabulary, n_true = 20000, 20000, 20

# an artificial corpus drawn from the model with a few true topics
rs = np.random.RandomState(0)
true_topic = rs.dirichlet(0.1 * np.ones(n_true), size=n_documents)
true_word = rs.dirichlet(0.05 * np.ones(n_vocabulary), size=n_true)
word_documents = rs.randint(n_documents, size=n_words)
z = (true_topic[word_documents].cumsum(-1) > rs.rand(n_words, 1)).argmax(-1)
cdf = true_word.cumsum(-1)
corpus = np.array([np.searchsorted(cdf[k], u) for k, u in zip(z, rs.rand(n_words))])
corpus = np.minimum(corpus, n_vocabulary - 1)

conc_topic = nodes.DirichletConcentration(n_topics, name='conc_topic')
conc_word = nodes.DirichletConcentration(n_vocabulary, name='conc_word')
p_topic = nodes.Dirichlet(conc_topic, plates=(n_documents,), name='p_topic')
p_word = nodes.Dirichlet(conc_word, plates=(n_topics,), name='p_word')
document_indices = nodes.Constant(CategoricalMoments(n_documents), word_documents,
                                  name='document_indices')
topics = nodes.Categorical(nodes.Gate(document_indices, p_topic), plates=(len(corpus),),
                           name='topics')
words = nodes.Categorical(nodes.Gate(topics, p_word), name='words')
words.observe(corpus)
p_topic.initialize_from_random()
p_word.initialize_from_random()

Q = VB(words, topics, p_word, p_topic, conc_topic, conc_word, document_indices,
       engine='fused+topics+hyper')
print('plan:', type(Q.plans[0]).__name__)
Q.update(repeat=30)
a, b = conc_topic.get_moments()[0], conc_word.get_moments()[0]
print('learnt concentration of the topic proportions: sum %.3f, largest %.4f' % (a.sum(), a.max()))
print('learnt concentration of the word distributions: sum %.3f, largest %.5f' % (b.sum(), b.max()))
logp = Q['p_word'].get_moments()[0]
used = np.argsort(-Q.plans[0].Ndk.sum(0).cpu().numpy())[:5]
print('most probable words of the five most used topics:')
for k in used:
    print('  topic %d:' % k, np.argsort(-logp[k])[:8])
