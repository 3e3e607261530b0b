"""Latent Dirichlet allocation (doc/source/examples/lda.rst) with more topics than one lane group
holds: the corpus of examples/lda.py -- 2 million tokens, 20 000 documents, a vocabulary of 20 000
words -- with 256 topics.  ``engine='fused+topics'`` runs it on the wide-topic form of the fused
block (65 to 1024 topics); a tokens x topics array of doubles would be 4 GB here and is never formed.

    python examples/lda_wide.py [tokens [topics]]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayespy_amd import nodes                                                          # noqa: E402
from bayespy_amd.inference import VB                                                   # noqa: E402
from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments             # noqa: E402

n_words = int(sys.argv[1]) if len(sys.argv) > 1 else 2000000
n_topics = int(sys.argv[2]) if len(sys.argv) > 2 else 256
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

p_topic = nodes.Dirichlet(np.ones(n_topics), plates=(n_documents,), name='p_topic')
p_word = nodes.Dirichlet(np.ones(n_vocabulary), plates=(n_topics,), name='p_word')
document_indices = nodes.Constant(CategoricalMoments(n_documents), word_documents,
                                  name='document_indices')
topics = nodes.Categorical(nodes.Gate(document_indices, p_topic), plates=(len(corpus),),
                           name='topics')
words = nodes.Categorical(nodes.Gate(topics, p_word), name='words')
words.observe(corpus)
p_topic.initialize_from_random()
p_word.initialize_from_random()

Q = VB(words, topics, p_word, p_topic, document_indices, engine='fused+topics')
print('plan:', type(Q.plans[0]).__name__)
Q.update(repeat=30)
logp = Q['p_word'].get_moments()[0]
used = np.argsort(-Q.plans[0].Ndk.sum(0).cpu().numpy())[:5]
print('most probable words of the five most used topics:')
for k in used:
    print('  topic %d:' % k, np.argsort(-logp[k])[:8])
