"""Latent Dirichlet allocation (doc/source/examples/lda.rst) at a size the reference cannot hold:
2 million tokens, 20 000 documents, a vocabulary of 20 000 words, 20 topics.  The reference forms
tokens x vocabulary and tokens x documents one-hot arrays of doubles (320 GB each here); the fused
block keeps the tokens as sorted int32 indices and the two count tables.

    python examples/lda.py [tokens]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayespy_amd import nodes                                                          # noqa: E402
from bayespy_amd.inference import VB                                                   # noqa: E402
from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments             # noqa: E402

n_words = int(sys.argv[1]) if len(sys.argv) > 1 else 2000000
n_documents, n_vocabulary, n_topics = 20000, 20000, 20

# an artificial corpus drawn from the model itself
rs = np.random.RandomState(0)
true_topic = rs.dirichlet(0.1 * np.ones(n_topics), size=n_documents)
true_word = rs.dirichlet(0.05 * np.ones(n_vocabulary), size=n_topics)
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

Q = VB(words, topics, p_word, p_topic, document_indices)
print('plan:', type(Q.plans[0]).__name__)
Q.update(repeat=30)
logp = Q['p_word'].get_moments()[0]
print('most probable words of the first topics:')
for k in range(5):
    print('  topic %d:' % k, np.argsort(-logp[k])[:8])
