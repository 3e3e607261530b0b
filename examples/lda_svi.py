"""Latent Dirichlet allocation by stochastic variational inference (doc/source/examples/lda.rst,
second half) at the corpus size of examples/lda.py: 2 million tokens, 20 000 documents, a
vocabulary of 20 000 words, 20 topics.  Every step observes a mini-batch of tokens that stands for
the whole corpus (``plates_multiplier``), updates the topic assignments of the batch and moves the
two Dirichlet tables along their natural gradients.  ``engine='fused'`` runs it on the fused block:
one token pass over the batch and one step kernel per table; the batches stay on the device.

    python examples/lda_svi.py [tokens] [batch] [steps]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayespy_amd import nodes                                                          # noqa: E402
from bayespy_amd.inference import VB                                                   # noqa: E402
from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments             # noqa: E402

n_words = int(sys.argv[1]) if len(sys.argv) > 1 else 2000000
subset_size = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
n_steps = int(sys.argv[3]) if len(sys.argv) > 3 else 50
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
document_indices = nodes.Constant(CategoricalMoments(n_documents), word_documents[:subset_size],
                                  name='document_indices')
topics = nodes.Categorical(nodes.Gate(document_indices, p_topic), plates=(subset_size,),
                           plates_multiplier=(n_words / subset_size,), name='topics')
words = nodes.Categorical(nodes.Gate(topics, p_word), name='words')
words.observe(corpus[:subset_size])
p_topic.initialize_from_random()
p_word.initialize_from_random()

Q = VB(words, topics, p_word, p_topic, document_indices, engine='fused')
print('plan:', type(Q.plans[0]).__name__)
Q.ignore_bound_checks = True

# the corpus lives on the device; a batch is a gather there
corpus_d = torch.from_numpy(corpus).cuda()
documents_d = torch.from_numpy(word_documents).cuda()
delay, forgetting_rate = 1, 0.7
for n in range(n_steps):
    subset = torch.from_numpy(rs.choice(n_words, subset_size)).cuda()
    Q['words'].observe(corpus_d[subset])
    Q['document_indices'].set_value(documents_d[subset])
    Q.update('topics', verbose=(n % 10 == 0))
    Q.gradient_step('p_topic', 'p_word', scale=(n + delay) ** (-forgetting_rate))
logp = Q['p_word'].get_moments()[0]
print('most probable words of the first topics:')
for k in range(5):
    print('  topic %d:' % k, np.argsort(-logp[k])[:8])
