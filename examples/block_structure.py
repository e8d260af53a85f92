"""Who connects to whom, and in which groups?  A planted two-population network -- dense excitation within a population, sparse connections
between them -- is simulated and fitted twice: with SBMSparseNetwork, which learns a partition of the neurons and the block-to-block
connection probabilities, and with NIWSparseNetwork(rho=0.5), which fixes the connection probability by hand.  Printed: the adjusted Rand
index of the consensus partition against the planted one, the posterior mean of rho within and between the populations under the block
model (the fixed prior says 0.5 everywhere), and the error of the posterior edge probabilities of both fits.

    python examples/block_structure.py [N_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
np.random.seed(0)

from pyglm_amd.models import SparseBernoulliGLM
from pyglm_amd.networks import NIWSparseNetwork, SBMSparseNetwork
from pyglm_amd.sbm import adjusted_rand
from pyglm_amd.utils.basis import cosine_basis

T = 20000   # time bins
N = 16      # neurons: two populations of 8
B = 1       # basis functions
L = 20      # autoregressive window
P_IN, P_OUT = 0.7, 0.05

basis = cosine_basis(B=B, L=L) / L
truth = np.repeat([0, 1], N // 2)
rng = np.random.default_rng(0)
A_true = rng.random((N, N)) < np.where(truth[:, None] == truth[None, :], P_IN, P_OUT)
np.fill_diagonal(A_true, True)

true_model = SparseBernoulliGLM(N, basis=basis, regression_kwargs=dict(S_w=10.0, mu_b=-2.))
for n in range(N):
    reg = true_model.regressions[n]
    reg.a[:] = A_true[n]
    reg.W[:, 0] = np.where(np.arange(N) == n, -2.0, 1.5) * A_true[n]
_, Y = true_model.generate(T=T, keep=False)

N_samples = int(sys.argv[1]) if len(sys.argv) > 1 else 100
burn = N_samples // 2
fits = {}
for name, network in (("SBM", SBMSparseNetwork(N, B, K=4)), ("NIW rho = 0.5", NIWSparseNetwork(N, B, rho=0.5))):
    model = SparseBernoulliGLM(N, basis=basis, network=network, regression_kwargs=dict(S_w=10.0, mu_b=-2.), seed=1)
    model.add_data(Y)
    summary = model.summarize(rates=False)
    blocks = model.block_structure() if name == "SBM" else None
    for itr in range(burn + N_samples):
        model.resample_model()
        if itr >= burn:
            summary.collect()
            if blocks is not None:
                blocks.collect()
    fits[name] = (summary.edge_prob, blocks)

same = truth[:, None] == truth[None, :]
off = ~np.eye(N, dtype=bool)
blocks = fits["SBM"][1]
consensus = blocks.consensus()
print("planted partition  ", truth)
print("consensus partition", consensus, " adjusted Rand index %.3f" % adjusted_rand(consensus, truth))
print("occupied blocks over the kept sweeps: %s" % np.bincount(blocks.occupied))
print("posterior mean of rho   within populations %.3f (planted %.2f)   between %.3f (planted %.2f)   NIW: 0.5 everywhere"
      % (blocks.rho_mean[same & off].mean(), P_IN, blocks.rho_mean[~same].mean(), P_OUT))
for name, (edge_prob, _) in fits.items():
    print("%-14s mean |P(edge) - truth| off the diagonal  %.3f" % (name, np.abs(edge_prob - A_true)[off].mean()))
