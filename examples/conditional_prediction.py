"""The flow of examples/synthetic.py ending in population-conditioned prediction: simulate a coupled network, fit a SparseBernoulliGLM, and
ask what the fit says two of the neurons do GIVEN the recorded activity of the others (model.conditional_check: the two are simulated from
the chain's states while every other neuron is clamped to the recording).  Their conditional log score -- the log predictive probability of
their recorded spikes -- is printed beside the score of the unconditional rate that model.predictive_check simulates: the difference is what
the coupling is worth in the time course.

    python examples/conditional_prediction.py [N_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
np.random.seed(0)

from pyglm_amd.utils.basis import cosine_basis
from pyglm_amd.models import SparseBernoulliGLM

T = 10000   # time bins
N = 6       # neurons
B = 1       # basis functions
L = 100     # autoregressive window
held_out = [0, 1]

basis = cosine_basis(B=B, L=L) / L

true_model = SparseBernoulliGLM(N, basis=basis, regression_kwargs=dict(S_w=10.0, mu_b=-2.))
for n in range(N):
    true_model.regressions[n].a[...] = False
    true_model.regressions[n].W[...] = 0.0                     # (generate() reads the stored W, edge or not)
    true_model.regressions[n].a[n] = True
    true_model.regressions[n].W[n, :] = -2.0
for n, (m, w) in zip(held_out, [(2, 20.0), (3, -20.0)]):         # each held-out neuron listens to one of the others
    true_model.regressions[n].a[m] = True
    true_model.regressions[n].W[m, :] = w
_, Y = true_model.generate(T=T, keep=False)

test_model = SparseBernoulliGLM(N, basis=basis, regression_kwargs=dict(S_w=10.0, mu_b=-2.))
test_model.add_data(Y)

N_samples = int(sys.argv[1]) if len(sys.argv) > 1 else 100
half = N_samples // 2
cond = test_model.conditional_check(held_out, replicates=8, seed=0)
ppc = test_model.predictive_check(replicates=8, seed=0)
for itr in range(N_samples):
    test_model.resample_model()
    if itr >= half:
        cond.collect()
        ppc.collect()

score = cond.log_score()
y = Y[:, held_out]
p = np.clip(ppc.rates.mean(axis=0)[held_out], 1e-12, 1 - 1e-12)       # the unconditional rate of the same chain: one number per neuron
flat = (y * np.log(p) + (1 - y) * np.log1p(-p)).sum(axis=0)
print("conditional replicates folded      %d" % cond.count)
print("held-out neurons                   ", held_out)
print("recorded spikes                    ", y.sum(axis=0).astype(int))
print("conditional log score              ", score["per_neuron"].round(1))
print("log score of the unconditional rate", flat.round(1))
print("gain per spike (nats)              ", ((score["per_neuron"] - flat) / np.maximum(y.sum(axis=0), 1)).round(3))
print("conditional rate, mean over bins   ", cond.rate_mean.mean(axis=0).round(4), " recorded", y.mean(axis=0).round(4))
