"""The standard confound of network inference, and what external covariates do about it: two populations of neurons with NO coupling at all,
both driven by one common stimulus.  Fitted without the stimulus (n_covariates=0), the model can explain the common modulation only through
the population's own spike history, and the spike-and-slab prior puts edges between the populations; fitted with the stimulus as a covariate
(n_covariates=2, add_data(..., covariates=S)) the modulation goes to beta and the edges have less to explain.  Prints the posterior edge
probability between the populations (and within them) in both fits, and the posterior of beta beside the truth.  How far the edge
probability falls depends on the length of the chain and on the prior: an edge the data say nothing about stays near the prior's rho with
a weight near zero, so "no coupling" shows as a lower probability and small weights, not as a probability of zero.

The data are drawn here in NumPy (the truth has no coupling, so there is nothing to simulate serially): generate() of a model with
covariates is refused, and simulate() needs covariates= for the bins it simulates (examples/predictive_check_confound.py checks the
fitted model that way).

    python examples/stimulus_confound.py [N_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
np.random.seed(0)

from pyglm_amd.covariates import offset_host
from pyglm_amd.models import SparseBernoulliGLM
from pyglm_amd.utils.basis import cosine_basis

T = 20000     # time bins
N = 8         # neurons: population A = 0..3, population B = 4..7
B = 2         # basis functions
L = 50        # autoregressive window

t = np.arange(T)
S = np.column_stack([np.sin(2 * np.pi * t / 400.0), (t % 3000 >= 1500).astype(float)])      # a slow oscillation and an on/off stimulus
beta_true = np.zeros((N, 2))
beta_true[:4] = [1.5, 1.0]          # population A follows both
beta_true[4:] = [1.2, -1.0]         # population B follows the oscillation too, and is suppressed by the on/off stimulus
bias_true = -2.5
rng = np.random.default_rng(0)
Y = (rng.random((T, N)) < 1.0 / (1.0 + np.exp(-(bias_true + offset_host(S, beta_true))))).astype(float)

basis = cosine_basis(B=B, L=L) / L
kw = dict(S_w=3.0, mu_b=-2.0)
blind = SparseBernoulliGLM(N, basis=basis, regression_kwargs=kw)                       # knows nothing of the stimulus
aware = SparseBernoulliGLM(N, basis=basis, regression_kwargs=kw, n_covariates=2)       # beta_n ~ N(0, I), drawn after every sweep
blind.add_data(Y)
aware.add_data(Y, covariates=S)

N_samples = int(sys.argv[1]) if len(sys.argv) > 1 else 200
half = N_samples // 2
accs = [("without the stimulus", blind, blind.summarize(rates=False)), ("stimulus as covariates", aware, aware.summarize(rates=False))]
for itr in range(N_samples):
    for _, model, acc in accs:
        model.resample_model()
        if itr >= half:
            acc.collect()

across = np.zeros((N, N), dtype=bool)
across[:4, 4:] = across[4:, :4] = True
within = ~across & ~np.eye(N, dtype=bool)
print("mean rate per bin", Y.mean(axis=0).round(3))
print("true coupling: none.  Posterior edge probability, mean over the pairs:")
for label, model, acc in accs:
    P = acc.edge_prob
    print("  %-24s between the populations %.3f   within a population %.3f   log-likelihood %.1f"
          % (label, P[across].mean(), P[within].mean(), np.mean(acc.log_likelihoods)))
acc = accs[1][2]
print("beta, truth              ", beta_true.T.round(2).tolist())
print("beta, posterior mean     ", acc.covariate_mean.T.round(2).tolist())
print("beta, posterior sd       ", np.sqrt(acc.covariate_var).T.round(2).tolist())
