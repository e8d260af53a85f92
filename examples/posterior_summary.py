"""The flow of examples/synthetic.py with the posterior accumulator instead of stacked samples: simulate a network with self-inhibition,
fit a SparseBernoulliGLM on the first half of the recording, keep running posterior summaries on the device (model.summarize) and print the
edge probabilities against the true adjacency, the posterior rates and the predictive density (lppd, WAIC) of the held-out half.

    python examples/posterior_summary.py [N_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
np.random.seed(0)

from pyglm_amd.utils.basis import cosine_basis
from pyglm_amd.models import SparseBernoulliGLM

T = 10000   # time bins
N = 4       # neurons
B = 1       # basis functions
L = 100     # autoregressive window

basis = cosine_basis(B=B, L=L) / L

true_model = SparseBernoulliGLM(N, basis=basis, regression_kwargs=dict(S_w=10.0, mu_b=-2.))
for n in range(N):
    true_model.regressions[n].a[n] = True
    true_model.regressions[n].W[n, :] = -2.0
_, Y = true_model.generate(T=T, keep=False)
Y_train, Y_test = Y[:T // 2], Y[T // 2:]

test_model = SparseBernoulliGLM(N, basis=basis, regression_kwargs=dict(S_w=10.0, mu_b=-2.))
test_model.add_data(Y_train)

N_samples = int(sys.argv[1]) if len(sys.argv) > 1 else 100
half = N_samples // 2
train = test_model.summarize(rates=True, pointwise=True)                      # moments of the state and of the rates on the training half
held = test_model.summarize(rates=False, pointwise=True, datas=[Y_test])      # predictive density of the held-out half
for itr in range(N_samples):
    test_model.resample_model()
    if itr >= half:
        ll = train.collect()            # = test_model.log_likelihood(), and the sample is folded into the running moments
        held.collect()
        if itr % 10 == 0:
            print("iteration %3d  log likelihood %.1f" % (itr, ll))

print("samples folded           %d" % train.count)
print("mean log likelihood      %.1f" % np.mean(train.log_likelihoods))
print("true adjacency\n", true_model.adjacency.astype(int))
print("edge probabilities\n", train.edge_prob.round(2))
print("posterior mean weights (sd)\n", train.weight_mean[:, :, 0].round(2), "\n", np.sqrt(train.weight_var[:, :, 0]).round(2))
print("posterior mean biases    ", train.bias_mean.round(2), "sd", np.sqrt(train.bias_var).round(2))
print("mean rate per neuron     ", train.rate_mean[0].mean(axis=0).round(4), "spikes per bin", Y_train.mean(axis=0).round(4))
w = train.waic()
print("training  lppd %.1f  p_waic %.1f  WAIC %.1f" % (w["lppd"], w["p_waic"], w["waic"]))
print("held-out  lppd %.1f  (mean of single-sample log likelihoods %.1f)" % (held.lppd()["total"], np.mean(held.log_likelihoods)))
