"""The flow of examples/synthetic.py ending in a posterior predictive check: simulate a network with self-inhibition, fit a
SparseBernoulliGLM to the recording, and after every kept sweep simulate fresh replicates of the recording from the current state
(model.predictive_check -> model.simulate, on the device when there is one).  Prints the replicated firing rates and Fano factors against the
observed ones, the two-sided posterior predictive p-values per neuron -- those of the cross-correlogram and of the inter-spike-interval
density and its coefficient of variation among them --, and a forecast that continues the recording.

    python examples/posterior_predictive.py [N_samples]
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
Y = true_model.simulate(T, seed=1).Y[0]          # one trajectory of the true model, from the package's own random stream

test_model = SparseBernoulliGLM(N, basis=basis, regression_kwargs=dict(S_w=10.0, mu_b=-2.))
test_model.add_data(Y)

N_samples = int(sys.argv[1]) if len(sys.argv) > 1 else 100
half = N_samples // 2
# lags: the cross-correlogram, the statistic that sees the coupling; isi: the interval density and its CV, which see the self-inhibition
ppc = test_model.predictive_check(replicates=8, seed=2, lags=10, isi=32)
for itr in range(N_samples):
    test_model.resample_model()
    if itr >= half:
        ppc.collect()                             # 8 fresh replicates of T bins from this sample of the posterior
        if itr % 10 == 0:
            print("iteration %3d  log likelihood %.1f" % (itr, test_model.log_likelihood()))

lo, mid, hi = ppc.rate_quantiles([0.05, 0.5, 0.95])
print("replicates               %d" % ppc.rates.shape[0])
print("observed rate            ", ppc.observed["rate"].round(4))
print("replicated rate 5/50/95 %", lo.round(4), mid.round(4), hi.round(4))
print("p-value (rate)           ", ppc.pvalue("rate").round(3))
print("observed Fano factor     ", ppc.observed["fano"].round(3))
print("replicated Fano 50 %     ", ppc.fano_quantiles(0.5).round(3))
print("p-value (Fano)           ", ppc.pvalue("fano").round(3))
p_xc = ppc.pvalue("xcorr")                        # (lags, N, N): neuron i leading neuron j by l bins
print("cross-correlogram: fraction of (lag, pair) cells with p < 0.05  %.3f" % np.mean(p_xc[~np.isnan(p_xc)] < 0.05))
p_isi = ppc.pvalue("isi")                         # (N, bins): the share of a neuron's intervals that last d bins (the last bin: 32 or more)
print("interval density: fraction of (neuron, length) cells with p < 0.05   %.3f" % np.mean(p_isi[~np.isnan(p_isi)] < 0.05))
print("observed CV of the intervals", ppc.observed["cv"].round(3))
print("replicated CV 50 %          ", ppc.cv_quantiles(0.5).round(3))
print("p-value (CV)                ", ppc.pvalue("cv").round(3))
forecast = test_model.simulate(500, replicates=16, seed=3, history=Y[-L:], t0=T)
print("forecast of the next 500 bins, mean rate over 16 replicates", forecast.rate().mean(axis=0).round(4))
