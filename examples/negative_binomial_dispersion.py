"""Learning the negative-binomial dispersion xi: simulate over-dispersed counts from a network with a true xi, fit one model that learns
xi from a wrong start (xi_prior) and one that keeps xi fixed at that wrong value, and print the posterior of xi beside the truth and the
time-rescaling verdict of both fits.  xi decides how over-dispersed the fit may be: the fixed, wrong xi shows up as rescaled intervals that
leave the Kolmogorov-Smirnov band, the learned one does not.  The start is wrong by a factor of four, not of forty: given xi the bias is
pinned by the mean count xi e^b and given the bias xi is pinned in turn, so the chain walks that ridge in small steps, and a neuron whose
xi the first sweeps (weights still a draw from the prior) throw far up the ridge needs hundreds of sweeps to come back.

    python examples/negative_binomial_dispersion.py [N_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
np.random.seed(0)

from pyglm_amd.utils.basis import cosine_basis
from pyglm_amd.models import SparseNegativeBinomialGLM

T = 10000     # time bins
N = 4         # neurons
B = 1         # basis functions
L = 100       # autoregressive window
XI_TRUE = 0.5
XI_START = 2.0

basis = cosine_basis(B=B, L=L) / L

true_model = SparseNegativeBinomialGLM(N, basis=basis, regression_kwargs=dict(S_w=10.0, mu_b=-2., xi=XI_TRUE))
for n in range(N):
    true_model.regressions[n].a[n] = True
    true_model.regressions[n].W[n, :] = -2.0
    true_model.regressions[n].b[:] = 0.5
_, Y = true_model.generate(T=T, keep=False)

kw = dict(S_w=10.0, mu_b=-2., xi=XI_START)
learned = SparseNegativeBinomialGLM(N, basis=basis, regression_kwargs=dict(kw, xi_prior=(1.0, 1.0)))     # xi ~ Gamma(1, rate 1), resampled
fixed = SparseNegativeBinomialGLM(N, basis=basis, regression_kwargs=kw)                                # xi stays XI_START
learned.add_data(Y)
fixed.add_data(Y)

N_samples = int(sys.argv[1]) if len(sys.argv) > 1 else 200
half = N_samples // 2
acc = learned.summarize(rates=False)
gofs = [("xi learned", learned, learned.time_rescaling(bins=64)), ("xi fixed at %g" % XI_START, fixed, fixed.time_rescaling(bins=64))]
for itr in range(N_samples):
    for _, model, gof in gofs:
        model.resample_model()
        if itr >= half:
            gof.collect()
    if itr >= half:
        acc.collect()

print("mean count per bin                 ", Y.mean(axis=0).round(3), " variance / mean", (Y.var(axis=0) / Y.mean(axis=0)).round(2))
print("true xi                             %g   (the chain started at %g)" % (XI_TRUE, XI_START))
print("xi, posterior mean (sd)            ", acc.xi_mean.round(3), np.sqrt(acc.xi_var).round(3))
for label, model, gof in gofs:
    print("%-16s KS, posterior mean  " % label, gof.ks_mean.round(4), " band", gof.band.round(4))
    print("%-16s share outside the band" % label, gof.exceed_fraction.round(2), " neurons not described:", list(gof.failing()))
