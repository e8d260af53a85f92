"""Checking a model of a confounded recording: the two-population stimulus problem of examples/stimulus_confound.py -- NO coupling, both
populations driven by one recorded stimulus -- fitted with the stimulus as covariates, and then checked by posterior predictive simulation
under that same stimulus: predictive_check(covariates="data", lags=K).  The lagged cross-correlogram is the statistic that sees coupling; a
model whose covariates explain the common modulation reproduces the data's between-population correlogram, so its two-sided p-values for
those pairs are not extreme.  The same check of the fit WITHOUT the stimulus has nothing but the history filters to make the populations
co-vary with.  Prints, per fit, the rate and correlogram p-values of the between-population pairs.

    python examples/predictive_check_confound.py [N_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
np.random.seed(0)

from pyglm_amd.covariates import offset_host
from pyglm_amd.models import SparseBernoulliGLM
from pyglm_amd.utils.basis import cosine_basis

T, N, B, L, LAGS = 20000, 8, 2, 50, 5          # population A = neurons 0..3, population B = 4..7

t = np.arange(T)
S = np.column_stack([np.sin(2 * np.pi * t / 400.0), (t % 3000 >= 1500).astype(float)])
beta_true = np.zeros((N, 2))
beta_true[:4] = [1.5, 1.0]
beta_true[4:] = [1.2, -1.0]
rng = np.random.default_rng(0)
Y = (rng.random((T, N)) < 1.0 / (1.0 + np.exp(-(-2.5 + offset_host(S, beta_true))))).astype(float)

basis = cosine_basis(B=B, L=L) / L
kw = dict(S_w=3.0, mu_b=-2.0)
blind = SparseBernoulliGLM(N, basis=basis, regression_kwargs=kw)
aware = SparseBernoulliGLM(N, basis=basis, regression_kwargs=kw, n_covariates=2)
blind.add_data(Y)
aware.add_data(Y, covariates=S)
checks = [("without the stimulus", blind, blind.predictive_check(replicates=4, seed=1, lags=LAGS)),
          ("stimulus as covariates", aware, aware.predictive_check(replicates=4, seed=1, lags=LAGS, covariates="data"))]

N_samples = int(sys.argv[1]) if len(sys.argv) > 1 else 100
for itr in range(N_samples):
    for _, model, ppc in checks:
        model.resample_model()
        if itr >= N_samples // 2:
            ppc.collect()

across = np.zeros((N, N), dtype=bool)
across[:4, 4:] = across[4:, :4] = True
print("observed between-population correlogram at lags 0..%d: %s" % (LAGS - 1, checks[0][2].observed["xcorr"][:, across].mean(axis=1).round(4).tolist()))
for label, model, ppc in checks:
    p = ppc.pvalue("xcorr")[:, across]           # (LAGS, 32 ordered pairs), two-sided
    print("%-24s replicated mean %s" % (label, ppc.xcorr_mean[:, across].mean(axis=1).round(4).tolist()))
    print("%-24s correlogram p-values of the between-population pairs: median %.3f, smallest %.3f, below 0.05: %d of %d; rate p-values %s"
          % ("", np.median(p), p.min(), int((p < 0.05).sum()), p.size, ppc.pvalue("rate").round(2).tolist()))
