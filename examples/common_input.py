"""The confound nobody recorded, and what latent factors do about it: the two uncoupled populations of examples/stimulus_confound.py with
the stimulus WITHHELD.  Both populations follow one common drive; fitted with n_latents=0 the model can explain the common modulation
only through the population's own spike history; fitted with n_latents=1 it infers a latent factor x_t shared by all neurons together
with the network.  Prints, for two drives, the posterior edge probability between the populations (and within them) in both fits and
the correlation of the posterior-mean common_input() with the true drive, neuron by neuron.  X and the loadings alone are defined only up
to sign (rotation, with more factors); their product, the common input, is what can be compared with the truth.

    slow   the stimulus of stimulus_confound.py (a 400-bin oscillation and an on/off step).  The prior on x_t is independent over time, so
           the latent follows a drive from the spikes of ONE bin, while the 50-bin history filters average a population's spikes over
           their window -- for a drive this slow they are the better estimator, the chain settles with the drive explained by edges
           WITHIN a population, and the latent stays near zero (correlation with the truth below 0.1, in 200 sweeps and in 600).  The third
           fit gives x_t the temporal prior this case needs, latent_ar=phi: an AR(1) process whose phi is the lag-1 autocorrelation of
           the stimulus's own drive (printed; 0.99965), drawn jointly over all bins (pyglm_amd/latents.py).  The
           latent then follows the drive (correlation 0.43 to 0.46 per neuron) -- but in 200 sweeps it does not take the drive off the
           history filters, which the chain fills first: the edges within a population stay (0.975) and those between rise (0.852).
    fast   a drive that changes within three bins, which no history filter can follow: the latent recovers it (correlation 0.8, the
           loadings' |C_n|^2 at the drive's true variance, a log-likelihood far above the fit without latents).  The edge probabilities
           stay near the prior's 0.5 in both fits: what the history cannot follow it cannot mistake for coupling either.

    python examples/common_input.py [N_samples]
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
rng = np.random.default_rng(0)
S = np.column_stack([np.sin(2 * np.pi * t / 400.0), (t % 3000 >= 1500).astype(float)])      # the stimulus of stimulus_confound.py: never shown to a model
beta_true = np.zeros((N, 2))
beta_true[:4] = [1.5, 1.0]
beta_true[4:] = [1.2, -1.0]
g = np.convolve(rng.standard_normal(T + 4), np.ones(3) / np.sqrt(3.0), mode="valid")[:T]      # unit variance, correlated over 3 bins
drives = [("slow", -2.5, offset_host(S, beta_true)), ("fast", -2.0, g[:, None] * np.r_[np.full(4, 1.5), np.full(4, -1.5)][None, :])]

basis = cosine_basis(B=B, L=L) / L
kw = dict(S_w=3.0, mu_b=-2.0)
N_samples = int(sys.argv[1]) if len(sys.argv) > 1 else 200
half = N_samples // 2
across = np.zeros((N, N), dtype=bool)
across[:4, 4:] = across[4:, :4] = True
within = ~across & ~np.eye(N, dtype=bool)

for name, bias_true, drive in drives:                   # drive (T, N): what the unrecorded input gives every neuron
    Y = (rng.random((T, N)) < 1.0 / (1.0 + np.exp(-(bias_true + drive)))).astype(float)
    blind = SparseBernoulliGLM(N, basis=basis, regression_kwargs=kw)
    latent = SparseBernoulliGLM(N, basis=basis, regression_kwargs=kw, n_latents=1)      # x_t ~ N(0, 1), loadings C_n ~ N(0, 1)
    fits = [("n_latents=0", blind), ("n_latents=1", latent)]
    if name == "slow":                                  # x_t = phi x_{t-1} + sqrt(1 - phi^2) eps_t: phi from the drive's own lag-1 autocorrelation
        d0 = drive[:, 0] - drive[:, 0].mean()
        phi = float(d0[1:].dot(d0[:-1]) / d0.dot(d0))
        print("slow drive: lag-1 autocorrelation of the drive %.5f -> latent_ar=%.5f" % (phi, phi))
        fits.append(("latent_ar=%.4f" % phi, SparseBernoulliGLM(N, basis=basis, regression_kwargs=kw, n_latents=1, latent_ar=phi)))
    for _, model in fits:
        model.add_data(Y)
    accs = [(label, model, model.summarize(rates=False)) for label, model in fits]
    commons, kept = [0.0] * len(fits), 0
    for itr in range(N_samples):
        for _, model, acc in accs:
            model.resample_model()
            if itr >= half:
                acc.collect()
        if itr >= half:
            commons = [c + (model.common_input() if model.Q else 0.0) for c, (_, model) in zip(commons, fits)]
            kept += 1
    print("%s drive: mean rate per bin %s" % (name, Y.mean(axis=0).round(3)))
    print("  true coupling: none.  Posterior edge probability, mean over the pairs:")
    for label, model, acc in accs:
        P = acc.edge_prob
        print("    %-12s between the populations %.3f   within a population %.3f   log-likelihood %.1f"
              % (label, P[across].mean(), P[within].mean(), np.mean(acc.log_likelihoods)))
    centred = drive - drive.mean(axis=0)                # (the drive's mean is the bias's to explain)
    for (label, model, acc), common in zip(accs, commons):
        if not model.Q:
            continue
        print("  %s: correlation of the posterior-mean common input with the true drive, per neuron:" % label,
              [round(float(np.corrcoef(common[:, n] / kept, centred[:, n])[0, 1]), 2) for n in range(N)])
        print("  %s: variance of the common drive per neuron, posterior mean of |C_n|^2:" % label, acc.common_input_var_mean.round(2).tolist(),
              " true:", drive.var(axis=0).round(2).tolist())
