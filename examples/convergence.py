"""How much chain is there?  The flow of examples/synthetic.py run as TWO chains from different seeds, each with chain diagnostics
(model.diagnose): after every 32 kept sweeps the smallest effective sample size per read-out, the largest R-hat over the edges, and the
median gain of the Rao-Blackwell edge probabilities over the 0/1 averages are printed; at the end both estimators of the edge probabilities
with their Monte Carlo standard errors.

    python examples/convergence.py [N_samples]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
np.random.seed(0)

from pyglm_amd.diagnostics import rhat
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

chains = []
for seed in (1, 2):
    model = SparseBernoulliGLM(N, basis=basis, regression_kwargs=dict(S_w=10.0, mu_b=-2.), seed=seed)
    model.add_data(Y)
    chains.append((model, model.diagnose(levels=8)))

N_samples = int(sys.argv[1]) if len(sys.argv) > 1 else 128
burn = N_samples // 4
for itr in range(burn + N_samples):
    for model, diag in chains:
        model.resample_model()
        if itr >= burn:
            diag.collect()
    kept = itr + 1 - burn
    if kept > 0 and kept % 32 == 0:
        diag = chains[0][1]
        worst = diag.min_ess()
        with np.errstate(invalid="ignore"):
            r_edge = rhat([d for _, d in chains], "edge")
            gain = diag.rb_gain
        print("kept %4d  level %d  min ESS  %s" % (kept, diag.level(), "  ".join("%s %.1f" % (k, v[0]) for k, v in worst.items())))
        print("           max R-hat over edges %.3f   R-hat of the log likelihood %.3f   median RB gain %.1f"
              % (np.nanmax(r_edge) if np.any(np.isfinite(r_edge)) else np.nan, rhat([d for _, d in chains], "ll"),
                 np.nanmedian(gain) if np.any(np.isfinite(gain)) else np.nan))

diag = chains[0][1]
print("true adjacency\n", true_model.adjacency.astype(int))
print("edge probabilities (0/1 average)\n", diag.edge_prob.round(3), "\n  MCSE\n", diag.mcse("edge").round(3))
print("edge probabilities (Rao-Blackwell)\n", diag.edge_prob_rb.round(3), "\n  MCSE\n", diag.mcse("edge_rb").round(3))
print("effective sample size of the biases", diag.ess("bias").round(1), "of", diag.count)
