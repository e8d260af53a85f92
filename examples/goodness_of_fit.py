"""The flow of examples/synthetic.py ending in the time-rescaling goodness-of-fit test: simulate a network with self-inhibition, fit a
SparseBernoulliGLM on the first half of the recording and ask, per neuron, whether the fitted rates describe the recorded spike train -- on
the training half and on the held-out half (model.time_rescaling).  Under the model the intensity integrated between consecutive spikes is
Exp(1); the Kolmogorov-Smirnov distance of the rescaled intervals from that law is compared with the 95 % band 1.36 / sqrt(M), sample by
sample of the chain.  The list at the end names the neurons whose distance left the band in more than half of the samples.

    python examples/goodness_of_fit.py [N_samples]
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
train = test_model.time_rescaling(bins=64)                       # the recorded training half against the fitted rates
held = test_model.time_rescaling(bins=64, datas=[Y_test])        # the held-out half
first = None
for itr in range(N_samples):
    if itr == 0:
        first = test_model.rescaled_intervals(bins=64)           # the state before any sweep: the prior's draw, which describes nothing
    test_model.resample_model()
    if itr >= half:
        train.collect()
        held.collect()

from pyglm_amd.rescale import ks_binned
print("samples folded                     %d" % train.count)
print("before the first sweep: sqrt(M) KS ", (np.sqrt(first[0].sum(axis=1)) * ks_binned(first[0])).round(2), "(the 95 % line is 1.36)")
for label, gof in (("training", train), ("held-out", held)):
    print("%s  intervals per neuron              " % label, gof.intervals)
    print("%s  KS, posterior mean (sd)           " % label, gof.ks_mean.round(4), gof.ks_std.round(4))
    print("%s  95 %% band 1.36 / sqrt(M)          " % label, gof.band.round(4))
    print("%s  share of samples outside the band " % label, gof.exceed_fraction.round(2))
    print("%s  neurons the model does not describe:" % label, list(gof.failing()))
