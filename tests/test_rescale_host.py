"""The time-rescaling test on its host path (pyglm_amd/rescale.py: rescale_host, ks_binned, TimeRescaling) -- the specification of
pgl_rescale_fold / pgl_rescale_ks -- against a brute-force loop over the intervals, and its statistical sense on simulated data.  CPU only:
models on engine_factory=OracleEngine, and a small NumPy engine for the mixed model of the statistical case.

Tolerances follow from fp64 rounding: a z is compared at rtol = 1e-13 (the sum of an interval is formed by NumPy's pairwise reduction, by a
plain loop in the brute force: len * 2^-53 relative, len <= 600), the sums of z at rtol = 1e-12."""
import functools

import numpy as np
import pytest

from oracle import pyglm_oracle as orc
from pyglm_amd import models as M
from pyglm_amd import rescale, simulate
from pyglm_amd.models import NonlinearAutoregressiveModel
from pyglm_amd.regression import SparseBernoulliRegression, SparseGaussianRegression, SparseNegativeBinomialRegression
from pyglm_amd.utils.basis import cosine_basis
from tests._oracle_engine import OracleEngine


def brute(psi, Y, par, D, seed, draw, neuron0, elem0):
    """the definition, one interval at a time: -> (hist, [z per column])"""
    T, N = psi.shape
    hist, zs = np.zeros((N, D), dtype=np.int64), []
    for j in range(N):
        w = simulate.philox_words(seed, 3, draw, elem0, neuron0 + j, T)
        r = simulate._unit(w[:, 0], w[:, 1])
        q = [par[j] * np.log1p(np.exp(psi[t, j])) for t in range(T)]
        ev = [t for t in range(T) if Y[t, j] > 0]
        z = []
        for s, e in zip(ev[:-1], ev[1:]):
            xi = 0.0
            for t in range(s + 1, e):
                xi += q[t]
            xi += -np.log1p(-r[e] * (-np.expm1(-q[e])))
            z.append(-np.expm1(-xi))
            hist[j, min(D - 1, int(z[-1] * D))] += 1
        zs.append(np.array(z))
    return hist, zs


def test_rescale_host_is_the_definition():
    rng = np.random.default_rng(11)
    T, N, D = 400, 7, 16
    psi = rng.uniform(-5.0, 1.0, size=(T, N))
    Y = (rng.random((T, N)) < np.array([0.0, 0.003, 0.05, 0.3, 1.0, 0.1, 0.1])).astype(float)
    Y[:, 5] = rng.choice([0.0, 1.0, 2.0, 5.0, -1.0, np.nan], size=T)
    Y[:, 1] = 0.0
    Y[57, 1] = 1.0                                              # one event: no interval
    par = np.array([1.0, 1.0, 1.0, 2.5, 1.0, 10.0, 2.5])
    hist, zsum, zs = rescale.rescale_host(psi, Y, par, D, 5, 3, 40, 1000)
    bh, bz = brute(psi, Y, par, D, 5, 3, 40, 1000)
    assert np.array_equal(hist, bh) and hist.dtype == np.int64
    assert list(hist.sum(axis=1)[:2]) == [0, 0] and hist[4].sum() == T - 1 and hist[2].sum() > 5
    for j in range(N):
        np.testing.assert_allclose(zs[j], bz[j], rtol=1e-13, atol=0)
        np.testing.assert_allclose(zsum[j], [bz[j].sum(), (bz[j] ** 2).sum()], rtol=1e-12, atol=0)
    # another draw, another neuron offset, another data-set offset: other uniforms, the same number of intervals
    for other in (dict(draw=4), dict(neuron0=41), dict(elem0=1001), dict(seed=6)):
        kw = dict(dict(seed=5, draw=3, neuron0=40, elem0=1000), **other)
        h2 = rescale.rescale_host(psi, Y, par, D, **kw)[0]
        assert np.array_equal(h2.sum(axis=1), hist.sum(axis=1)) and not np.array_equal(h2, hist)
    # a scalar par is every neuron's
    assert np.array_equal(rescale.rescale_host(psi, Y, 1.0, D, 5, 3, 40, 1000)[0][:3], hist[:3])


def test_the_uniforms_are_call_draw_of_purpose_3():
    elems = np.array([0, 1, 17, 399])
    for seed, draw, stream, elem0 in ((5, 0, 0, 0), (2 ** 40 + 3, 7, 2 ** 33 + 5, 123456), (1, 2 ** 24 + 1, 9, 2 ** 32 - 100)):
        w = simulate.philox_words(seed, rescale.PURPOSE_RESCALE, draw, elem0, stream, 400)
        u = rescale.event_uniforms(seed, draw, stream, elem0 + elems)
        assert np.array_equal(u, simulate._unit(w[elems, 0], w[elems, 1])) and np.all((u > 0) & (u < 1))
        w2 = simulate.philox_words(seed, simulate.PURPOSE_SIM, draw, elem0, stream, 400)
        assert not np.array_equal(w, w2)
    assert rescale.PURPOSE_RESCALE == 3


def test_ks_binned():
    h = np.array([[5, 5, 5, 5], [20, 0, 0, 0], [0, 0, 0, 20], [0, 0, 0, 0], [1, 2, 3, 4]])
    ks = rescale.ks_binned(h)
    assert ks[0] == 0.0 and ks[1] == 0.75 and ks[2] == 0.75 and np.isnan(ks[3])
    # |C_d D - d M| / (M D), d = 1 .. 3: |4 - 10|, |12 - 20|, |24 - 30| over 40
    assert ks[4] == 8.0 / 40.0
    big = np.full((1, 256), 2 ** 31 - 1, dtype=np.int64)          # the numerator stays inside 64 bits at the largest int32 counts
    assert rescale.ks_binned(big)[0] == 0.0
    assert rescale.band(1.36, np.array([0, 4]))[0] == np.inf and rescale.band(1.36, np.array([0, 4]))[1] == 0.68


N, B, T = 6, 2, 600


def test_time_rescaling_is_a_stack_of_per_sample_folds():
    np.random.seed(0)
    model = M.SparseBernoulliGLM(N, B=B, regression_kwargs=dict(S_w=3.0, mu_b=-1.0), engine_factory=OracleEngine, seed=1)
    rng = np.random.default_rng(3)
    Ys = [(rng.random((T, N)) < 0.2).astype(float), (rng.random((T // 2, N)) < 0.1).astype(float)]
    for Y in Ys:
        model.add_data(Y)
    D, S = 16, 4
    gof = model.time_rescaling(bins=D, seed=9, coef=1.0)
    assert gof.count == 0
    with pytest.raises(RuntimeError):
        gof.ks_mean
    hists, kss = [], []
    for k in range(S):
        model.resample_model()
        gof.collect()
        a, W, b = model._local_state()
        h = sum(rescale.rescale_host(model.engine.psi(a, W, b, i), Y, 1.0, D, 9, k, 0, e0)[0] for i, (Y, e0) in enumerate(zip(Ys, (0, T))))
        hists.append(h)
        kss.append(rescale.ks_binned(h))
        assert np.array_equal(gof.hist_last, h) and np.array_equal(gof.ks_last, kss[-1])
    hists, kss = np.array(hists), np.array(kss)
    M_ = np.array([(Ys[0][:, n] > 0).sum() - 1 + (Ys[1][:, n] > 0).sum() - 1 for n in range(N)])
    assert gof.count == S and np.array_equal(gof.intervals, M_) and np.array_equal(gof.hist, hists.sum(axis=0))
    np.testing.assert_allclose(gof.ks_mean, kss.mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(gof.ks_std, kss.std(axis=0), rtol=0, atol=1e-13)
    assert np.array_equal(gof.band, 1.0 / np.sqrt(M_))
    assert np.array_equal(gof.exceed_fraction, (kss > 1.0 / np.sqrt(M_)).mean(axis=0))
    assert 0 < gof.exceed_fraction.sum() < N                                  # (coef = 1: some neurons leave the band, some do not)
    assert np.array_equal(gof.failing(0.5), np.flatnonzero(gof.exceed_fraction > 0.5))
    z1 = gof.zsum_last
    assert z1.shape == (N, 2) and np.all(z1[:, 0] > 0) and np.all(z1[:, 1] < z1[:, 0])
    # the model's one-off read-out is sample 1 (call 0) of one data set at the current state
    h1, zs1 = model.rescaled_intervals(data=1, bins=D, seed=9)
    a, W, b = model._local_state()
    ref = rescale.rescale_host(model.engine.psi(a, W, b, 1), Ys[1], 1.0, D, 9, 0, 0, T)
    assert np.array_equal(h1, ref[0]) and np.array_equal(zs1, ref[1])
    gof.reset()
    assert gof.count == 0
    gof.collect()
    assert np.array_equal(gof.hist, gof.hist_last) and np.array_equal(gof.ks_mean, gof.ks_last) and not gof.ks_std.any()
    # held-out data go through the engine of summarize(datas=...)
    held = model.time_rescaling(bins=D, seed=9, datas=[Ys[1]])
    held.collect()
    eng = model._heldout_engine([Ys[1]])
    assert np.array_equal(held.hist, rescale.rescale_host(eng.psi(a, W, b, 0), Ys[1], 1.0, D, 9, 0, 0, 0)[0])
    model.add_data(Ys[1])
    with pytest.raises(RuntimeError, match="data was added"):
        gof.collect()


def test_a_gaussian_neuron_is_refused_by_name():
    regs = [SparseBernoulliRegression(4, 2) for _ in range(4)]
    regs[2] = SparseGaussianRegression(4, 2, eta=0.3)
    model = NonlinearAutoregressiveModel(4, regs, B=2, engine_factory=OracleEngine)
    with pytest.raises(ValueError, match="neuron 2 is Gaussian"):
        model.time_rescaling()
    with pytest.raises(ValueError, match="neuron 2 is Gaussian"):
        model.rescaled_intervals()
    for bins in (1, 257):
        with pytest.raises(ValueError, match="bins"):
            rescale.check_bins(bins)


# ---- statistical sense
class PsiEngine(object):
    """NumPy stand-in for GibbsEngine where only psi is needed, for any list of regressions: X by the oracle's basis convolution,
    psi = X (a * W)' + b"""

    def __init__(self, N, B, n0=0, n1=None, **kw):
        self.N, self.B, self.n0, self.n1 = N, B, n0, N if n1 is None else n1
        self.datasets = []

    def add_data(self, Y, X=None, basis=None, **kw):
        self.datasets.append(orc.convolve_with_basis(Y, basis) if X is None else np.asarray(X))

    def design_matrix(self, i=0):
        return self.datasets[i]

    def psi(self, a, W, b, i=0):
        X = self.datasets[i]
        return X.reshape(X.shape[0], -1).dot((np.asarray(a)[:, :, None] * np.asarray(W)).reshape(len(b), -1).T) + np.asarray(b).reshape(-1)


STAT_N, STAT_T = 8, 20000
STAT_SEED = 1          # of the state and of the simulated recording: with it the host path meets both verdicts below (tried 1 first)


def statistical_model(engine_factory=PsiEngine):
    """N = 8 neurons, Bernoulli and negative binomial (xi = 2) in turn, at a sparse random state"""
    np.random.seed(STAT_SEED)
    Nn, Bb = STAT_N, 3
    regs = [SparseBernoulliRegression(Nn, Bb, mu_b=-2.0, S_b=0.1) if i % 2 == 0 else SparseNegativeBinomialRegression(Nn, Bb, xi=2.0, mu_b=-1.0, S_b=0.1)
            for i in range(Nn)]
    model = NonlinearAutoregressiveModel(Nn, regs, basis=cosine_basis(Bb, L=30) / 30, engine_factory=engine_factory)
    A, W, b = model._adopt_state()
    rng = np.random.default_rng(STAT_SEED)
    A[...] = rng.random((Nn, Nn)) < 0.5
    W[...] = rng.standard_normal(W.shape) * 0.15
    b[:, 0] = np.where(np.arange(Nn) % 2 == 0, -2.5, -3.0) + 0.3 * rng.standard_normal(Nn)
    return model


@functools.lru_cache(maxsize=None)
def statistical_data(gpu=False):
    """T = 20 000 bins simulated from statistical_model(); here on the NumPy path (the device path follows the same law to the last bit,
    tests/test_gpu_simulate.py, and takes a fraction of the time: what the GPU tests use)"""
    Y = statistical_model(engine_factory=None if gpu else PsiEngine).simulate(STAT_T, seed=STAT_SEED, gpu=gpu).Y[0]
    Y.setflags(write=False)
    return Y


def statistical_verdicts(model, host=False):
    """(ks, M, exceed_fraction) at the generating state and with every bias shifted by + 0.5, one sample each, through the class behind
    model.time_rescaling() (host=True: its NumPy fold whatever the engine) -- restores the state"""
    out = []
    _, _, b = model._adopt_state()
    b0 = b.copy()
    for shift in (0.0, 0.5):
        b[...] = b0 + shift
        try:
            gof = rescale.TimeRescaling(model, bins=64, seed=STAT_SEED, coef=1.63, host=host)
            gof.collect()
            out.append((gof.ks_last, gof.intervals, gof.exceed_fraction))
        finally:
            b[...] = b0
    return out


def check_verdicts(verdicts):
    (ks0, M0, ex0), (ks1, M1, ex1) = verdicts
    assert np.array_equal(M0, M1) and M0.min() >= 200
    assert np.sum(ks0 > 1.63 / np.sqrt(M0)) <= 1 and np.array_equal(ex0, ks0 > 1.63 / np.sqrt(M0))
    assert np.all(ks1[M1 >= 200] > 1.63 / np.sqrt(M1[M1 >= 200])) and np.array_equal(ex1, ks1 > 1.63 / np.sqrt(M1))


def test_the_generating_state_passes_and_shifted_biases_fail():
    model = statistical_model()
    model.add_data(np.array(statistical_data()))
    verdicts = statistical_verdicts(model)
    print("sqrt(M) ks at the generating state", np.sqrt(verdicts[0][1]) * verdicts[0][0])
    print("sqrt(M) ks with the biases shifted", np.sqrt(verdicts[1][1]) * verdicts[1][0])
    check_verdicts(verdicts)
