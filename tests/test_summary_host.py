"""The posterior accumulator (model.summarize, pyglm_amd/summary.py) on its host fallback -- the specification of the device kernels --
against brute force over stacked samples.  CPU only: models on engine_factory=OracleEngine, and a small stub engine for the hooks mode.

Tolerances follow from fp64 rounding: means rtol = 1e-12 with atol = 1e-12 max|x| (a weight mean may cancel to nearly zero); variances and
M2-derived values atol = 1e-12 max(x^2) (Welford against the two-pass formula differs by O(S eps max x^2), S <= 32 samples); lppd and
p_waic rtol = 1e-10."""
import numpy as np
import pytest
from scipy.special import logsumexp

from oracle import pyglm_oracle as orc
from pyglm_amd import models as M
from pyglm_amd import regression as R
from pyglm_amd.utils.utils import logistic
from tests._oracle_engine import OracleEngine

N, B, T = 6, 2, 600


def close_mean(x, ref):
    ref = np.asarray(ref, dtype=float)
    np.testing.assert_allclose(x, ref, rtol=1e-12, atol=1e-12 * max(np.max(np.abs(ref)), 1e-300))


def close_var(x, ref, scale):
    """scale: the values the variance is of"""
    np.testing.assert_allclose(x, ref, rtol=0, atol=1e-12 * max(np.max(np.asarray(scale, dtype=float) ** 2), 1e-300))


def terms_of(model, Y, psi):
    """the per-cell log-likelihood term, (T, N), from psi and the regressions' own hooks (eta for Gaussian observations)"""
    out = np.empty_like(psi)
    for n, r in enumerate(model.regressions):
        y = Y[:, n]
        if isinstance(r, R.SparseGaussianRegression):
            out[:, n] = -0.5 * np.log(2 * np.pi * r.eta) - (y - psi[:, n]) ** 2 / (2 * r.eta)
        else:
            out[:, n] = np.log(r.c_func(y)) + r.a_func(y) * psi[:, n] - r.b_func(y) * np.log1p(np.exp(psi[:, n]))
    return out


def psi_of(model, eng, i=0):
    a, W, b = model._local_state()
    return np.asarray(eng.psi(a, W, b, i))


class Brute(object):
    """stacked samples, as the reference's workflow keeps them"""

    def __init__(self):
        self.A, self.W, self.b, self.mu, self.l, self.ll = [], [], [], [], [], []

    def take(self, model, Y, eng=None, rates=True):
        self.A.append(model.adjacency)
        self.W.append(model.adjacency[:, :, None] * model.weights)
        self.b.append(model.biases)
        if rates:
            self.mu.append(model.means[0])
        self.l.append(terms_of(model, Y, psi_of(model, eng or model.engine)))

    def check_state(self, acc):
        A, W, b = np.array(self.A, dtype=float), np.array(self.W), np.array(self.b)
        close_mean(acc.edge_prob, A.mean(0))
        close_mean(acc.weight_mean, W.mean(0))
        close_var(acc.weight_var, W.var(0), W)
        close_mean(acc.bias_mean, b.mean(0))
        close_var(acc.bias_var, b.var(0), b)

    def check_rates(self, acc):
        mu = np.array(self.mu)
        close_mean(acc.rate_mean[0], mu.mean(0))
        close_var(acc.rate_std[0] ** 2, mu.var(0), mu)

    def check_pointwise(self, acc):
        l = np.array(self.l)
        S = l.shape[0]
        per = (logsumexp(l, axis=0) - np.log(S)).sum(axis=0)
        got = acc.lppd()
        np.testing.assert_allclose(got["per_neuron"], per, rtol=1e-10)
        np.testing.assert_allclose(got["total"], per.sum(), rtol=1e-10)
        if S >= 2:
            p = l.var(axis=0, ddof=1).sum(axis=0)
            w = acc.waic()
            np.testing.assert_allclose(w["lppd"], per.sum(), rtol=1e-10)
            np.testing.assert_allclose(w["p_waic"], p.sum(), rtol=1e-10)
            np.testing.assert_allclose(w["waic"], -2 * (per.sum() - p.sum()), rtol=1e-10)
            np.testing.assert_allclose(w["per_neuron"], -2 * (per - p), rtol=1e-10)


def bernoulli_model():
    np.random.seed(0)
    model = M.SparseBernoulliGLM(N, B=B, regression_kwargs=dict(S_w=3.0, mu_b=-1.0), engine_factory=OracleEngine, seed=1)
    Y = (np.random.default_rng(3).random((T, N)) < 0.2).astype(float)
    model.add_data(Y)
    return model, Y


def test_bernoulli_every_readout_against_stacked_samples():
    model, Y = bernoulli_model()
    acc = model.summarize(rates=True, pointwise=True)
    assert acc.count == 0 and acc.log_likelihoods == []
    brute, lls = Brute(), []
    for it in range(12):
        model.resample_model()
        if it >= 2:
            ll = acc.collect()
            assert ll == model.log_likelihood()
            lls.append(ll)
            brute.take(model, Y)
    assert acc.count == 10 and acc.log_likelihoods == lls
    freq = np.array(brute.A, dtype=float).mean(0)
    assert np.sum((freq > 0) & (freq < 1)) >= N * N // 2, "the fixture no longer exercises the mean of the adjacency"
    brute.check_state(acc)
    brute.check_rates(acc)
    brute.check_pointwise(acc)
    assert acc.edge_prob.shape == (N, N) and acc.weight_var.shape == (N, N, B) and acc.rate_std[0].shape == (T, N)


def test_heldout_pointwise_against_brute_force():
    model, Y = bernoulli_model()
    Y2 = (np.random.default_rng(5).random((400, N)) < 0.2).astype(float)
    acc = model.summarize(rates=False, pointwise=True, datas=[Y2])
    brute = Brute()
    for it in range(6):
        model.resample_model()
        assert acc.collect() == model.log_likelihood([Y2])
        brute.take(model, Y2, eng=model._heldout_engine([Y2]), rates=False)
    brute.check_pointwise(acc)
    brute.check_state(acc)
    with pytest.raises(RuntimeError, match="rates"):
        acc.rate_mean


@pytest.mark.parametrize("kind", ["gaussian", "negbin", "binomial"])
def test_other_observation_models(kind):
    np.random.seed(0)
    rng = np.random.default_rng(3)
    if kind == "gaussian":
        model = M.SparseGaussianGLM(N, B=B, engine_factory=OracleEngine, seed=1)
        Y = rng.standard_normal((T, N))
    elif kind == "negbin":
        model = M.SparseNegativeBinomialGLM(N, B=B, regression_kwargs=dict(xi=2.5), engine_factory=OracleEngine, seed=1)
        Y = np.floor(3 * rng.random((T, N)))
    else:
        model = M.SparseBinomialGLM(N, B=B, regression_kwargs=dict(n=3), engine_factory=OracleEngine, seed=1)
        Y = np.floor(2.2 * rng.random((T, N)))
    model.add_data(Y)
    acc = model.summarize(rates=True, pointwise=True)
    brute = Brute()
    for it in range(12):
        model.resample_model()
        if it >= 2:
            assert acc.collect() == model.log_likelihood()
            brute.take(model, Y)
    assert np.all(np.isfinite(acc.rate_mean[0]))
    brute.check_state(acc)
    brute.check_rates(acc)
    brute.check_pointwise(acc)


# ---- hooks mode: OracleEngine.add_data takes no obs_terms and cannot sweep that mode; a stub engine and states set by hand
class StubEngine(object):
    def __init__(self, N, B, n0=0, n1=None, obs="bernoulli", xi=1.0, **kw):
        self.N, self.B, self.n0, self.n1 = N, B, n0, N if n1 is None else n1
        self.obs, self.datasets = obs, []

    def add_data(self, Y, X=None, basis=None, obs_terms=None):
        if X is None:
            X = orc.convolve_with_basis(Y, basis)
        self.datasets.append((np.asarray(X).reshape(Y.shape[0], self.N * self.B), np.asarray(Y, float), obs_terms))

    def psi(self, a, W, b, i=0):
        aw = (np.asarray(a, float)[:, :, None] * np.asarray(W, float)).reshape(self.n1 - self.n0, -1)
        return self.datasets[i][0].dot(aw.T) + np.asarray(b, float).reshape(-1)

    def log_likelihood(self, a, W, b):
        out = 0.0
        for i, (X, Y, (A, Bv, logC)) in enumerate(self.datasets):
            psi = self.psi(a, W, b, i)
            out = out + (logC + A * psi - Bv * np.log1p(np.exp(psi))).sum(axis=0)
        return out


def hooks_model():
    np.random.seed(0)
    regs = [R.SparseBernoulliRegression(N, B) for _ in range(2)] + [R.SparseBinomialRegression(N, B, n=4) for _ in range(2)] \
        + [R.SparseNegativeBinomialRegression(N, B, xi=2.0) for _ in range(2)]
    model = M.GLM(N, regs, B=B, engine_factory=StubEngine, seed=1)
    rng = np.random.default_rng(7)
    Y = np.floor(2 * rng.random((T, N)))
    Y[:, :2] = Y[:, :2] > 0
    model.add_data(Y)
    assert model.engine_obs() == "hooks"
    return model, Y, rng


def set_state(model, rng):
    for r in model.regressions:
        r.a = rng.random(N) < 0.5
        r.W = 0.3 * rng.standard_normal((N, B))
        r.b = rng.standard_normal(1) - 1.0


def test_hooks_mode_rates_per_neurons_own_model_and_lppd():
    model, Y, rng = hooks_model()
    acc = model.summarize(rates=True, pointwise=True)
    brute = Brute()
    for _ in range(4):
        set_state(model, rng)
        assert acc.collect() == model.log_likelihood()
        brute.take(model, Y)
    mu = np.array(brute.mu)
    psi = psi_of(model, model.engine)
    np.testing.assert_allclose(mu[-1][:, 0], logistic(psi[:, 0]), rtol=1e-12)           # each neuron's own model
    np.testing.assert_allclose(mu[-1][:, 2], 4 * logistic(psi[:, 2]), rtol=1e-12)
    np.testing.assert_allclose(mu[-1][:, 4], 2.0 * np.exp(psi[:, 4]), rtol=1e-12)
    brute.check_state(acc)
    brute.check_rates(acc)
    brute.check_pointwise(acc)


def test_hooks_mode_user_mean_raises_and_rates_false_works():
    class OwnMean(R.SparseBernoulliRegression):
        def mean(self, X):
            return 0.5 * logistic(self.activation(X))

        def b_func(self, data):
            return 1.0 + 0 * data

    model, Y, rng = hooks_model()
    np.random.seed(1)
    model.regressions[1] = OwnMean(N, B)
    with pytest.raises(ValueError, match=r"OwnMean.*rates=False"):
        model.summarize(rates=True)
    acc = model.summarize(rates=False, pointwise=True)
    brute = Brute()
    for _ in range(3):
        set_state(model, rng)
        acc.collect()
        brute.take(model, Y, rates=False)
    brute.check_pointwise(acc)


def test_errors():
    model, Y = bernoulli_model()
    acc = model.summarize(rates=True, pointwise=False)
    for name in ("edge_prob", "weight_mean", "weight_var", "bias_mean", "bias_var", "rate_mean", "rate_std"):
        with pytest.raises(RuntimeError):
            getattr(acc, name)
    acc.collect()
    acc.edge_prob
    with pytest.raises(RuntimeError, match="pointwise"):
        acc.lppd()
    with pytest.raises(RuntimeError, match="pointwise"):
        acc.waic()
    pw = model.summarize(rates=False, pointwise=True)
    with pytest.raises(RuntimeError):
        pw.lppd()
    pw.collect()
    pw.lppd()
    with pytest.raises(RuntimeError, match="at least 2"):
        pw.waic()
    model.add_data(Y[:100])
    with pytest.raises(RuntimeError, match="after summarize"):
        acc.collect()


def test_reset_then_the_same_folds_gives_the_same_bits():
    model, Y = bernoulli_model()
    acc = model.summarize(rates=True, pointwise=True)
    states = []
    for _ in range(4):
        model.resample_model()
        states.append(model.get_state())
        acc.collect()
    first = [acc.edge_prob, acc.weight_mean, acc.weight_var, acc.bias_var, acc.rate_mean[0], acc.rate_std[0], acc.lppd()["per_neuron"],
             acc.waic()["per_neuron"], list(acc.log_likelihoods)]
    acc.reset()
    assert acc.count == 0 and acc.log_likelihoods == []
    for st in states:
        model.set_state(st)
        acc.collect()
    again = [acc.edge_prob, acc.weight_mean, acc.weight_var, acc.bias_var, acc.rate_mean[0], acc.rate_std[0], acc.lppd()["per_neuron"],
             acc.waic()["per_neuron"], list(acc.log_likelihoods)]
    for x, y in zip(first, again):
        np.testing.assert_array_equal(x, y)
