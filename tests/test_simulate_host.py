"""model.simulate() and model.predictive_check() on the NumPy path (pyglm_amd/simulate.py): the Philox words against the oracle's, the four laws
against scipy.stats on 1e6 i.i.d. draws each (fixed seeds: deterministic), the per-neuron dispatch, the negative-binomial cap, replicate
independence, continuation, and the posterior predictive p-values.  No GPU."""
import numpy as np
import pytest
from scipy import stats

from pyglm_amd import simulate
from pyglm_amd._lib import PglError
from pyglm_amd.models import NonlinearAutoregressiveModel, SparseBernoulliGLM
from pyglm_amd.regression import (SparseBernoulliRegression, SparseBinomialRegression, SparseGaussianRegression,
                                  SparseNegativeBinomialRegression)
from pyglm_amd.utils.basis import cosine_basis
from pyglm_amd.utils.utils import logistic
from tests._oracle_engine import OracleEngine

P_MIN = 1e-4


@pytest.mark.parametrize("seed,j,elem0,stream", [
    (1, 0, 0, 0), (0xDEADBEEF12345678, 3, 2 ** 31 - 5, (7 << 32) | 1023), (5, 0, 100, ((2 ** 31 - 2) << 32) | 5), (2 ** 64 - 1, 77, 12345, 1 << 32)])
def test_philox_words_are_the_oracles(seed, j, elem0, stream):
    from oracle.pyglm_oracle import philox_words
    assert np.array_equal(simulate.philox_words(seed, simulate.PURPOSE_SIM, j, elem0, stream, 17), philox_words(seed, 2, j, elem0, stream, 17))


def test_the_uniforms_are_call_zero_of_the_documented_stream():
    u1, u2 = simulate.sim_uniforms(9, 41, [3, 1000], [0, 6])
    for i, rep in enumerate((0, 6)):
        for k, n in enumerate((3, 1000)):
            w = simulate.philox_words(9, simulate.PURPOSE_SIM, 0, 41, (rep << 32) | n, 1)[0].astype(object)
            assert u1[i, k] == ((((w[1] << 32) | w[0]) >> 11) + 0.5) / 2.0 ** 53 and u2[i, k] == ((((w[3] << 32) | w[2]) >> 11) + 0.5) / 2.0 ** 53


def _iid(kind, par, psi, seed):
    """1e6 i.i.d. draws: 100 neurons without connections at a constant bias, 100 replicates, 100 bins"""
    N, B, L = 100, 1, 3
    sim = simulate.simulate(np.zeros((N, N * B)), np.full(N, psi), np.ones((L, B)), np.full(N, kind), np.full(N, par), 100, replicates=100, seed=seed)
    assert sim.Y.shape == (100, 100, N)
    return sim.Y.ravel()


def _chi2_p(y, pmf):
    """p-value of the chi-square test of integer draws y against pmf(k), k = 0 .. kmax, cells pooled until each expects >= 10"""
    counts = np.bincount(y.astype(np.int64))
    expect = y.size * pmf(np.arange(counts.size))
    obs, exp, o, e = [], [], 0.0, 0.0
    for c, x in zip(counts, expect):
        o, e = o + c, e + x
        if e >= 10:
            obs.append(o)
            exp.append(e)
            o = e = 0.0
    tail = y.size - sum(exp)                                   # everything beyond the last full cell
    if tail >= 10:
        obs.append(y.size - sum(obs))
        exp.append(tail)
    else:
        obs[-1] += y.size - sum(obs)
        exp[-1] += tail
    return stats.chisquare(obs, exp).pvalue


def test_bernoulli_law():
    psi = -1.3
    y = _iid(simulate.KIND_BERNOULLI, 0.0, psi, seed=101)
    assert set(np.unique(y)) == {0.0, 1.0}
    assert _chi2_p(y, lambda k: stats.bernoulli.pmf(k, logistic(psi))) > P_MIN


@pytest.mark.parametrize("n,psi,seed", [(1, -0.8, 111), (1, 0.6, 112), (10, -0.8, 113), (10, 0.6, 114), (64, -0.8, 115), (64, 0.6, 116), (64, 3.0, 117)])
def test_binomial_law(n, psi, seed):
    y = _iid(simulate.KIND_BINOMIAL, float(n), psi, seed)
    assert y.min() >= 0 and y.max() <= n and np.all(y == np.floor(y))
    assert _chi2_p(y, lambda k: stats.binom.pmf(k, n, logistic(psi))) > P_MIN


@pytest.mark.parametrize("xi,psi,seed", [(1.0, -0.5, 121), (1.0, 1.2, 122), (2.5, -0.5, 123), (2.5, 1.2, 124)])
def test_negative_binomial_law(xi, psi, seed):
    y = _iid(simulate.KIND_NEGBIN, xi, psi, seed)
    assert y.min() >= 0 and np.all(y == np.floor(y))
    assert abs(y.mean() / (xi * np.exp(psi)) - 1) < 0.01       # the mean the regression's `mean` states
    assert _chi2_p(y, lambda k: stats.nbinom.pmf(k, xi, 1.0 - logistic(psi))) > P_MIN


def test_gaussian_law():
    psi, eta = 0.7, 0.3
    y = _iid(simulate.KIND_GAUSSIAN, np.sqrt(eta), psi, seed=131)
    assert stats.kstest((y - psi) / np.sqrt(eta), "norm").pvalue > P_MIN


# ---- dispatch
def _mixed_model(N=6, B=2, L=15, seed=0):
    np.random.seed(seed)
    regs = [SparseBernoulliRegression(N, B, mu_b=-1.0, S_b=0.1), SparseNegativeBinomialRegression(N, B, xi=2.5, mu_b=-1.0, S_b=0.1),
            SparseBinomialRegression(N, B, n=10, mu_b=-1.0, S_b=0.1), SparseBernoulliRegression(N, B, mu_b=-1.0, S_b=0.1),
            SparseNegativeBinomialRegression(N, B, xi=1.0, mu_b=-1.0, S_b=0.1), SparseBinomialRegression(N, B, n=64, mu_b=1.0, S_b=0.1)][:N]
    model = NonlinearAutoregressiveModel(N, regs, basis=cosine_basis(B, L=L) / L)
    model._adopt_state()[1][...] *= 0.2
    return model


def test_a_mixed_list_gives_per_neuron_kind_and_par():
    model = _mixed_model()
    kind, par = simulate.observation_kinds(model.regressions)
    assert kind.tolist() == [0, 2, 3, 0, 2, 3] and par[[1, 2, 4, 5]].tolist() == [2.5, 10.0, 1.0, 64.0]
    sim = model.simulate(400, replicates=2, seed=3, gpu=False)
    Y, s, ss, hist = sim
    assert Y.shape == (2, 400, 6) and s.shape == ss.shape == (2, 6) and hist.shape == (2, 15, 6)
    assert set(np.unique(Y[:, :, [0, 3]])) == {0.0, 1.0} and Y[:, :, 2].max() <= 10 and 10 < Y[:, :, 5].max() <= 64 and Y[:, :, 1].max() > 1
    g = SparseGaussianRegression(6, 2, eta=0.25)
    assert simulate.observation_kinds([g])[1][0] == 0.5


def test_the_activation_is_that_of_means():
    # a weight behind a closed edge must not act: simulate() uses a*W where generate() uses the stored W
    model = _mixed_model()
    A, W, b = model._adopt_state()
    base = model.simulate(200, replicates=2, seed=5, gpu=False)
    W[~A] = 50.0
    assert np.array_equal(model.simulate(200, replicates=2, seed=5, gpu=False).Y, base.Y)


class _OwnRvs(SparseBernoulliRegression):
    def rvs(self, X=None, size=[], psi=None):
        return (np.random.rand(*psi.shape) < 0.5 * logistic(psi)).astype(float)


class _HooksOnly(SparseBernoulliRegression):
    def b_func(self, data):
        return 2.0 * np.ones_like(data, dtype=float)


def test_a_user_model_is_refused_by_name():
    N, B = 4, 2
    for make, name in [(lambda: _OwnRvs(N, B), "_OwnRvs"), (lambda: _HooksOnly(N, B), "_HooksOnly")]:
        regs = [SparseBernoulliRegression(N, B) for _ in range(N - 1)] + [make()]
        model = NonlinearAutoregressiveModel(N, regs, B=B)
        with pytest.raises(ValueError, match=name):
            model.simulate(10, gpu=False)
    regs = [SparseBernoulliRegression(N, B) for _ in range(N)]
    regs[1].rvs = lambda **kw: None                            # an attribute of the instance
    with pytest.raises(ValueError, match="regression 1"):
        NonlinearAutoregressiveModel(N, regs, B=B).simulate(10, gpu=False)
    regs = [SparseBinomialRegression(N, B, n=65) for _ in range(N)]
    with pytest.raises(ValueError, match="n <= 64"):
        NonlinearAutoregressiveModel(N, regs, B=B).simulate(10, gpu=False)


def test_gpu_true_without_a_gpu_is_an_error():
    import torch
    model = _mixed_model()
    if torch.cuda.is_available():                              # (run on a GPU box: gpu=True is then simply the device path)
        assert model.simulate(10, gpu=True).Y.shape == (1, 10, 6)
        return
    with pytest.raises(PglError):
        model.simulate(10, gpu=True)
    assert model.simulate(10, gpu=None).Y.shape == (1, 10, 6)  # gpu=None: the NumPy path


def test_an_exploding_count_model_raises_with_bin_replicate_and_neuron():
    model = _mixed_model()
    model._adopt_state()[2][4, 0] = 40.0
    with pytest.raises(PglError) as err:
        model.simulate(20, replicates=3, seed=1, first_replicate=7, gpu=False)
    msg = str(err.value)
    assert "neuron 4" in msg and "replicate 7" in msg and "bin 0" in msg and str(simulate.NEGBIN_CAP) in msg


# ---- what a path depends on
def test_replicates_are_independent_of_how_they_are_batched():
    model = _mixed_model()
    six = model.simulate(300, replicates=6, seed=9, first_replicate=4, gpu=False)
    for r in range(6):
        one = model.simulate(300, replicates=1, seed=9, first_replicate=4 + r, gpu=False)
        assert np.array_equal(one.Y[0], six.Y[r]) and np.array_equal(one.sum[0], six.sum[r]) and np.array_equal(one.sumsq[0], six.sumsq[r])
    assert len(np.unique(six.sum, axis=0)) == 6
    np.random.seed(123)                                        # NumPy's global generator plays no part
    assert np.array_equal(model.simulate(300, replicates=6, seed=9, first_replicate=4, gpu=False).Y, six.Y)
    assert not np.array_equal(model.simulate(300, replicates=6, seed=10, first_replicate=4, gpu=False).Y, six.Y)


def test_continuation_and_sums(monkeypatch):
    model = _mixed_model()
    whole = model.simulate(300, replicates=3, seed=4, gpu=False)
    first = model.simulate(100, replicates=3, seed=4, gpu=False)
    second = model.simulate(200, replicates=3, seed=4, gpu=False, history=first)
    assert (second.t0, second.t1) == (100, 300)
    assert np.array_equal(np.concatenate([first.Y, second.Y], axis=1), whole.Y)
    assert np.array_equal(first.sum + second.sum, whole.sum) and np.array_equal(second.history, whole.history)
    assert np.array_equal(whole.history, whole.Y[:, -15:])
    assert np.array_equal(model.simulate(200, replicates=3, seed=4, gpu=False, history=first.history, t0=100).Y, second.Y)
    monkeypatch.setattr(simulate, "HOST_BLOCK_BINS", 37)       # the rolling buffer of a run that keeps no paths wraps
    bare = model.simulate(300, replicates=3, seed=4, gpu=False, keep_paths=False)
    assert bare.Y is None and np.array_equal(bare.sum, whole.Y.sum(axis=1)) and np.array_equal(bare.sumsq, (whole.Y ** 2).sum(axis=1))
    assert np.array_equal(bare.history, whole.history)
    np.testing.assert_allclose(bare.fano(), whole.Y.var(axis=1) / whole.Y.mean(axis=1), rtol=1e-9)


def test_a_forecast_starts_from_the_rows_given():
    model = _mixed_model()
    data = model.simulate(100, seed=2, gpu=False).Y[0]
    f = model.simulate(50, replicates=4, seed=6, history=data[-15:], t0=100, gpu=False)
    longer = model.simulate(50, replicates=4, seed=6, history=data, t0=100, gpu=False)       # only the last L rows count
    assert np.array_equal(f.Y, longer.Y) and f.t0 == 100
    silent = model.simulate(50, replicates=4, seed=6, t0=100, gpu=False)
    assert not np.array_equal(f.Y, silent.Y)
    # the first bin of the forecast is drawn at the activation the data's last rows give
    x = data[-15:][::-1].T.dot(model.basis).reshape(-1)
    A, W, b = model._adopt_state()
    psi = (W * A[:, :, None]).reshape(6, -1).dot(x) + b[:, 0]
    u1, _ = simulate.sim_uniforms(6, 100, np.arange(6), np.arange(4))
    assert np.array_equal(f.Y[:, 0, 0], (u1[:, 0] < logistic(psi[0])).astype(float))
    with pytest.raises(ValueError):
        model.simulate(5, replicates=4, history=np.zeros((3, 15, 6)), gpu=False)


# ---- the predictive check
def test_predictive_check_flags_the_neuron_that_fires_at_three_times_its_rate():
    N, B, L, T, S, R = 6, 2, 20, 2000, 5, 8
    np.random.seed(0)
    model = SparseBernoulliGLM(N, basis=cosine_basis(B, L=L) / L, regression_kwargs=dict(mu_b=-2.0, S_b=0.1), engine_factory=OracleEngine, seed=1)
    A, W, b = model._adopt_state()
    rng = np.random.default_rng(1)
    W[...] = 0.5 * rng.standard_normal(W.shape)
    b[:, 0] = -2.0 + 0.2 * rng.standard_normal(N)
    data = model.simulate(T, seed=82, gpu=False).Y[0]          # from the model itself, with another seed than the check's
    rate3 = data[:, 3].mean()
    data[:, 3] = np.random.default_rng(2).random(T) < 3.0 * rate3
    model.add_data(data)
    ppc = model.predictive_check(replicates=R, seed=0, gpu=False)
    for _ in range(S):                                         # a fixed state: S collections of R fresh replicates
        ppc.collect()
    assert ppc.rates.shape == ppc.fanos.shape == (S * R, N) and ppc.calls == S
    assert len(np.unique(ppc.rates, axis=0)) == S * R          # no replicate index was used twice
    p = ppc.pvalue("rate")
    assert p[3] == 2.0 / (S * R + 1)                           # the smallest value the two-sided estimator attains
    others = np.delete(p, 3)
    assert np.all((others >= 0.02) & (others <= 0.98)), p
    q = ppc.rate_quantiles([0.05, 0.5, 0.95])
    assert q.shape == (3, N) and np.all(q[0] <= q[1]) and np.all(q[1] <= q[2]) and data[:, 3].mean() > q[2, 3]
    assert ppc.fano_quantiles([0.5]).shape == (1, N) and ppc.pvalue("fano").shape == (N,)
    with pytest.raises(ValueError):
        ppc.pvalue("isi")
