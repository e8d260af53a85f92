"""The lagged cross-correlogram on the NumPy path (pyglm_amd/simulate.py): the definition of the lagged products against a triple loop, the
normalisation on a hand-made pair of series, the sums that simulate(gpu=False, lags=K) folds block by block, the streamed p-values of
PredictiveCheck(lags=K) against the rule applied to explicitly stacked replicates, and the limits on `lags`.  No GPU."""
import numpy as np
import pytest

from pyglm_amd import simulate
from pyglm_amd.models import NonlinearAutoregressiveModel
from pyglm_amd.regression import SparseBernoulliRegression, SparseBinomialRegression, SparseNegativeBinomialRegression
from pyglm_amd.utils.basis import cosine_basis
from tests._oracle_engine import OracleEngine


def _model(N, B, L, kinds, seed, **kw):
    make = {"bernoulli": lambda i: SparseBernoulliRegression(N, B, mu_b=-2.0, S_b=0.1),
            "negbin": lambda i: SparseNegativeBinomialRegression(N, B, xi=2.5, mu_b=-1.0, S_b=0.1),
            "binomial": lambda i: SparseBinomialRegression(N, B, n=10, mu_b=-1.0, S_b=0.1)}
    np.random.seed(seed)
    regs = [make[kinds[i % len(kinds)]](i) for i in range(N)]
    model = NonlinearAutoregressiveModel(N, regs, basis=cosine_basis(B, L=L) / L, **kw)
    A, W, b = model._adopt_state()
    rng = np.random.default_rng(seed)
    A[...] = rng.random((N, N)) < 0.5
    W[...] = rng.standard_normal(W.shape) * 0.5 / np.sqrt(N)
    W /= np.array([getattr(r, "n", 4.0 if hasattr(r, "xi") else 1.0) for r in regs], dtype=float)[None, :, None]
    b[:, 0] = -1.0 + 0.3 * rng.standard_normal(N)
    return model


def test_lagged_products_are_the_triple_loop():
    rng = np.random.default_rng(0)
    Y = rng.integers(-5, 6, size=(37, 3)).astype(float)
    K = 5
    S = simulate.lagged_products_host(Y, K)
    assert S.shape == (K, 3, 3)
    for l in range(K):
        for i in range(3):
            for j in range(3):
                assert S[l, i, j] == sum(int(Y[t, i]) * int(Y[t + l, j]) for t in range(37 - l))


def test_correlogram_of_a_hand_made_pair():
    # neuron 1 repeats neuron 0 one bin later; neuron 2 never fires
    a = np.array([1, 0, 0, 1, 0, 1, 0, 0], dtype=float)
    Y = np.stack([a, np.roll(a, 1), np.zeros(8)], axis=1)
    Y[0, 1] = 0.0
    T = 8
    S = simulate.lagged_products_host(Y, 2)
    c = simulate.correlogram(S, Y.sum(axis=0), (Y * Y).sum(axis=0), T)
    assert c.shape == (2, 3, 3)
    m0, m1 = 3 / 8, 3 / 8
    v0, v1 = m0 - m0 * m0, m1 - m1 * m1
    # lag 1, 0 -> 1: every spike of neuron 0 (bins 0, 3, 5) is followed by one of neuron 1: S = 3 over 7 pairs
    assert S[1, 0, 1] == 3 and c[1, 0, 1] == (3 / 7 - m0 * m1) / np.sqrt(v0 * v1)
    # lag 0, 0 -> 1: never in the same bin
    assert S[0, 0, 1] == 0 and c[0, 0, 1] == (0 / 8 - m0 * m1) / np.sqrt(v0 * v1)
    # lag 0 of a neuron with itself is 1
    np.testing.assert_allclose(c[0, 0, 0], 1.0, rtol=1e-15)
    # a silent neuron has no variance: its row and column are undefined
    assert np.all(np.isnan(c[:, 2, :])) and np.all(np.isnan(c[:, :, 2])) and not np.any(np.isnan(c[:, :2, :2]))
    # "i leads j": the transpose is the other direction
    assert S[1, 1, 0] == sum(Y[t, 1] * Y[t + 1, 0] for t in range(7)) and S[1, 1, 0] != S[1, 0, 1]


@pytest.mark.parametrize("kinds,T,K", [(("bernoulli", "binomial"), 300, 7), (("negbin", "bernoulli"), 120, 120)])
def test_host_simulation_carries_the_lagged_products_of_its_own_paths(kinds, T, K, monkeypatch):
    model = _model(5, 2, 10, kinds, seed=3)
    sim = model.simulate(T, replicates=3, seed=4, gpu=False, lags=K)
    assert sim.lagged.shape == (3, K, 5, 5) and sim.Y.sum() > 0
    for r in range(3):
        assert np.array_equal(sim.lagged[r], simulate.lagged_products_host(sim.Y[r], K))
    np.testing.assert_array_equal(sim.correlogram(), simulate.correlogram(sim.lagged, sim.sum, sim.sumsq, T))
    plain = model.simulate(T, replicates=3, seed=4, gpu=False)
    assert plain.lagged is None and np.array_equal(plain.Y, sim.Y) and np.array_equal(plain.history, sim.history)
    # without the paths, in blocks shorter than K - 1 and not dividing T
    monkeypatch.setattr(simulate, "HOST_BLOCK_BINS", 5 if K > 7 else 64)
    bare = model.simulate(T, replicates=3, seed=4, gpu=False, lags=K, keep_paths=False)
    assert bare.Y is None and np.array_equal(bare.lagged, sim.lagged) and np.array_equal(bare.sum, sim.sum)
    assert np.array_equal(bare.history, sim.history)


def test_lagged_products_do_not_pair_with_the_initial_history():
    model = _model(4, 2, 10, ("bernoulli",), seed=5)
    first = model.simulate(50, replicates=2, seed=6, gpu=False)
    second = model.simulate(80, replicates=2, seed=6, gpu=False, history=first, lags=6)
    for r in range(2):
        assert np.array_equal(second.lagged[r], simulate.lagged_products_host(second.Y[r], 6))


def test_streamed_pvalues_are_the_rule_on_stacked_replicates():
    model = _model(4, 2, 10, ("bernoulli",), seed=7, engine_factory=OracleEngine)        # (add_data without a GPU)
    model._adopt_state()[2][3, 0] = -30.0                                   # neuron 3 is silent in the replicates: undefined cells there
    data = model.simulate(400, seed=8, gpu=False).Y[0]
    data[7, 3] = 1.0                                                        # ... but defined in the data
    model.add_data(data)
    K, R = 6, 4
    ppc = model.predictive_check(replicates=R, seed=9, gpu=False, lags=K)
    stack = []
    for call in range(3):
        ppc.collect()
        sim = model.simulate(400, replicates=R, seed=9, first_replicate=call * R, gpu=False, lags=K)
        stack.append(sim.correlogram())
    rep = np.concatenate(stack, axis=0)                                     # (12, K, N, N)
    obs = ppc.observed["xcorr"]
    assert obs.shape == (K, 4, 4)
    assert np.array_equal(obs, simulate.correlogram(simulate.lagged_products_host(data, K), data.sum(0), (data * data).sum(0), 400), equal_nan=True)
    ok = ~np.isnan(rep)
    M = ok.sum(axis=0)
    ge, le = (ok & (rep >= obs)).sum(axis=0), (ok & (rep <= obs)).sum(axis=0)
    want = np.where(np.isnan(obs), np.nan, np.minimum(1.0, 2.0 * np.minimum(1 + ge, 1 + le) / (M + 1.0)))
    p = ppc.pvalue("xcorr")
    assert p.shape == (K, 4, 4) and np.array_equal(p, want, equal_nan=True)
    assert np.all(M[:, 3, :] == 0) and np.all(M[:, :3, :3] == 12)          # the excluded cells are really there
    assert np.all(p[:, 3, :] == 1.0) and p[:, :3, :3].min() >= 2.0 / 13.0
    with np.errstate(invalid="ignore"):
        np.testing.assert_allclose(ppc.xcorr_mean[:, :3, :3], rep[:, :, :3, :3].mean(axis=0), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(ppc.xcorr_std[:, :3, :3], rep[:, :, :3, :3].std(axis=0, ddof=1), rtol=1e-10, atol=1e-14)
    assert np.all(np.isnan(ppc.xcorr_mean[:, 3, :])) and np.all(np.isnan(ppc.xcorr_std[:, :, 3]))
    # the marginal statistics are what they were
    plain = model.predictive_check(replicates=R, seed=9, gpu=False)
    for _ in range(3):
        plain.collect()
    assert np.array_equal(plain.pvalue("rate"), ppc.pvalue("rate")) and np.array_equal(plain.pvalue("fano"), ppc.pvalue("fano"), equal_nan=True)
    with pytest.raises(ValueError):
        plain.pvalue("xcorr")


def test_limits_on_lags():
    model = _model(4, 2, 10, ("bernoulli",), seed=11, engine_factory=OracleEngine)
    Y = np.zeros((10, 4))
    assert simulate.lagged_products_host(Y, 10).shape == (10, 4, 4)           # K - 1 = 9 < T = 10
    with pytest.raises(ValueError):
        simulate.lagged_products_host(Y, 11)                                  # lags >= T + 1
    with pytest.raises(ValueError):
        model.simulate(10, gpu=False, lags=11)
    with pytest.raises(ValueError):
        model.simulate(1000, gpu=False, lags=simulate.PGL_LAG_MAX + 1)
    with pytest.raises(ValueError):
        simulate.lagged_products_host(np.zeros((1000, 4)), simulate.PGL_LAG_MAX + 1)
    model.add_data(np.zeros((10, 4)))
    with pytest.raises(ValueError):
        model.predictive_check(gpu=False, lags=11)
    with pytest.raises(ValueError):
        model.cross_correlogram(lags=11, gpu=False)
    assert simulate.PGL_LAG_MAX == 256
