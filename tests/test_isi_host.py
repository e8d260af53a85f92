"""The inter-spike-interval statistics on the host: simulate.isi_host -- the definition -- against a per-bin loop; the block-by-block fold of
simulate(isi=D, gpu=False) against isi_host of the kept path; PredictiveCheck(isi=D) against a brute-force computation over stacked
densities; and that the statistic flags a model without refractoriness which the rate does not."""
import functools

import numpy as np
import pytest

from pyglm_amd import simulate
from pyglm_amd.models import NonlinearAutoregressiveModel, SparseBernoulliGLM
from pyglm_amd.regression import SparseBernoulliRegression, SparseGaussianRegression
from pyglm_amd.utils.basis import cosine_basis
from tests._oracle_engine import OracleEngine
from tests.test_simulate_host import _mixed_model


def isi_loop(Y, D):
    """the definition, bin by bin"""
    T, N = Y.shape
    hist, moments = np.zeros((N, D), dtype=np.int64), np.zeros((N, 3), dtype=np.int64)
    for n in range(N):
        last = None
        for t in range(T):
            if Y[t, n] > 0:
                if last is not None:
                    d = t - last
                    hist[n, min(d, D) - 1] += 1
                    moments[n] += (1, d, d * d)
                last = t
    return hist, moments


def crafted_columns(T):
    """silent; one event; events at the first and last row only; every bin; values of {0, 1, 2, 5, -1, NaN}"""
    rng = np.random.default_rng(T)
    cols = np.zeros((T, 5))
    cols[T // 3, 1] = 1.0
    cols[0, 2] = cols[T - 1, 2] = 1.0
    cols[:, 3] = 1.0
    cols[:, 4] = rng.choice([0.0, 1.0, 2.0, 5.0, -1.0, np.nan], size=T)
    return cols


@pytest.mark.parametrize("T,D", [(1, 2), (2, 2), (300, 8), (300, 256), (700, 16)])
def test_isi_host_is_the_per_bin_loop(T, D):
    rng = np.random.default_rng(T + D)
    Y = np.concatenate([crafted_columns(T), (rng.random((T, 6)) < [0.01, 0.05, 0.2, 0.5, 0.9, 0.99]).astype(float)], axis=1)
    hist, moments = simulate.isi_host(Y, D)
    want = isi_loop(Y, D)
    assert hist.dtype == moments.dtype == np.int64 and hist.shape == (11, D) and moments.shape == (11, 3)
    assert np.array_equal(hist, want[0]) and np.array_equal(moments, want[1])
    assert np.array_equal(hist.sum(axis=1), moments[:, 0])
    assert not hist[:2].any() and list(moments[0]) == list(moments[1]) == [0, 0, 0]
    if T > 1:
        assert list(moments[2]) == [1, T - 1, (T - 1) ** 2] and hist[2, min(T - 1, D) - 1] == 1
        assert list(moments[3]) == [T - 1, T - 1, T - 1] and hist[3, 0] == T - 1


def test_the_chunked_fold_with_since_is_the_definition():
    T, D = 800, 16
    Y = np.concatenate([crafted_columns(T), (np.random.default_rng(3).random((T, 65)) < 0.07).astype(float)], axis=1)
    N = Y.shape[1]
    hist, moments, since = np.zeros((1, N, D), dtype=np.int64), np.zeros((1, N, 3), dtype=np.int64), np.full((1, N), -1, dtype=np.int64)
    done = 0
    for cut in (1, 255, 513, T):
        simulate._isi_fold_host(hist, moments, since, Y[None, done:cut])
        done = cut
        want = simulate.isi_host(Y[:done], D)
        assert np.array_equal(hist[0], want[0]) and np.array_equal(moments[0], want[1])
        ev = [np.flatnonzero(Y[:done, n] > 0) for n in range(N)]
        assert since[0].tolist() == [done - 1 - e[-1] if e.size else -1 for e in ev]


@functools.lru_cache(maxsize=None)
def _whole():
    model = _mixed_model()
    whole = model.simulate(300, replicates=3, seed=4, gpu=False, isi=16)
    return model, whole


def test_simulate_folds_the_intervals_of_its_paths(monkeypatch):
    model, whole = _whole()
    assert whole.isi.shape == (3, 6, 16) and whole.isi_moments.shape == (3, 6, 3) and whole.isi.dtype == whole.isi_moments.dtype == np.int64
    ref = [simulate.isi_host(whole.Y[r], 16) for r in range(3)]
    assert all(np.array_equal(whole.isi[r], ref[r][0]) and np.array_equal(whole.isi_moments[r], ref[r][1]) for r in range(3))
    assert (whole.isi_moments[:, :, 0] > 50).sum() >= 15 and whole.isi_moments[:, :, 0].min() < 2      # (one neuron is nearly silent)
    monkeypatch.setattr(simulate, "HOST_BLOCK_BINS", 37)       # the rolling buffer wraps: the fold goes block by block with the carry
    for lags in (0, 5):
        bare = model.simulate(300, replicates=3, seed=4, gpu=False, keep_paths=False, isi=16, lags=lags)
        assert bare.Y is None and np.array_equal(bare.isi, whole.isi) and np.array_equal(bare.isi_moments, whole.isi_moments)
        if lags:
            assert np.array_equal(bare.lagged, np.stack([simulate.lagged_products_host(whole.Y[r], lags) for r in range(3)]))
    M, sd, sd2 = (whole.isi_moments[..., k].astype(float) for k in range(3))
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(whole.isi_density(), np.where(M[..., None] > 0, whole.isi / M[..., None], np.nan), equal_nan=True)
        np.testing.assert_allclose(whole.isi_mean(), np.where(M > 0, sd / M, np.nan), rtol=1e-15)
        np.testing.assert_allclose(whole.isi_cv(), np.where(M > 1, np.sqrt(sd2 / M - (sd / M) ** 2) / (sd / M), np.nan), rtol=1e-9)
    plain = model.simulate(50, gpu=False)
    assert plain.isi is None and plain.isi_moments is None
    with pytest.raises(ValueError):
        plain.isi_cv()


def test_undefined_densities_and_cvs_are_nan():
    hist = np.array([[0, 0], [1, 0], [1, 1]])
    moments = np.array([[0, 0, 0], [1, 1, 1], [2, 4, 10]])
    d = simulate.isi_density(hist, moments)
    assert np.isnan(d[0]).all() and d[1].tolist() == [1.0, 0.0] and d[2].tolist() == [0.5, 0.5]
    cv = simulate.isi_cv(moments)
    assert np.isnan(cv[:2]).all() and cv[2] == np.sqrt(5.0 - 4.0) / 2.0
    assert np.isnan(simulate.isi_mean(moments)[0]) and simulate.isi_mean(moments)[2] == 2.0


def test_a_continued_simulation_counts_its_own_bins_only():
    model, whole = _whole()
    first = model.simulate(100, replicates=3, seed=4, gpu=False, isi=16)
    second = model.simulate(200, replicates=3, seed=4, gpu=False, isi=16, history=first)
    assert np.array_equal(np.concatenate([first.Y, second.Y], axis=1), whole.Y)
    for r in range(3):
        h, m = simulate.isi_host(whole.Y[r, 100:], 16)
        assert np.array_equal(second.isi[r], h) and np.array_equal(second.isi_moments[r], m)
    # the intervals across the cut are in neither call
    assert np.all(first.isi_moments[..., 0] + second.isi_moments[..., 0] <= whole.isi_moments[..., 0])
    assert (first.isi_moments[..., 0] + second.isi_moments[..., 0] < whole.isi_moments[..., 0]).any()
    empty = model.simulate(0, replicates=3, gpu=False, isi=16)
    assert empty.isi.shape == (3, 6, 16) and not empty.isi.any() and not empty.isi_moments.any()


def test_check_isi_bins_refusals():
    assert simulate.PGL_ISI_MAX_BINS == 256
    assert [simulate.check_isi_bins(v) for v in (0, 2, 64, 256)] == [0, 2, 64, 256]
    for bad in (-1, 1, 257, 1000):
        with pytest.raises(ValueError):
            simulate.check_isi_bins(bad)
    model = _mixed_model()
    with pytest.raises(ValueError):
        model.simulate(10, gpu=False, isi=1)
    with pytest.raises(ValueError):
        model.simulate(10, gpu=False, isi=257)
    with pytest.raises(ValueError):
        simulate.isi_host(np.zeros((5, 2)), 0)


def test_a_gaussian_neuron_is_refused_by_name():
    N, B = 4, 2
    np.random.seed(0)
    regs = [SparseBernoulliRegression(N, B) for _ in range(N)]
    regs[2] = SparseGaussianRegression(N, B, eta=0.1)
    model = NonlinearAutoregressiveModel(N, regs, B=B)
    assert model.simulate(10, gpu=False).Y.shape == (1, 10, N)             # without isi the model simulates
    with pytest.raises(ValueError, match="neuron 2"):
        model.simulate(10, gpu=False, isi=8)
    model.data_list.append((None, np.zeros((10, N))))
    with pytest.raises(ValueError, match="neuron 2"):
        model.isi_histogram(bins=8, gpu=False)
    with pytest.raises(ValueError, match="neuron 2"):
        model.predictive_check(gpu=False, isi=8)


# ---- the predictive check
def _pvalue(rep, obs):
    ok = ~np.isnan(rep)
    M = ok.sum(axis=0)
    with np.errstate(invalid="ignore"):
        ge, le = (ok & (rep >= obs)).sum(axis=0), (ok & (rep <= obs)).sum(axis=0)
    return ge, le, M, np.where(np.isnan(obs), np.nan, np.minimum(1.0, 2.0 * np.minimum(1 + ge, 1 + le) / (M + 1.0)))


def test_predictive_check_of_the_intervals_is_the_brute_force_computation():
    N, B, L, T, S, R, D = 6, 2, 20, 600, 3, 4, 8
    np.random.seed(0)
    model = SparseBernoulliGLM(N, basis=cosine_basis(B, L=L) / L, regression_kwargs=dict(mu_b=-2.0, S_b=0.1), engine_factory=OracleEngine, seed=1)
    A, W, b = model._adopt_state()
    rng = np.random.default_rng(1)
    W[...] = 0.5 * rng.standard_normal(W.shape)
    b[:, 0] = -2.0 + 0.2 * rng.standard_normal(N)
    b[5, 0] = -6.5                                              # a neuron that has no interval in some replicates
    data = model.simulate(T, seed=82, gpu=False).Y[0]
    model.add_data(data)
    ppc = model.predictive_check(replicates=R, seed=7, gpu=False, isi=D)
    for _ in range(S):
        ppc.collect()
    hist, moments = simulate.isi_host(data, D)
    assert np.array_equal(model.isi_histogram(bins=D, gpu=False)[0], hist)
    obs_d, obs_cv = simulate.isi_density(hist, moments), simulate.isi_cv(moments)
    assert np.array_equal(ppc.observed["isi"], obs_d, equal_nan=True) and np.array_equal(ppc.observed["cv"], obs_cv, equal_nan=True)
    dens, cvs = [], []
    for k in range(S):
        sim = model.simulate(T, replicates=R, seed=7, first_replicate=k * R, keep_paths=True, gpu=False)
        for r in range(R):
            h, m = simulate.isi_host(sim.Y[r], D)
            dens.append(simulate.isi_density(h, m))
            cvs.append(simulate.isi_cv(m))
    dens, cvs = np.stack(dens), np.stack(cvs)
    assert np.isnan(dens[:, 5]).any() and not np.isnan(dens[:, :5]).any()
    ge, le, M, p = _pvalue(dens, obs_d)
    state = ppc._isi_state()
    assert np.array_equal(state[0], ge) and np.array_equal(state[1], le) and np.array_equal(state[2], M)
    assert ppc.pvalue("isi").shape == (N, D) and np.array_equal(ppc.pvalue("isi"), p, equal_nan=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(M > 0, np.nansum(dens, axis=0) / np.maximum(M, 1), np.nan)
        dev = np.where(np.isnan(dens), 0.0, dens - np.where(M > 0, mean, 0.0))
        std = np.where(M > 1, np.sqrt((dev * dev).sum(axis=0) / np.maximum(M - 1.0, 1.0)), np.nan)
    np.testing.assert_allclose(ppc.isi_mean, mean, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ppc.isi_std, std, rtol=0, atol=1e-12)
    assert np.array_equal(ppc.cvs, cvs, equal_nan=True) and ppc.cvs.shape == (S * R, N)
    assert np.array_equal(ppc.pvalue("cv"), _pvalue(cvs, obs_cv)[3], equal_nan=True) and ppc.pvalue("cv").shape == (N,)
    assert ppc.cv_quantiles([0.1, 0.9]).shape == (2, N)
    with pytest.raises(ValueError, match="'isi'"):
        ppc.pvalue("median")
    bare = model.predictive_check(replicates=R, seed=7, gpu=False)
    bare.collect()
    for stat in ("isi", "cv"):
        with pytest.raises(ValueError):
            bare.pvalue(stat)


def test_the_interval_density_sees_refractoriness_where_the_rate_does_not():
    """Data from a model whose self-weights make a spike in the bin after a spike nearly impossible (-12 on the previous bin).  A state without
    those self-weights, its biases refitted so that every neuron fires at the data's rate -- what a fit without self-coupling arrives at --
    passes the rate check and fails the first cell of the interval density (the data have no interval of one bin, its replicates have them at
    about the firing rate) with the smallest p-value the estimator attains; the generating state passes both."""
    N, B, T, S, R, D = 5, 2, 1500, 3, 8, 8
    np.random.seed(0)
    basis = np.eye(4)[:, :B]                                    # basis function 0 = the previous bin, 1 = the one before it
    model = SparseBernoulliGLM(N, basis=basis, regression_kwargs=dict(mu_b=-1.0, S_b=0.1), engine_factory=OracleEngine, seed=1)
    A, W, b = model._adopt_state()
    rng = np.random.default_rng(5)
    A[...] = True
    W[...] = 0.1 * rng.standard_normal(W.shape)
    W[np.arange(N), np.arange(N), 0] = -12.0
    b[:, 0] = -1.0 + 0.2 * rng.standard_normal(N)
    data = model.simulate(T, seed=11, gpu=False).Y[0]
    assert simulate.isi_host(data, D)[0][:, 0].sum() == 0
    model.add_data(data)
    p_min = 2.0 / (S * R + 1)

    def check():
        ppc = model.predictive_check(replicates=R, seed=3, gpu=False, isi=D)
        for _ in range(S):
            ppc.collect()
        return ppc

    true = check()
    assert (true.pvalue("isi")[:, 0] > p_min).sum() >= N - 1, true.pvalue("isi")[:, 0]
    W_true, b_true = W.copy(), b.copy()
    W[np.arange(N), np.arange(N), 0] = 0.0
    rate = data.mean(axis=0)
    b[:, 0] = np.log(rate / (1.0 - rate))
    flat = check()
    assert np.all(flat.pvalue("isi")[:, 0] == p_min), flat.pvalue("isi")[:, 0]
    assert (flat.pvalue("rate") > p_min).sum() >= N - 1, flat.pvalue("rate")
    W[...], b[...] = W_true, b_true
