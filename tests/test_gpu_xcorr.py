"""The lagged products on the GPU (pgl_lagged_products, pyglm_amd/csrc/pgl_xcorr.hip) against their definition, simulate.lagged_products_host:
the int8 mode bit for bit -- below a tile, across tiles, lags that are no multiples of 4 or 16, rows that are no multiple of 64, K close to
rows, chunks that compose, sums beyond 2^31, the range check that leaves S alone --, the fp64 mode bit for bit on integers and within the
a-priori bound of a sum of `rows` products on real data; then model.simulate(lags=K), its fp64 fallback for counts beyond 127, and
PredictiveCheck(lags=K) against the NumPy path."""
import functools

import numpy as np
import pytest

from pyglm_amd import simulate
from pyglm_amd.models import NonlinearAutoregressiveModel
from pyglm_amd.regression import (SparseBernoulliRegression, SparseBinomialRegression, SparseGaussianRegression,
                                  SparseNegativeBinomialRegression)
from pyglm_amd.utils.basis import cosine_basis

pytestmark = pytest.mark.gpu

I8, F64 = simulate.LAG_I8, simulate.LAG_F64
SHAPES = [(4, 1, 100), (12, 17, 1000), (20, 5, 333), (70, 33, 2049), (16, 64, 70)]      # (N, K, rows)


def _device_products(Y, K, mode, cuts=None, S0=None):
    """pgl_lagged_products on Y (R, T, N), as one call or cut into the chunks `cuts` (accumulate = 1 after the first, or from the start on a
    given S0) -> (S (R, K, N, N), status (4,)) as NumPy arrays"""
    import torch
    from pyglm_amd._lib import call, load, ptr
    R, T, N = Y.shape
    Y_d = torch.from_numpy(np.array(Y, dtype=np.float64)).cuda()
    S = torch.full((R, K, N, N), float("nan"), dtype=torch.float64, device="cuda") if S0 is None else torch.from_numpy(S0.copy()).cuda()
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    done = 0
    for rows in (cuts or [T]):
        work = torch.empty(load().pgl_lagged_work_bytes(N, K, R, rows), dtype=torch.uint8, device="cuda")
        call("pgl_lagged_products", ptr(Y_d[0, done:]), N, T * N, rows, min(K - 1, done), N, K, R, ptr(S), K * N * N,
             1 if (done or S0 is not None) else 0, mode, ptr(work), ptr(status), None)
        done += rows
    assert done == T
    torch.cuda.synchronize()
    return S.cpu().numpy(), status.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _int_case(N, K, rows, R):
    """int8 inputs over the whole range and their lagged products by the definition"""
    rng = np.random.default_rng(N * 1000 + K + rows + R)
    Y = rng.integers(-127, 128, size=(R, rows, N)).astype(np.float64)
    Y[0, 0, 0], Y[-1, -1, -1] = -127.0, 127.0
    Y.setflags(write=False)
    ref = np.stack([simulate.lagged_products_host(Y[r], K) for r in range(R)])
    ref.setflags(write=False)
    return Y, ref


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("N,K,rows", SHAPES)
def test_int8_mode_is_the_definition_bit_for_bit(N, K, rows, R):
    Y, ref = _int_case(N, K, rows, R)
    S, status = _device_products(Y, K, I8)
    assert status[0] == 0
    assert np.array_equal(S, ref)


def test_int8_chunks_compose_to_the_whole_series():
    N, K, rows = 70, 33, 2049
    Y, ref = _int_case(N, K, rows, 3)
    S, status = _device_products(Y, K, I8, cuts=[700, 1, 1348])
    assert status[0] == 0 and np.array_equal(S, ref)
    # and onto sums that are already there
    S0 = np.random.default_rng(1).integers(-1000, 1000, size=ref.shape).astype(np.float64)
    S, _ = _device_products(Y, K, I8, S0=S0)
    assert np.array_equal(S, S0 + ref)


def test_int8_sums_beyond_the_int32_range_are_exact():
    N, K, rows = 16, 2, 140000
    S, status = _device_products(np.full((1, rows, N), 127.0), K, I8)
    assert status[0] == 0 and 127 * 127 * rows > 2 ** 31
    for l in range(K):
        want = 127 * 127 * (rows - l)
        assert all(int(v) == want and v == float(want) for v in S[0, l].ravel())


@pytest.mark.parametrize("bad", [128.0, 0.5, -128.0, float("nan")])
def test_int8_mode_refuses_what_is_no_int8_and_leaves_S_alone(bad):
    N, K, rows, R = 20, 5, 333, 3
    Yc, ref = _int_case(N, K, rows, R)
    Y = Yc.copy()
    Y[1, 200, 13] = bad
    S0 = np.random.default_rng(2).standard_normal(ref.shape)
    for given in (S0, None):                                  # accumulate = 1 onto S0; accumulate = 0 onto the NaN fill
        S, status = _device_products(Y, K, I8, S0=given)
        assert list(status) == [3, 200, 1, 13]
        assert np.array_equal(S, S0) if given is not None else np.all(np.isnan(S))
    # the next valid call works, and the fp64 mode takes the refused array (a NaN aside)
    S, status = _device_products(Yc, K, I8)
    assert status[0] == 0 and np.array_equal(S, ref)
    if bad == 128.0 or bad == -128.0:
        S, status = _device_products(Y, K, F64)
        assert status[0] == 0 and np.array_equal(S, np.stack([simulate.lagged_products_host(Y[r], K) for r in range(R)]))


@pytest.mark.parametrize("N,K,rows", [(12, 17, 1000), (21, 5, 333), (70, 33, 2049)])
def test_fp64_mode_is_exact_on_integers(N, K, rows):
    rng = np.random.default_rng(rows)
    Y = rng.integers(-3000, 3000, size=(2, rows, N)).astype(np.float64)
    ref = np.stack([simulate.lagged_products_host(Y[r], K) for r in range(2)])
    S, status = _device_products(Y, K, F64)
    assert status[0] == 0 and np.abs(Y).max() > 127 and np.array_equal(S, ref)
    S, _ = _device_products(Y, K, F64, cuts=[rows // 3, 1, rows - rows // 3 - 1])
    assert np.array_equal(S, ref)


def _longdouble_products(Y, K):
    """(the lagged products of Y (T, N) in np.longdouble, those of |Y|)"""
    Yl = np.asarray(Y, dtype=np.longdouble)
    T = Yl.shape[0]
    ref = np.stack([Yl[:T - l].T @ Yl[l:] for l in range(K)])
    mag = np.stack([np.abs(Yl[:T - l]).T @ np.abs(Yl[l:]) for l in range(K)])
    return ref, mag


def _assert_within_summation_bound(S, Y, K):
    """|S - S_ref| <= (rows + 1) 2^-53 sum |y_i y_j|, cell by cell: the a-priori bound of a sum of `rows` products in any order"""
    ref, mag = _longdouble_products(Y, K)
    err = np.abs(S.astype(np.longdouble) - ref)
    bound = (Y.shape[0] + 1) * np.longdouble(2.0) ** -53 * mag
    assert np.all(err <= bound), float((err / bound).max())


@pytest.mark.parametrize("N,K,rows", [(12, 17, 1000), (70, 33, 2049)])
def test_fp64_mode_on_real_data_is_within_the_summation_bound(N, K, rows):
    Y = np.random.default_rng(N).standard_normal((1, rows, N))
    S, status = _device_products(Y, K, F64)
    assert status[0] == 0
    _assert_within_summation_bound(S[0], Y[0], K)
    S, _ = _device_products(Y, K, F64, cuts=[rows // 2, rows - rows // 2])
    _assert_within_summation_bound(S[0], Y[0], K)


# ---- the model
_MAKE = {
    "bernoulli": lambda N, B, i: SparseBernoulliRegression(N, B, mu_b=-2.0, S_b=0.1),
    "negbin": lambda N, B, i: SparseNegativeBinomialRegression(N, B, xi=(1.0, 2.5)[i % 2], mu_b=-1.0, S_b=0.1),
    "binomial": lambda N, B, i: SparseBinomialRegression(N, B, n=(1, 10, 64)[i % 3], mu_b=-1.0, S_b=0.1),
    "gaussian": lambda N, B, i: SparseGaussianRegression(N, B, eta=(0.3, 0.05)[i % 2], mu_b=0.0, S_b=0.1),
}


def _model(N, B, L, kinds, seed, w_scale=None):
    """a model whose neuron i is of kind kinds[i % len(kinds)], at a random sparse state"""
    np.random.seed(seed)
    regs = [_MAKE[kinds[i % len(kinds)]](N, B, i) for i in range(N)]
    model = NonlinearAutoregressiveModel(N, regs, basis=cosine_basis(B, L=L) / L)
    A, W, b = model._adopt_state()
    rng = np.random.default_rng(seed)
    A[...] = rng.random((N, N)) < 0.5
    W[...] = rng.standard_normal(W.shape) * (w_scale if w_scale is not None else 0.5 / np.sqrt(N))
    W /= np.array([getattr(r, "n", 4.0 if hasattr(r, "xi") else 1.0) for r in regs], dtype=float)[None, :, None]   # counts weigh as spikes do
    base = {"bernoulli": -2.0, "negbin": -0.5, "binomial": -1.0, "gaussian": 0.1}
    b[:, 0] = [base[kinds[i % len(kinds)]] for i in range(N)] + 0.3 * rng.standard_normal(N)
    return model


MODELS = [(12, 3, 30, ("bernoulli", "binomial"), 3, 2000, 20), (64, 5, 100, ("bernoulli",), 8, 1500, 50)]


@functools.lru_cache(maxsize=None)
def _model_case(case):
    """the model of MODELS[case] and its simulation on the NumPy path, lagged products included"""
    N, B, L, kinds, R, T, K = MODELS[case]
    model = _model(N, B, L, kinds, seed=N + R)
    host = model.simulate(T, replicates=R, seed=500 + N, gpu=False, lags=K)
    for a in (host.Y, host.lagged):
        a.setflags(write=False)
    return model, host


@pytest.mark.parametrize("case", range(len(MODELS)))
def test_simulate_on_the_device_folds_the_lagged_products_of_its_paths(case):
    N, B, L, kinds, R, T, K = MODELS[case]
    model, host = _model_case(case)
    sim = model.simulate(T, replicates=R, seed=500 + N, gpu=True, lags=K)
    assert sim.lagged.shape == (R, K, N, N) and sim.lag_redos == 0 and sim.Y.sum() > 0
    for r in range(R):
        assert np.array_equal(sim.lagged[r], simulate.lagged_products_host(sim.Y[r], K))
    assert np.array_equal(sim.Y, host.Y) and np.array_equal(sim.lagged, host.lagged)
    assert np.array_equal(sim.correlogram(), host.correlogram(), equal_nan=True)
    bare = model.simulate(T, replicates=R, seed=500 + N, gpu=True, lags=K, keep_paths=False)
    assert bare.Y is None and np.array_equal(bare.lagged, host.lagged) and np.array_equal(bare.history, host.history)
    plain = model.simulate(T, replicates=R, seed=500 + N, gpu=True)
    assert plain.lagged is None and np.array_equal(plain.Y, host.Y)


@pytest.mark.parametrize("case,chunk", [(0, 7), (0, 300), (1, 37), (1, 400)])
def test_simulate_folds_the_same_sums_whatever_the_chunks(case, chunk, monkeypatch):
    # 7 < K - 1 = 19 and 37 < K - 1 = 49: a chunk shorter than the rows kept before it; none of the four divides T
    N, B, L, kinds, R, T, K = MODELS[case]
    model, host = _model_case(case)
    assert T % chunk != 0
    monkeypatch.setattr(simulate, "chunk_bins", lambda N, B, R=1: chunk)
    for keep in (True, False):
        sim = model.simulate(T, replicates=R, seed=500 + N, gpu=True, lags=K, keep_paths=keep)
        assert np.array_equal(sim.lagged, host.lagged) and np.array_equal(sim.sum, host.sum)


def test_counts_beyond_127_are_folded_in_fp64():
    N, B, L, R, T, K = 12, 3, 30, 3, 600, 20
    model = _model(N, B, L, ("negbin",), seed=41, w_scale=0.02 / np.sqrt(N))
    model._adopt_state()[2][:, 0] = 3.0 + 0.1 * np.random.default_rng(42).standard_normal(N)
    before = simulate.LAG_REDOS
    sim = model.simulate(T, replicates=R, seed=43, gpu=True, lags=K)
    assert sim.Y.max() > 127
    assert sim.lag_redos > 0 and simulate.LAG_REDOS == before + sim.lag_redos
    for r in range(R):
        assert np.array_equal(sim.lagged[r], simulate.lagged_products_host(sim.Y[r], K))
    host = model.simulate(T, replicates=R, seed=43, gpu=False, lags=K)
    assert np.array_equal(sim.Y, host.Y) and np.array_equal(sim.lagged, host.lagged)
    # a count model that stays below 128 never leaves the int8 kernel
    calm = _model(N, B, L, ("negbin",), seed=41, w_scale=0.02 / np.sqrt(N))
    low = calm.simulate(T, replicates=R, seed=43, gpu=True, lags=K)
    assert low.Y.max() <= 127 and low.lag_redos == 0
    assert np.array_equal(low.lagged[0], simulate.lagged_products_host(low.Y[0], K))


def test_a_gaussian_model_is_folded_in_fp64_within_the_summation_bound():
    N, B, L, R, T, K = 12, 3, 30, 2, 1500, 20
    model = _model(N, B, L, ("gaussian", "bernoulli"), seed=31, w_scale=0.5 / np.sqrt(N * B))
    sim = model.simulate(T, replicates=R, seed=32, gpu=True, lags=K)
    assert np.std(sim.Y) > 0.1 and sim.lag_redos == 0
    for r in range(R):
        _assert_within_summation_bound(sim.lagged[r], sim.Y[r], K)
    host = model.simulate(T, replicates=R, seed=32, gpu=False, lags=K)
    np.testing.assert_allclose(sim.lagged, host.lagged, rtol=1e-9, atol=1e-9)        # (the two paths' Y agree to 1e-10: test_gpu_simulate.py)


def test_memory_for_the_lagged_products_is_checked_before_allocating():
    from pyglm_amd._lib import PglError
    N, R, K = 4096, 16, 256                                     # 512 GiB of sums
    with pytest.raises(PglError) as err:
        simulate.simulate(np.zeros((N, N)), np.zeros(N), np.ones((2, 1)), np.zeros(N, dtype=np.int32), np.zeros(N), 1000, replicates=R, seed=1,
                          keep_paths=False, on_device=True, lags=K)
    assert "lags" in str(err.value) and "replicates" in str(err.value)


def test_cross_correlogram_of_a_data_set():
    model = _model(12, 3, 30, ("bernoulli", "binomial"), seed=51)
    data = model.simulate(1200, seed=52, gpu=False).Y[0]
    model.add_data(data)
    d, h = model.cross_correlogram(lags=15, gpu=True), model.cross_correlogram(lags=15, gpu=False)
    assert d.shape == (15, 12, 12) and np.array_equal(d, h, equal_nan=True) and np.isfinite(d).any()


def test_predictive_check_with_lags_matches_the_host_path():
    N, R, K = 12, 4, 10
    model = _model(N, 3, 30, ("bernoulli", "binomial"), seed=61)
    model.add_data(model.simulate(1000, seed=62, gpu=False).Y[0])
    out = []
    for gpu in (True, False):
        ppc = model.predictive_check(replicates=R, seed=63, gpu=gpu, lags=K)
        for _ in range(3):
            ppc.collect()
        out.append(ppc)
    d, h = out
    assert d.observed["xcorr"].shape == (K, N, N) and np.array_equal(d.observed["xcorr"], h.observed["xcorr"], equal_nan=True)
    p = d.pvalue("xcorr")
    assert p.shape == (K, N, N) and np.array_equal(p, h.pvalue("xcorr"), equal_nan=True)
    assert np.nanmin(p) >= 2.0 / 13.0 and len(np.unique(p[~np.isnan(p)])) > 3
    np.testing.assert_allclose(d.xcorr_mean, h.xcorr_mean, rtol=0, atol=1e-12)
    np.testing.assert_allclose(d.xcorr_std, h.xcorr_std, rtol=0, atol=1e-12)
    for stat in ("rate", "fano"):
        assert np.array_equal(d.pvalue(stat), h.pvalue(stat), equal_nan=True)
