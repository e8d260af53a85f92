"""model.simulate() on the GPU (pgl_simulate) against the NumPy path of the same law (pyglm_amd/simulate.py): the same bits for the count and
spike models at every kernel shape (one workgroup; lanes in groups per neuron; rows of Wm in registers on a grid of workgroups; rings in global
memory; x too wide for LDS), replicate independence, chunking, continuation, forecasts, the sums, the negative-binomial cap and the predictive
check.  Every case stays below 1e7 draws: a decision within an ulp of its threshold -- where libm and the device's math library may differ -- is
then expected less than 1e-8 times, and bit-equality is the honest condition."""
import numpy as np
import pytest

from pyglm_amd import simulate
from pyglm_amd._lib import PglError
from pyglm_amd.models import NonlinearAutoregressiveModel
from pyglm_amd.regression import (SparseBernoulliRegression, SparseBinomialRegression, SparseGaussianRegression,
                                  SparseNegativeBinomialRegression)
from pyglm_amd.utils.basis import cosine_basis

pytestmark = pytest.mark.gpu

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


def _both(model, T, **kw):
    return model.simulate(T, gpu=True, **kw), model.simulate(T, gpu=False, **kw)


def _assert_same(d, h, exact=True):
    assert d.Y.shape == h.Y.shape and d.Y.dtype == np.float64
    for name in ("Y", "sum", "sumsq", "history"):
        if exact:
            assert np.array_equal(getattr(d, name), getattr(h, name)), name
        else:
            np.testing.assert_allclose(getattr(d, name), getattr(h, name), rtol=1e-10, atol=1e-12, err_msg=name)
    assert (d.t0, d.t1) == (h.t0, h.t1)


@pytest.mark.parametrize("N,B,L,kinds,R,T", [
    (4, 1, 100, ("bernoulli",), 1, 3000),                      # one workgroup, a wave per neuron
    (4, 1, 100, ("negbin",), 3, 2000),
    (12, 3, 30, ("bernoulli",), 3, 2000),                      # one workgroup, lanes in groups of 16 per neuron
    (12, 3, 30, ("negbin",), 8, 1500),
    (12, 3, 30, ("binomial",), 3, 2000),
    (12, 3, 30, ("bernoulli", "negbin", "binomial"), 8, 2000),
    (64, 5, 100, ("bernoulli",), 8, 1500),                     # 16 workgroups, rows of Wm in registers, rings in LDS
    (64, 5, 100, ("binomial",), 3, 1500),
    (64, 5, 100, ("negbin", "bernoulli", "binomial"), 1, 2000),
    (64, 5, 100, ("bernoulli", "negbin"), 24, 300),            # the rings of 24 replicates do not fit in LDS
    (64, 5, 400, ("bernoulli", "negbin"), 5, 300),             # rings of 64 000 B and a basis of 16 000 B: together with x beyond the LDS
])
def test_device_is_the_host_path(N, B, L, kinds, R, T):
    assert R * T * N <= 10 ** 7
    model = _model(N, B, L, kinds, seed=N + R)
    d, h = _both(model, T, replicates=R, seed=1000 + N)
    _assert_same(d, h)
    assert d.Y.shape == (R, T, N) and 0 < d.Y.sum() and np.all(d.Y >= 0) and np.all(d.Y == np.floor(d.Y))
    assert len(np.unique(d.sum, axis=0)) == R                  # the replicates differ


def test_wide_model_whose_x_does_not_fit_in_lds():
    # N*B = 8400 > 8192: every workgroup reads x from the exchange buffer and streams its rows of Wm; the arrays go in directly
    N, B, L, R, T = 2100, 4, 10, 3, 30
    rng = np.random.default_rng(41)
    Wm = rng.standard_normal((N, N * B)) * (0.5 / np.sqrt(N)) * (rng.random((N, N * B)) < 0.5)
    kind = (np.arange(N) % 3 + (np.arange(N) % 3 > 0)).astype(np.int32)       # Bernoulli, negative binomial, binomial in turn
    par = np.where(kind == simulate.KIND_NEGBIN, 2.5, 10.0)
    Wm /= np.repeat(np.where(kind == simulate.KIND_BERNOULLI, 1.0, 5.0), B)[None, :]    # counts weigh as spikes do
    bias = np.where(kind == simulate.KIND_BERNOULLI, -2.0, -0.7) + 0.3 * rng.standard_normal(N)
    basis = cosine_basis(B, L=L) / L
    d, h = (simulate.simulate(Wm, bias, basis, kind, par, T, replicates=R, seed=42, on_device=dev) for dev in (True, False))
    _assert_same(d, h)
    assert all(d.Y[:, :, kind == k].sum() > 0 for k in (0, 2, 3)) and d.Y[:, :, kind == 3].max() <= 10


@pytest.mark.parametrize("N,B,L,R,T", [(5, 2, 30, 3, 3000), (96, 3, 40, 8, 1500)])
def test_gaussian_parity(N, B, L, R, T):
    model = _model(N, B, L, ("gaussian",), seed=31, w_scale=0.5 / np.sqrt(N * B))
    d, h = _both(model, T, replicates=R, seed=32)
    _assert_same(d, h, exact=False)
    assert np.std(d.Y) > 0.1


def test_one_call_of_six_replicates_is_six_calls_of_one():
    model = _model(64, 5, 100, ("bernoulli", "negbin", "binomial"), seed=5)
    d = model.simulate(800, replicates=6, seed=9, first_replicate=10, gpu=True)
    for r in range(6):
        one = model.simulate(800, replicates=1, seed=9, first_replicate=10 + r, gpu=True)
        assert np.array_equal(one.Y[0], d.Y[r]) and np.array_equal(one.sum[0], d.sum[r]) and np.array_equal(one.history[0], d.history[r])
    other = model.simulate(800, replicates=1, seed=10, first_replicate=10, gpu=True)
    assert not np.array_equal(other.Y[0], d.Y[0])


def test_chunks_that_do_not_divide_T(monkeypatch):
    model = _model(16, 2, 10, ("bernoulli", "negbin"), seed=7)
    whole = model.simulate(100, replicates=3, seed=8, gpu=True)
    monkeypatch.setattr(simulate, "chunk_bins", lambda N, B, R=1: 7)       # 14 launches of 7 bins and one of 2
    cut = model.simulate(100, replicates=3, seed=8, gpu=True)
    _assert_same(cut, whole)
    _assert_same(cut, model.simulate(100, replicates=3, seed=8, gpu=False))


@pytest.mark.parametrize("kinds,exact", [(("bernoulli", "negbin", "binomial"), True), (("gaussian",), False)])
def test_sums_without_paths_are_the_column_sums_of_the_paths(kinds, exact):
    model = _model(64, 5, 100, kinds, seed=11, w_scale=0.3 / np.sqrt(64))
    kept = model.simulate(1200, replicates=3, seed=12, gpu=True)
    bare = model.simulate(1200, replicates=3, seed=12, gpu=True, keep_paths=False)
    assert bare.Y is None and bare.sum.shape == bare.sumsq.shape == (3, 64)
    assert np.array_equal(bare.sum, kept.sum) and np.array_equal(bare.sumsq, kept.sumsq) and np.array_equal(bare.history, kept.history)
    if exact:
        assert np.array_equal(bare.sum, kept.Y.sum(axis=1)) and np.array_equal(bare.sumsq, (kept.Y ** 2).sum(axis=1))
    else:
        np.testing.assert_allclose(bare.sum, kept.Y.sum(axis=1), rtol=1e-12, atol=1e-12 * 1200)
        np.testing.assert_allclose(bare.sumsq, (kept.Y ** 2).sum(axis=1), rtol=1e-12)
    np.testing.assert_allclose(bare.rate(), kept.Y.mean(axis=1), rtol=1e-12, atol=1e-15)


def test_continuation_from_the_returned_history():
    model = _model(64, 5, 100, ("bernoulli", "negbin"), seed=13)
    whole = model.simulate(700, replicates=3, seed=14, gpu=True)
    first = model.simulate(250, replicates=3, seed=14, gpu=True)             # 250 is no multiple of L = 100: the ring is mid-way
    second = model.simulate(450, replicates=3, seed=14, gpu=True, history=first)
    assert (second.t0, second.t1) == (250, 700)
    assert np.array_equal(np.concatenate([first.Y, second.Y], axis=1), whole.Y)
    assert np.array_equal(second.history, whole.history) and np.array_equal(first.sum + second.sum, whole.sum)
    # the rows alone, with the origin given
    again = model.simulate(450, replicates=3, seed=14, gpu=True, history=first.history, t0=250)
    assert np.array_equal(again.Y, second.Y)


def test_forecast_from_the_last_rows_of_a_data_set():
    model = _model(12, 3, 30, ("bernoulli", "binomial"), seed=15)
    data = model.simulate(500, seed=16, gpu=False).Y[0]
    d, h = _both(model, 400, replicates=3, seed=17, history=data[-30:], t0=500)
    _assert_same(d, h)
    assert np.array_equal(d.history, d.Y[:, -30:])
    short, short_h = _both(model, 50, replicates=3, seed=17, history=data[-7:])      # fewer than L rows: preceded by silence
    _assert_same(short, short_h)
    assert not np.array_equal(short.Y, model.simulate(50, replicates=3, seed=17, gpu=True).Y)


def test_an_exploding_count_model_is_an_error_and_the_next_call_works():
    model = _model(64, 5, 100, ("bernoulli", "negbin"), seed=19)
    good = model.simulate(50, replicates=2, seed=20, gpu=True)
    model._adopt_state()[2][5, 0] = 40.0                                      # neuron 5 is negative binomial: its walk cannot end
    with pytest.raises(PglError) as err:
        model.simulate(50, replicates=2, seed=20, first_replicate=3, gpu=True)
    assert "neuron 5" in str(err.value) and "bin 0" in str(err.value) and ("replicate 3" in str(err.value) or "replicate 4" in str(err.value))
    with pytest.raises(PglError) as err_h:
        model.simulate(50, replicates=2, seed=20, first_replicate=3, gpu=False)
    assert "neuron 5" in str(err_h.value) and "bin 0" in str(err_h.value) and "replicate 3" in str(err_h.value)
    model._adopt_state()[2][5, 0] = -0.5
    fixed, fixed_h = _both(model, 50, replicates=2, seed=20)
    _assert_same(fixed, fixed_h)
    assert good.Y.shape == fixed.Y.shape
    # the one-workgroup kernel ends its launch as well
    small = _model(4, 1, 100, ("negbin",), seed=21)
    small._adopt_state()[2][2, 0] = 40.0
    with pytest.raises(PglError) as err:
        small.simulate(2000, replicates=1, seed=22, gpu=True)
    assert "neuron 2" in str(err.value) and "replicate 0" in str(err.value)


def test_predictive_check_matches_the_host_path():
    model = _model(6, 2, 20, ("bernoulli", "negbin"), seed=23)
    model.add_data(model.simulate(1500, seed=24, gpu=False).Y[0])
    out = []
    for gpu in (True, False):
        ppc = model.predictive_check(replicates=8, seed=25, gpu=gpu)
        for _ in range(3):
            ppc.collect()
        assert ppc.rates.shape == ppc.fanos.shape == (24, 6)
        out.append(ppc)
    for stat in ("rate", "fano"):
        assert np.array_equal(out[0].pvalue(stat), out[1].pvalue(stat))
    assert np.array_equal(out[0].rates, out[1].rates)
    assert np.array_equal(out[0].rate_quantiles([0.1, 0.9]), out[1].rate_quantiles([0.1, 0.9]))


def test_memory_for_the_paths_is_checked_before_allocating():
    model = _model(64, 5, 100, ("bernoulli",), seed=27)
    with pytest.raises(PglError) as err:
        model.simulate(2 ** 30, replicates=64, seed=1, gpu=True)             # 32 TiB of paths
    assert str(8 * 64 * 2 ** 30 * 64) in str(err.value)


def test_full_size_runs_and_its_prefix_is_the_host_path():
    N, B, L, R, T = 1024, 5, 100, 8, 2000
    model = _model(N, B, L, ("bernoulli",), seed=29, w_scale=1.0 / np.sqrt(N))
    d = model.simulate(T, replicates=R, seed=30, keep_paths=False, gpu=True)
    assert d.Y is None and d.sum.shape == (R, N) and np.all(d.sum > 0) and np.all(d.sum == d.sumsq)
    head = model.simulate(200, replicates=1, seed=30, gpu=True)
    h = model.simulate(200, replicates=1, seed=30, gpu=False)
    assert np.array_equal(head.Y, h.Y) and 0 < h.Y.sum() < h.Y.size
    # replicate 0 of the long run went through the same first 200 bins: its final history continues head's trajectory
    rest = model.simulate(T - 200, replicates=1, seed=30, history=head, keep_paths=False, gpu=True)
    assert np.array_equal(rest.history[0], d.history[0]) and np.array_equal(head.sum[0] + rest.sum[0], d.sum[0])
