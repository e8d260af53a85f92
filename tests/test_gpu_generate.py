"""generate() on the GPU (pyglm_amd/simulate.py, pgl_generate): the same (X, Y) and the same final state of NumPy's global generator as
the host loop, at the sizes and shapes that exercise the one-workgroup kernel, the grid of workgroups, chunks that do not divide T, T < L,
and the full N = 1024 model.  Each Bernoulli seed is checked to be a fair exact test: no decision of the host trajectory lies within
1e-12 of its threshold."""
import time

import numpy as np
import pytest

from pyglm_amd import simulate
from pyglm_amd.models import NonlinearAutoregressiveModel, SparseGaussianGLM
from pyglm_amd.regression import SparseBernoulliRegression, SparseNegativeBinomialRegression
from pyglm_amd.utils.basis import cosine_basis
from pyglm_amd.utils.utils import logistic

pytestmark = pytest.mark.gpu


def _bernoulli_model(N, B, L, seed, w_scale=None, basis=None):
    np.random.seed(seed)
    basis = cosine_basis(B, L=L) / L if basis is None else basis
    regs = [SparseBernoulliRegression(N, B, rho=0.0, mu_b=-2.0, S_b=0.1) for _ in range(N)]
    model = NonlinearAutoregressiveModel(N, regs, basis=basis)
    _, W, b = model._adopt_state()
    rng = np.random.default_rng(seed)
    W[...] = rng.standard_normal(W.shape) * (w_scale if w_scale is not None else 2.0 / np.sqrt(N))
    b[:, 0] = -2.0 + 0.3 * rng.standard_normal(N)
    return model


def _min_margin(model, X, Y, state):
    """min |u - p| over the host trajectory: u replayed from the generator state before the call, p from (X, W, b)"""
    T, N = Y.shape
    rs = np.random.RandomState()
    rs.set_state(state)
    u = rs.rand(T, N)
    psi = X.reshape(T, -1).dot(model.weights.reshape(N, -1).T) + model.biases
    p = logistic(psi)
    assert np.array_equal(Y, (u < p).astype(float))
    return np.min(np.abs(u - p))


def _states_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _parity(model, T, seed):
    np.random.seed(seed)
    s0 = np.random.get_state()
    Xh, Yh = model.generate(keep=False, T=T, gpu=False)
    sh = np.random.get_state()
    np.random.seed(seed)
    Xd, Yd = model.generate(keep=False, T=T, gpu=True)
    sd = np.random.get_state()
    assert _min_margin(model, Xh, Yh, s0) > 1e-12, "the seed puts a decision within rounding of its threshold: not a fair exact test"
    assert Yd.shape == Yh.shape and Xd.shape == Xh.shape
    assert np.array_equal(Yd, Yh)
    np.testing.assert_allclose(Xd, Xh, rtol=1e-12, atol=1e-13)
    assert _states_equal(sd, sh)
    return Yh


@pytest.mark.parametrize("N,B,L,T,seed", [
    (4, 1, 100, 10000, 3),          # configs[0]-sized: the one-workgroup kernel
    (64, 5, 100, 20000, 4),         # a grid of 16 workgroups
    (300, 2, 20, 3000, 5),          # N a multiple of nothing: 75 workgroups of 4 neurons
    (8, 3, 100, 50, 6),             # T < L
])
def test_bernoulli_parity(N, B, L, T, seed):
    Y = _parity(_bernoulli_model(N, B, L, seed), T, seed + 100)
    assert 0 < Y.sum() < Y.size


def test_bernoulli_parity_g3_setup():
    # the set-up of golden G3 (reference test/test_generate.py:10-39): N = 2, B = 3, cosine_basis(3, L=10) / 10, weights from the prior
    np.random.seed(1)
    regs = [SparseBernoulliRegression(2, 3, mu_b=-2, S_b=0.1) for _ in range(2)]
    model = NonlinearAutoregressiveModel(2, regs, basis=cosine_basis(3, L=10) / 10)
    _parity(model, 1000, 11)


def test_chunks_that_do_not_divide_T(monkeypatch):
    model = _bernoulli_model(16, 2, 10, 7)
    monkeypatch.setattr(simulate, "chunk_bins", lambda N, B: 7)
    _parity(model, 100, 8)                                       # 14 chunks of 7 bins and one of 2


def test_length_one_basis_is_refused_by_both_paths():
    # flipud of a one-row basis is the basis itself: the reference's argument check (models.py:120) fails on either path, before any draw
    model = _bernoulli_model(4, 2, 1, 9, basis=np.ones((1, 2)))
    for gpu in (False, True):
        np.random.seed(0)
        s0 = np.random.get_state()
        with pytest.raises(AssertionError):
            model.generate(keep=False, T=20, gpu=gpu)
        assert _states_equal(np.random.get_state(), s0)


def test_wide_model_against_a_host_restatement():
    # N = 4096, B = 8: Wm is 1 GiB and streams from HBM every bin; only correctness is asked of it
    N, B, L, T = 4096, 8, 12, 24
    rng = np.random.default_rng(12)
    basis = cosine_basis(B, L=L) / L
    Wm = rng.standard_normal((N, N * B)) * (2.0 / np.sqrt(N))
    bias = -1.0 + 0.3 * rng.standard_normal(N)
    np.random.seed(13)
    Xd, Yd = simulate.generate(Wm, bias, basis, T, simulate.OBS_BERNOULLI)
    np.random.seed(13)
    U = np.random.rand(T, N)
    Y = np.zeros((T + L, N))
    margin = np.inf
    for t in range(L, T + L):
        x = Y[t - L:t].T.dot(basis[::-1]).reshape(-1)
        p = logistic(Wm.dot(x) + bias)
        Y[t] = U[t - L] < p
        margin = min(margin, np.min(np.abs(U[t - L] - p)))
        np.testing.assert_allclose(Xd[t - L].reshape(-1), x, rtol=1e-12, atol=1e-13)
    assert margin > 1e-12
    assert np.array_equal(Yd, Y[L:]) and 0 < Yd.sum() < Yd.size


def test_full_size_within_budget_and_its_prefix_matches_the_host_loop():
    N, B, L, T = 1024, 5, 100, 100000
    model = _bernoulli_model(N, B, L, 21, w_scale=1.0 / np.sqrt(N))
    np.random.seed(22)
    t = time.perf_counter()
    Xd, Yd = model.generate(keep=False, T=T, gpu=True)
    wall = time.perf_counter() - t
    assert wall < 60.0, wall
    assert Yd.shape == (T, N) and Xd.shape == (T, N, B)
    # row-major rand(T, N): the first 2000 bins see the same draws as a host run of 2000 bins
    np.random.seed(22)
    s0 = np.random.get_state()
    Xh, Yh = model.generate(keep=False, T=2000, gpu=False)
    assert _min_margin(model, Xh, Yh, s0) > 1e-12
    assert np.array_equal(Yd[:2000], Yh)
    np.testing.assert_allclose(Xd[:2000], Xh, rtol=1e-12, atol=1e-13)
    assert 0 < Yd.sum() < Yd.size


def _gaussian_model(N, B, L, seed):
    np.random.seed(seed)
    model = SparseGaussianGLM(N, basis=cosine_basis(B, L=L) / L, regression_kwargs=dict(eta=0.3))
    _, W, b = model._adopt_state()
    rng = np.random.default_rng(seed)
    W[...] = rng.standard_normal(W.shape) * (0.5 / np.sqrt(N * B))
    b[:, 0] = 0.2 * rng.standard_normal(N)
    return model


@pytest.mark.parametrize("N,B,L,T", [(5, 2, 30, 3000), (96, 3, 40, 1500)])
def test_gaussian_parity(N, B, L, T):
    model = _gaussian_model(N, B, L, 31)
    np.random.seed(32)
    Xh, Yh = model.generate(keep=False, T=T, gpu=False)
    sh = np.random.get_state()
    np.random.seed(32)
    Xd, Yd = model.generate(keep=False, T=T, gpu=True)
    assert _states_equal(np.random.get_state(), sh)
    np.testing.assert_allclose(Yd, Yh, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(Xd, Xh, rtol=1e-10, atol=1e-12)
    assert np.std(Yd) > 0.1


def test_reference_generate_tests_through_the_device():
    # reference test/test_generate.py:42-55 (lags with the identity basis) and :10-39 (X is the convolution of Y; means agree)
    np.random.seed(0)
    N, B = 2, 3
    regs = [SparseBernoulliRegression(N, B, mu_b=-2, S_b=0.1) for _ in range(N)]
    model = NonlinearAutoregressiveModel(N, regs, B=B)
    X, Y = model.generate(T=1000, keep=False, gpu=True)
    for n in range(N):
        for b in range(B):
            assert np.allclose(Y[:-(b + 1), n], X[(b + 1):, n, b])
    np.random.seed(1)
    regs = [SparseBernoulliRegression(N, B, mu_b=-2, S_b=0.1) for _ in range(N)]
    model = NonlinearAutoregressiveModel(N, regs, basis=cosine_basis(B, L=10) / 10)
    X, Y = model.generate(T=1000, keep=False, gpu=True)
    model.add_data(Y)
    assert np.allclose(X, np.asarray(model.data_list[0][0]))
    means = model.means
    model2 = NonlinearAutoregressiveModel(N, regs, basis=cosine_basis(B, L=10) / 10)
    model2.add_data(Y, X=X)
    assert np.allclose(means[0], model2.means[0])


def test_keep_adds_the_data_as_the_host_path_does():
    twins = [_bernoulli_model(32, 3, 25, 41) for _ in range(2)]
    for m, gpu in zip(twins, (True, False)):
        np.random.seed(42)
        m.generate(keep=True, T=1500, gpu=gpu)
    (Xd, Yd), (Xh, Yh) = twins[0].data_list[-1], twins[1].data_list[-1]
    assert np.array_equal(Yd, Yh)
    np.testing.assert_allclose(np.asarray(Xd), np.asarray(Xh), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(twins[0].log_likelihood(), twins[1].log_likelihood(), rtol=1e-10)


class _OwnRvs(SparseBernoulliRegression):
    def rvs(self, X=None, size=[], psi=None):
        return (np.random.rand(*psi.shape) < 0.5 * logistic(psi)).astype(float)


@pytest.mark.parametrize("cls", [SparseNegativeBinomialRegression, _OwnRvs])
def test_other_observation_models_keep_the_host_loop(cls):
    np.random.seed(51)
    N, B = 6, 2
    model = NonlinearAutoregressiveModel(N, [cls(N, B, mu_b=-1.0, S_b=0.1) for _ in range(N)], basis=cosine_basis(B, L=15) / 15)
    out = []
    for gpu in (None, False):
        np.random.seed(52)
        out.append(model.generate(keep=False, T=400, gpu=gpu) + (np.random.get_state(),))
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][0], out[1][0]) and _states_equal(out[0][2], out[1][2])
    with pytest.raises(ValueError):
        model.generate(keep=False, T=10, gpu=True)
