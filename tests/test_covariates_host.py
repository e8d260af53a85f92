"""External covariates on the host (pyglm_amd/covariates.py, the law the kernels of pgl_covariates.hip are held to): the conditional of beta
is the right Gaussian, the offset keeps its stated rounding, the rank exchange carries beta, and what cannot work is refused.  Runs without
a GPU; tests/test_gpu_covariates.py holds the kernels to these functions."""
import ctypes

import numpy as np
import pytest

from pyglm_amd import covariates as cov
from pyglm_amd import models

LD = np.longdouble


def _bernoulli_case(seed=3, T=40, K=2):
    """one neuron, fixed omega: S, omega, kappa = y - 1/2, psi_net, the offset o_old the 'sweep' ran under, a non-trivial prior"""
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((T, K))
    om = rng.uniform(0.05, 0.25, size=(T, 1))
    y = (rng.random((T, 1)) < 0.4).astype(float)
    psi_net = rng.standard_normal((T, 1))
    o_old = cov.offset_host(S, rng.standard_normal((1, K)))
    mu0 = np.array([0.3, -0.7])[:K]
    A = rng.standard_normal((K, K))
    Sigma0 = A.dot(A.T) + 0.5 * np.eye(K)
    return S, om, y - 0.5, psi_net, o_old, mu0, Sigma0


def test_conditional_draw_is_the_gaussian_conditional():
    """N = 1, K = 2, T = 40.  (i) over fixed normals -- z = 0 and the unit vectors -- the draw's mean is Lambda^-1 r and the draw's
    covariance M M' (M = the map from z to beta) is Lambda^-1, written out by hand, to 1e-12.  (ii) r and Lambda are the gradient and the
    negative Hessian at beta = 0 of the augmented log-density sum_t kappa_t psi_t - omega_t psi_t^2 / 2 + log N(beta; mu0, Sigma0), by
    central differences in long double (the function is quadratic: the differences are exact up to rounding at any step; step 1)."""
    S, om, kappa, psi_net, o_old, mu0, Sigma0 = _bernoulli_case()
    K = S.shape[1]
    _, _, Lambda0, h0 = cov.prior_terms(K, (mu0, Sigma0))
    kappa_reduced = kappa - om * o_old                                  # what the sweep under o_old leaves in Kappa
    Lam, r = cov.covariate_stats_host(S, om, kappa_reduced, o_old, psi_net)
    Lam_n, r_n = Lam[0] + Lambda0, r[0] + h0
    # (i)
    mean = cov.covariate_draw_host(Lam, r, Lambda0, h0, np.zeros((1, K)))[0]
    M = np.stack([cov.covariate_draw_host(Lam, r, Lambda0, h0, np.eye(K)[i:i + 1])[0] - mean for i in range(K)], axis=1)
    hand_cov = np.linalg.inv(Lam_n)
    hand_mean = hand_cov.dot(r_n)
    np.testing.assert_allclose(mean, hand_mean, rtol=1e-12, atol=1e-12 * np.abs(hand_mean).max())
    np.testing.assert_allclose(M.dot(M.T), hand_cov, rtol=1e-12, atol=1e-12 * np.abs(hand_cov).max())
    # (ii)
    Sl, oml, kl, pl = (np.asarray(v, dtype=LD) for v in (S, om[:, 0], kappa[:, 0], psi_net[:, 0]))
    L0l, mul = np.asarray(Lambda0, dtype=LD), np.asarray(mu0, dtype=LD)

    def f(beta):
        psi = pl + Sl.dot(beta)
        d = beta - mul
        return np.sum(kl * psi - oml * psi * psi / 2) - d.dot(L0l).dot(d) / 2
    e = np.eye(K, dtype=LD)
    z0 = np.zeros(K, dtype=LD)
    grad = np.array([(f(e[i]) - f(-e[i])) / 2 for i in range(K)], dtype=LD)
    hess = np.array([[(f(e[i] + e[j]) - f(e[i] - e[j]) - f(-e[i] + e[j]) + f(-e[i] - e[j])) / 4 for j in range(K)] for i in range(K)], dtype=LD)
    assert f(z0) == f(z0)
    np.testing.assert_allclose(r_n, grad.astype(np.float64), rtol=1e-12, atol=1e-12 * np.abs(r_n).max())
    np.testing.assert_allclose(Lam_n, -hess.astype(np.float64), rtol=1e-12, atol=1e-12 * np.abs(Lam_n).max())


def test_step_composes_stats_and_draw_over_data_sets():
    rng = np.random.default_rng(5)
    N, K = 3, 4
    sets = []
    for T in (17, 30):
        S = rng.standard_normal((T, K))
        sets.append((S, rng.uniform(0.05, 0.25, (T, N)), rng.standard_normal((T, N)), cov.offset_host(S, rng.standard_normal((N, K))),
                     rng.standard_normal((T, N))))
    _, _, Lambda0, h0 = cov.prior_terms(K)
    z = rng.standard_normal((N, K))
    parts = [cov.covariate_stats_host(*d) for d in sets]
    want = cov.covariate_draw_host(parts[0][0] + parts[1][0], parts[0][1] + parts[1][1], Lambda0, h0, z)
    np.testing.assert_array_equal(cov.covariate_step_host(sets, Lambda0, h0, z), want)
    # the long-double statistics agree with the fp64 ones to the sums' rounding
    Ll, rl = cov.covariate_stats_host(*sets[0], dtype=LD)
    assert Ll.dtype == LD and np.allclose(Ll.astype(np.float64), parts[0][0], rtol=1e-12) and np.allclose(rl.astype(np.float64), parts[0][1], rtol=1e-11, atol=1e-12)
    # tri_pack / tri_unpack: the layout of the device's Lambda
    P = cov.tri_pack(parts[0][0])
    assert P.shape == (N, K * (K + 1) // 2) and P[1, 2 * 3 // 2 + 1] == parts[0][0][1, 2, 1]
    U = cov.tri_unpack(P, K)                                           # (symmetric, from the lower triangle)
    np.testing.assert_array_equal(np.tril(U), np.tril(parts[0][0])), np.testing.assert_array_equal(U, U.transpose(0, 2, 1))


@pytest.mark.parametrize("T, N, K", [(1, 1, 1), (50, 7, 9), (33, 5, 32)])
def test_offset_host(T, N, K):
    """against S @ beta.T within 2 K 2^-53 sum |terms|; and the stated order: from 0.0, k ascending, product and sum rounded in turn"""
    rng = np.random.default_rng(T + N + K)
    S, beta = rng.standard_normal((T, K)) * 10.0 ** rng.integers(-3, 4, size=(T, K)), rng.standard_normal((N, K))
    o = cov.offset_host(S, beta)
    terms = np.abs(S[:, None, :] * beta[None, :, :]).sum(axis=2)
    assert o.shape == (T, N) and np.all(np.abs(o - S @ beta.T) <= 2 * K * 2.0 ** -53 * terms)
    want = np.zeros((T, N))
    for t in range(T):
        for n in range(N):
            acc = 0.0
            for k in range(K):
                acc = acc + S[t, k] * beta[n, k]
            want[t, n] = acc
    np.testing.assert_array_equal(o, want)


def test_draws_are_keyed_by_the_global_neuron_on_their_own_lane():
    from pyglm_amd.engine import make_draws
    z = cov.covariate_draws(7, 11, range(6), 3)
    np.testing.assert_array_equal(cov.covariate_draws(7, 11, [2, 3], 3), z[2:4])
    assert not np.array_equal(cov.covariate_draws(7, 12, [2], 3), z[2:3]) and cov.COV_LANE == 3
    assert not np.array_equal(make_draws(7, 11, [2], 2, 2)[2][0, :3], z[2])            # (lane 0: the sweep's own normals)


def _today_pack(N, B, a, W, b, eta, stats):
    """the packed rows as they were before covariates existed, written out from the documented layout"""
    D, nl = N * B, a.shape[0]
    rb = 8 * D + 16 + 8 * (1 + B + B * B) + -(-N // 8) * 8
    buf = np.zeros((nl, rb), dtype=np.uint8)
    buf[:, :8 * D] = np.ascontiguousarray(W).reshape(nl, -1).view(np.uint8)
    buf[:, 8 * D:8 * D + 8] = np.ascontiguousarray(b).reshape(nl, 1).view(np.uint8)
    buf[:, 8 * D + 8:8 * D + 16] = np.ascontiguousarray(eta).reshape(nl, 1).view(np.uint8)
    buf[:, 8 * D + 16:8 * D + 16 + 8 * (1 + B + B * B)] = np.ascontiguousarray(stats).reshape(nl, -1).view(np.uint8)
    buf[:, rb - -(-N // 8) * 8:rb - -(-N // 8) * 8 + N] = a.astype(np.uint8)
    return buf


def test_rank_exchange_carries_beta():
    N, B = 5, 2
    rng = np.random.default_rng(0)
    a, W, b = rng.random((3, N)) < 0.5, rng.standard_normal((3, N, B)), rng.standard_normal(3)
    eta, stats, beta = rng.random(3), rng.standard_normal((3, 1 + B + B * B)), rng.standard_normal((3, 3))
    m0 = models.SparseBernoulliGLM(N, B=B, seed=1)
    assert m0.K == 0 and m0.covariate_weights.shape == (N, 0)
    assert models.state_row_layout(N, B) == models.state_row_layout(N, B, 0)
    packed0 = m0._pack_rows_host(a, W, b, eta, stats)
    assert packed0.tobytes() == _today_pack(N, B, a, W, b, eta, stats).tobytes()        # K = 0: byte for byte today's rows
    m3 = models.SparseBernoulliGLM(N, B=B, seed=1, n_covariates=3)
    packed = m3._pack_rows_host(a, W, b, eta, stats, beta)
    assert packed.shape[1] == packed0.shape[1] + 24 and packed[:, :packed0.shape[1]].tobytes() == packed0.tobytes()
    a2, W2, b2, eta2, stats2, beta2 = m3._unpack_rows(packed)
    np.testing.assert_array_equal(beta2, beta)
    assert m0._unpack_rows(packed0)[5] is None
    np.testing.assert_array_equal(a2.astype(bool), a)
    np.testing.assert_array_equal(np.asarray(W2).reshape(3, N, B), W)
    np.testing.assert_array_equal(b2, b), np.testing.assert_array_equal(eta2, eta), np.testing.assert_array_equal(stats2, stats)


def test_state_carries_beta():
    m = models.SparseBernoulliGLM(4, B=2, seed=1, n_covariates=2)
    m.covariate_weights = np.arange(8.0).reshape(4, 2)
    st = m.get_state()
    m.covariate_weights = 0.0
    assert not m.covariate_weights.any()
    m.set_state(st)
    np.testing.assert_array_equal(m.covariate_weights, np.arange(8.0).reshape(4, 2))


def test_model_chain_on_the_cpu_engine():
    """the model's side on the oracle engine with covariates (tests/_covariate_engine.py): resample_model() draws beta behind the sweep from
    what that sweep left, the log-likelihood sees the offset, and set_state(get_state()) resumes the chain exactly, beta included"""
    from tests._covariate_engine import CovariateOracleEngine
    rng = np.random.default_rng(4)
    N, T, K = 3, 400, 2
    S = np.column_stack([np.sin(np.arange(T) / 7.0), rng.standard_normal(T)])
    bt = np.array([[1.0, 0.0], [-1.0, 0.5], [0.0, 1.0]])
    Y = (rng.random((T, N)) < 1 / (1 + np.exp(1.0 - cov.offset_host(S, bt)))).astype(float)
    m = models.SparseBernoulliGLM(N, B=1, seed=9, n_covariates=K, engine_factory=CovariateOracleEngine)
    m.add_data(Y, covariates=S)
    m.resample_model()
    eng = m.engine
    Om, Kp, off = eng.last
    a, W, b = m._local_state()
    want = cov.covariate_step_host([(S, Om[0], Kp[0], off[0], eng.psi_net(a, W, b, 0))], eng.cov_prior[2], eng.cov_prior[3],
                                   cov.covariate_draws(m.seed, 0, range(N), K))
    np.testing.assert_array_equal(m.covariate_weights, want)
    assert not off[0].any() and np.abs(want).min() > 0                    # the first sweep ran under beta = 0
    psi = eng.psi_net(a, W, b, 0) + cov.offset_host(S, want)
    np.testing.assert_allclose(m.log_likelihood(), np.sum(Y * psi - np.log1p(np.exp(psi))), rtol=1e-12)
    st = m.get_state()
    m.resample_model()
    after = (m.covariate_weights, m.weights, m.biases)
    m.set_state(st)
    np.testing.assert_array_equal(m.covariate_weights, want)
    m.resample_model()
    for x, y in zip(after, (m.covariate_weights, m.weights, m.biases)):
        np.testing.assert_array_equal(x, y)
    acc = m.summarize(rates=False)
    acc.collect()
    np.testing.assert_array_equal(acc.covariate_mean, m.covariate_weights)


def _chain_model(kind, N, K):
    """a model of each family whose resample_model() has a step BEHIND the covariate step: none (Bernoulli), eta (Gaussian), xi (negative
    binomial with xi_prior)"""
    from tests._covariate_engine import CovariateOracleEngine
    kw = dict(B=1, seed=9, n_covariates=K, engine_factory=CovariateOracleEngine)
    if kind == "gaussian":
        return models.SparseGaussianGLM(N, **kw)
    if kind == "negbin_xi":
        return models.SparseNegativeBinomialGLM(N, regression_kwargs=dict(S_w=2.0, mu_b=-1.5, xi=1.0, xi_prior=(2.0, 1.0)), **kw)
    return models.SparseBernoulliGLM(N, **kw)


@pytest.mark.parametrize("kind", ["bernoulli", "gaussian", "negbin_xi"])
def test_beta_survives_the_steps_behind_it(kind):
    """every observation model, Gaussian and xi-learning included: after each of three resample_model() calls the model's covariate_weights
    are the engine's beta and are covariate_step_host of what that sweep left -- the eta and xi steps that follow the covariate step leave
    beta alone (and themselves ran: eta / xi moved) --, and the next sweep runs under the offsets of exactly that beta"""
    rng = np.random.default_rng(6)
    N, T, K = 3, 200, 2
    S = np.column_stack([np.sin(np.arange(T) / 7.0), rng.standard_normal(T)])
    bt = np.array([[1.0, 0.0], [-1.0, 0.5], [0.0, 1.0]])
    o = cov.offset_host(S, bt)
    if kind == "gaussian":
        Y = 0.5 + o + 0.7 * rng.standard_normal((T, N))
    elif kind == "negbin_xi":
        Y = rng.negative_binomial(2.0, 1.0 / (1.0 + np.exp(-1.0 + o))).astype(np.float64)
    else:
        Y = (rng.random((T, N)) < 1 / (1 + np.exp(1.0 - o))).astype(float)
    m = _chain_model(kind, N, K)
    m.add_data(Y, covariates=S)
    eng = m.engine
    second = lambda: np.array([r.eta if kind == "gaussian" else getattr(r, "xi", 1.0) for r in m.regressions])
    prev = np.zeros((N, K))
    for sweep in range(3):
        before = second()
        m.resample_model()
        Om, Kp, off = eng.last
        np.testing.assert_array_equal(off[0], cov.offset_host(S, prev))                       # (the sweep ran under the beta before it)
        a, W, b = m._local_state()
        want = cov.covariate_step_host([(S, Om[0], Kp[0], off[0], eng.psi_net(a, W, b, 0))], eng.cov_prior[2], eng.cov_prior[3],
                                       cov.covariate_draws(m.seed, sweep, range(N), K))
        assert want.shape == (N, K) and len(np.unique(want)) == N * K
        np.testing.assert_array_equal(eng.beta, want)
        np.testing.assert_array_equal(m.covariate_weights, want)
        if kind != "bernoulli":
            assert np.all(second() != before)
        prev = want


def test_refusals():
    N, B, T = 3, 2, 20
    Y = np.zeros((T, N))
    with pytest.raises(ValueError, match="0 to 32"):
        models.SparseBernoulliGLM(N, B=B, n_covariates=33)
    with pytest.raises(ValueError, match="n_covariates=0"):
        models.SparseBernoulliGLM(N, B=B, covariate_prior=(np.zeros(2), np.eye(2)))
    with pytest.raises(ValueError, match="Sigma0"):
        models.SparseBernoulliGLM(N, B=B, n_covariates=2, covariate_prior=(np.zeros(2), np.eye(3)))
    m = models.SparseBernoulliGLM(N, B=B, seed=1, n_covariates=2)
    with pytest.raises(ValueError, match=r"covariates=S of shape \(20, 2\) is required"):
        m.add_data(Y)
    with pytest.raises(ValueError, match=r"\(20, 2\) is required"):
        m.add_data(Y, covariates=np.zeros((T, 3)))
    with pytest.raises(ValueError, match=r"\(20, 2\) is required"):
        m.add_data(Y, covariates=np.zeros((T - 1, 2)))
    with pytest.raises(ValueError, match="finite"):
        m.add_data(Y, covariates=np.full((T, 2), np.nan))
    for call in (lambda: m.simulate(10), lambda: m.generate(T=10), lambda: m.predictive_check()):
        with pytest.raises(ValueError, match="free-running simulation of a model with covariates"):
            call()
    m0 = models.SparseBernoulliGLM(N, B=B, seed=1)
    with pytest.raises(ValueError, match="n_covariates=0"):
        m0.add_data(Y, covariates=np.zeros((T, 2)))
    with pytest.raises(ValueError, match="goes with datas"):
        m0.log_likelihood(covariates=[np.zeros((T, 2))])


def test_fifth_header_is_bound():
    """the entries of include/pyglm_hip_covariates.h, in tables of their own beside those of pyglm_hip.h (which tests/test_abi.py pins)"""
    from pyglm_amd import _lib
    assert sorted(_lib.COVARIATES_FUNCTIONS) == ["pgl_covariate_add_offset", "pgl_covariate_draw", "pgl_covariate_fold", "pgl_covariate_max",
                                                 "pgl_covariate_offset", "pgl_covariate_reduce_kappa", "pgl_covariate_work_bytes", "pgl_sweep_offset"]
    assert _lib.COVARIATES_CONSTANTS == {"PGL_COVARIATE_MAX": cov.COVARIATE_MAX, "PGL_COVARIATE_ROWS": 256}
    for other in (_lib.FUNCTIONS, _lib.DISPERSION_FUNCTIONS, _lib.DIAGNOSTICS_FUNCTIONS, _lib.SBM_FUNCTIONS):
        assert not set(_lib.COVARIATES_FUNCTIONS) & set(other)
    restype, params = _lib.COVARIATES_FUNCTIONS["pgl_sweep_offset"]
    assert restype is ctypes.c_int and params[0] == ("s", ctypes.POINTER(_lib.Sweep)) and params[1] == ("offsets", ctypes.c_void_p)
    assert [p for p, _ in _lib.COVARIATES_FUNCTIONS["pgl_covariate_draw"][1]] == ["Lambda", "r", "Lambda0", "h0", "z", "Beta_out", "status", "nloc", "K",
                                                                                 "hip_stream"]
    assert _lib.COVARIATES_FUNCTIONS["pgl_covariate_work_bytes"] == (ctypes.c_size_t, [("nloc", ctypes.c_int), ("T", ctypes.c_int), ("K", ctypes.c_int)])
