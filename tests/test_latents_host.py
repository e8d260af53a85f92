"""Latent common input on the host (pyglm_amd/latents.py, the law the kernels of pgl_latents.hip are held to): the conditional of x_t is the
right Gaussian, the normals are the stated Philox stream, the model's chain replays through the host law, the latents take the confound
off the network, and what cannot work is refused.  Runs without a GPU; tests/test_gpu_latents.py holds the kernels to these functions."""
import ctypes
import math

import numpy as np
import pytest

from pyglm_amd import covariates as cov
from pyglm_amd import latents as lat
from pyglm_amd import models

LD = np.longdouble


def _case(seed=3, N=3, Q=2, T=5, K_obs=1):
    """fixed omega: S_obs, beta = [b_obs | C], omega, kappa = y - 1/2, psi_net, the latents x_old the 'sweep' ran under"""
    rng = np.random.default_rng(seed)
    S_obs = rng.standard_normal((T, K_obs))
    beta = rng.standard_normal((N, K_obs + Q))
    om = rng.uniform(0.05, 0.25, size=(T, N))
    kappa = (rng.random((T, N)) < 0.4).astype(float) - 0.5
    psi_net = rng.standard_normal((T, N))
    x_old = rng.standard_normal((T, Q))
    return S_obs, beta, om, kappa, psi_net, x_old


def test_stats_are_gradient_and_hessian_of_the_augmented_density():
    """N = 3, Q = 2, T = 5, K_obs = 1.  r_t and Lambda_t + I are the gradient and the negative Hessian at x_t = 0 of the augmented
    log-density sum_n kappa psi - omega psi^2 / 2 - |x_t|^2 / 2, psi = psi_net + S_obs b_obs + x_t . C_n, by central differences in long
    double (the function is quadratic: the differences are exact up to rounding at any step; step 1).  The statistics are formed from the
    REDUCED Kappa and the old latents alone: they do not see the offset."""
    S_obs, beta, om, kappa, psi_net, x_old = _case()
    K_obs, Q, T = S_obs.shape[1], x_old.shape[1], x_old.shape[0]
    C = beta[:, K_obs:]
    o_sweep = cov.offset_host(np.column_stack([S_obs, x_old]), beta)
    Lam, r = lat.latent_stats_host(C, x_old, om, kappa - om * o_sweep, psi_net)
    o_obs = np.asarray(S_obs, dtype=LD).dot(np.asarray(beta[:, :K_obs], dtype=LD).T)
    oml, kl, pl, Cl = (np.asarray(v, dtype=LD) for v in (om, kappa, psi_net, C))
    e = np.eye(Q, dtype=LD)
    for t in range(T):
        def f(x):
            psi = pl[t] + o_obs[t] + Cl.dot(x)
            return np.sum(kl[t] * psi - oml[t] * psi * psi / 2) - x.dot(x) / 2
        grad = np.array([(f(e[i]) - f(-e[i])) / 2 for i in range(Q)], dtype=LD)
        hess = np.array([[(f(e[i] + e[j]) - f(e[i] - e[j]) - f(-e[i] + e[j]) + f(-e[i] - e[j])) / 4 for j in range(Q)] for i in range(Q)], dtype=LD)
        np.testing.assert_allclose(r[t], grad.astype(np.float64), rtol=1e-12, atol=1e-12 * np.abs(r[t]).max())
        np.testing.assert_allclose(Lam[t] + np.eye(Q), -hess.astype(np.float64), rtol=1e-12, atol=1e-12)
    Ll, rl = lat.latent_stats_host(C, x_old, om, kappa - om * o_sweep, psi_net, dtype=LD)
    assert Ll.dtype == LD and np.allclose(Ll.astype(np.float64), Lam, rtol=1e-13) and np.allclose(rl.astype(np.float64), r, rtol=1e-11, atol=1e-13)


def test_draw_over_fixed_normals():
    """z = 0 and the unit vectors: the draw's mean is A^-1 r and its covariance M M' (M: the map from z to x) is A^-1, by hand"""
    S_obs, beta, om, kappa, psi_net, x_old = _case(seed=8, N=4, Q=3, T=6, K_obs=0)
    Q = 3
    Lam, r = lat.latent_stats_host(beta, x_old, om, kappa, psi_net)
    mean = lat.latent_draw_host(Lam, r, np.zeros_like(r))
    for t in range(r.shape[0]):
        A = Lam[t] + np.eye(Q)
        M = np.stack([lat.latent_draw_host(Lam[t:t + 1], r[t:t + 1], np.eye(Q)[i:i + 1])[0] - mean[t] for i in range(Q)], axis=1)
        np.testing.assert_allclose(mean[t], np.linalg.inv(A).dot(r[t]), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(M.dot(M.T), np.linalg.inv(A), rtol=1e-12, atol=1e-13)
    np.testing.assert_array_equal(lat.latent_step_host(beta, x_old, om, kappa, psi_net, np.ones_like(r)), lat.latent_draw_host(Lam, r, np.ones_like(r)))
    with pytest.raises(np.linalg.LinAlgError):
        lat.latent_draw_host(-2.0 * np.eye(Q)[None], r[:1], np.zeros((1, Q)))


def _philox_scalar(c, key):
    """Philox4x32-10 on Python integers: counter (c0, c1, c2, c3), key (k0, k1) -> four 32-bit words"""
    c0, c1, c2, c3 = c
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def test_normals_are_the_stated_stream():
    """latent_normals_host against a scalar restatement: key = seed, counter = (q | 6 << 24, elem0 + t, sweep lo, sweep hi), u = ((64 bits >>
    11) + 1/2) 2^-53 from words (0, 1) and (2, 3), Box-Muller with the cosine; distinct (sweep, element, q) give distinct draws"""
    seed, sweep, elem0, T, Q = (5 << 40) + 77, (3 << 32) + 9, 1000, 7, 3
    z = lat.latent_normals_host(seed, sweep, elem0, T, Q)
    assert lat.PURPOSE_LATENT == 6 and z.shape == (T, Q)
    for t in range(T):
        for q in range(Q):
            w = _philox_scalar((q | (6 << 24), elem0 + t, sweep & 0xFFFFFFFF, sweep >> 32), (seed & 0xFFFFFFFF, seed >> 32))
            u0 = (((w[0] | (w[1] << 32)) >> 11) + 0.5) / 2.0 ** 53
            u1 = (((w[2] | (w[3] << 32)) >> 11) + 0.5) / 2.0 ** 53
            assert abs(z[t, q] - math.sqrt(-2.0 * math.log(u0)) * math.cos(2.0 * math.pi * u1)) <= 1e-14
    np.testing.assert_array_equal(lat.latent_normals_host(seed, sweep, elem0 + 2, T - 2, Q), z[2:])           # keyed by the element, not the call
    others = [lat.latent_normals_host(seed, sweep + 1, elem0, T, Q), lat.latent_normals_host(seed, sweep, elem0 + T, T, Q),
              lat.latent_normals_host(seed + 1, sweep, elem0, T, Q)]
    flat = np.concatenate([z.ravel()] + [o.ravel() for o in others])
    assert np.unique(flat).size == flat.size
    big = lat.latent_normals_host(1, 2, 0, 20000, 2)
    assert abs(big.mean()) < 0.02 and abs(big.std() - 1.0) < 0.02 and abs(np.corrcoef(big[:, 0], big[:, 1])[0, 1]) < 0.03


def test_counts_and_priors():
    assert lat.check_count(0) == 0 and lat.check_count(8, 24) == 8 and lat.LATENT_MAX == 8
    for bad in ((9, 0), (-1, 0), (1.5, 0), (1, 32), (8, 25)):
        with pytest.raises(ValueError):
            lat.check_count(*bad)
    mu, Sigma = lat.joint_prior(2, 3, (np.array([1.0, 2.0]), 4.0), (0.5, np.diag([1.0, 2.0, 3.0])))
    np.testing.assert_array_equal(mu, [1.0, 2.0, 0.5, 0.5, 0.5])
    np.testing.assert_array_equal(Sigma, np.diag([4.0, 4.0, 1.0, 2.0, 3.0]))
    mu, Sigma = lat.joint_prior(0, 2)
    np.testing.assert_array_equal(mu, np.zeros(2)), np.testing.assert_array_equal(Sigma, np.eye(2))
    with pytest.raises(ValueError, match="latent_loading_prior"):
        lat.joint_prior(1, 2, None, (0.0, np.eye(3)))
    with pytest.raises(ValueError):
        lat.check_latents(np.zeros((4, 2)), 5, 2)
    with pytest.raises(ValueError):
        lat.check_latents(np.full((5, 2), np.nan), 5, 2)


def _cpu_model(N=3, K_obs=1, Q=2, **kw):
    from tests._latent_engine import LatentOracleEngine
    return models.SparseBernoulliGLM(N, B=1, seed=9, n_covariates=K_obs, n_latents=Q, engine_factory=LatentOracleEngine, **kw)


def _cpu_data(N=3, T=300, K_obs=1):
    rng = np.random.default_rng(4)
    S = np.sin(np.arange(T) / 7.0)[:, None] * np.ones((1, K_obs))
    g = rng.standard_normal(T)
    Y = (rng.random((T, N)) < 1 / (1 + np.exp(1.0 - 0.8 * S[:, :1] - g[:, None] * np.array([1.5, -1.5, 1.0])[:N]))).astype(float)
    return Y, S


def test_model_chain_replays_through_the_host_law():
    """the model's chain on the oracle engine (tests/_latent_engine.py): in every sweep the latents are latent_step_host of what the sweep
    left -- before beta moves, from the loadings and latents the sweep ran under -- and beta is covariate_step_host given the NEW latents and
    the offset the sweep ran under; two read-outs (log-likelihood, means) see psi_net + offset_host([S_obs | X], beta); the state, latents
    included, round-trips"""
    N, K_obs, Q = 3, 1, 2
    Y, S = _cpu_data(N)
    m = _cpu_model(N, K_obs, Q)
    m.add_data(Y, covariates=S)
    eng = m.engine
    assert m.K == 3 and m.covariate_weights.shape == (N, K_obs) and m.latent_loadings.shape == (N, Q)
    assert m.latents[0].shape == (Y.shape[0], Q) and not m.latents[0].any() and not m.common_input().any()
    for sweep in range(3):
        beta_old, x_old = m._beta.copy(), m.latents[0]
        m.resample_model()
        Om, Kp, off = eng.last
        a, W, b = m._local_state()
        psi_net = eng.psi_net(a, W, b, 0)
        np.testing.assert_array_equal(off[0], cov.offset_host(np.column_stack([S, x_old]), beta_old))        # the offset the sweep ran under
        x_new = lat.latent_step_host(beta_old[:, K_obs:], x_old, Om[0], Kp[0], psi_net, lat.latent_normals_host(m.seed, sweep, 0, Y.shape[0], Q))
        np.testing.assert_array_equal(m.latents[0], x_new)
        S_new = np.column_stack([S, x_new])
        want = cov.covariate_step_host([(S_new, Om[0], Kp[0], off[0], psi_net)], eng.cov_prior[2], eng.cov_prior[3],
                                       cov.covariate_draws(m.seed, sweep, range(N), K_obs + Q))
        np.testing.assert_array_equal(m._beta, want)
        np.testing.assert_array_equal(m.covariate_weights, want[:, :K_obs]), np.testing.assert_array_equal(m.latent_loadings, want[:, K_obs:])
        if sweep == 0:
            np.testing.assert_array_equal(x_new, lat.latent_normals_host(m.seed, 0, 0, Y.shape[0], Q))      # C = 0: the first draw is the prior's
    np.testing.assert_array_equal(m.common_input(), cov.offset_host(x_new, want[:, K_obs:]))
    psi = psi_net + cov.offset_host(S_new, want)
    np.testing.assert_allclose(m.log_likelihood(), np.sum(Y * psi - np.log1p(np.exp(psi))), rtol=1e-12)
    np.testing.assert_allclose(m.means[0], 1.0 / (1.0 + np.exp(-psi)), rtol=1e-12)
    st = m.get_state()
    np.testing.assert_array_equal(st["latents"][0], x_new)
    m.resample_model()
    after = (m.latents[0], m._beta.copy(), m.weights, m.biases)
    m.set_latents(0, np.zeros_like(x_new))
    assert not m.latents[0].any()
    m.set_state(st)
    np.testing.assert_array_equal(m.latents[0], x_new)
    m.resample_model()
    for x, y in zip(after, (m.latents[0], m._beta, m.weights, m.biases)):
        np.testing.assert_array_equal(x, y)
    acc = m.summarize(rates=False)
    acc.collect()
    np.testing.assert_array_equal(acc.common_input_var_mean, np.sum(m.latent_loadings ** 2, axis=1))
    np.testing.assert_array_equal(acc.covariate_mean, m.covariate_weights)
    m.resample_model(), acc.collect()
    assert acc.common_input_var_var.shape == (N,) and np.all(acc.common_input_var_var >= 0)


def test_latents_take_the_common_input_off_the_network():
    """two uncoupled populations under one unrecorded drive (tests/_latent_engine.py: recovery_problem), fixed seed: the between-population
    edge probability with one latent is below that without, and every neuron's mean common input follows its true drive better than any
    single spike train follows the drive"""
    from tests import _latent_engine as le
    from tests._oracle_engine import OracleEngine
    Y, drive, load = le.recovery_problem()
    P0, _ = le.recovery_run(le.recovery_model(0, engine_factory=OracleEngine), Y)
    P1, common = le.recovery_run(le.recovery_model(1, engine_factory=le.LatentOracleEngine), Y)
    ok, fig = le.recovery_verdict(P0, P1, common, Y, drive, load)
    print(fig)
    assert ok, fig


def test_refusals():
    from tests._latent_engine import LatentOracleEngine
    from tests._oracle_engine import OracleEngine
    with pytest.raises(ValueError, match="n_latents"):
        models.SparseBernoulliGLM(3, B=1, n_latents=9)
    with pytest.raises(ValueError, match="at most"):
        models.SparseBernoulliGLM(3, B=1, n_covariates=30, n_latents=3)
    with pytest.raises(ValueError, match="latent_loading_prior"):
        models.SparseBernoulliGLM(3, B=1, latent_loading_prior=(0.0, 1.0))
    with pytest.raises(ValueError, match="shard"):
        models.SparseBernoulliGLM(4, B=1, n_latents=1, shard=(0, 2))
    Y, S = _cpu_data()
    m = _cpu_model()
    m.add_data(Y, covariates=S)
    for call in (lambda: m.log_likelihood(datas=[Y], covariates=[S]), lambda: m.summarize(datas=[Y], covariates=[S]),
                 lambda: m.time_rescaling(datas=[Y], covariates=[S])):
        with pytest.raises(ValueError, match="held-out"):
            call()
    for call in (lambda: m.generate(T=10), lambda: m.simulate(10), lambda: m.predictive_check()):
        with pytest.raises(ValueError, match="n_latents=2"):
            call()
    plain = models.SparseBernoulliGLM(3, B=1, seed=1, n_latents=1, engine_factory=OracleEngine)
    with pytest.raises(ValueError, match="latent_step"):
        plain.add_data(Y)
    none = models.SparseBernoulliGLM(3, B=1, seed=1, engine_factory=LatentOracleEngine, n_covariates=1)
    for call in (lambda: none.latents, lambda: none.latent_loadings, lambda: none.common_input(), lambda: none.set_latents(0, np.zeros((1, 1)))):
        with pytest.raises(ValueError, match="n_latents=0"):
            call()
    with pytest.raises(ValueError):
        m.set_latents(0, np.zeros((Y.shape[0], 5)))


def test_without_latents_state_and_rows_are_as_before():
    """n_latents=0: the state's keys and bytes and the packed rows are those of a model built without the argument"""
    import pickle
    N, B = 5, 2
    rng = np.random.default_rng(0)
    a, W, b = rng.random((3, N)) < 0.5, rng.standard_normal((3, N, B)), rng.standard_normal(3)
    eta, stats, beta = rng.random(3), rng.standard_normal((3, 1 + B + B * B)), rng.standard_normal((3, 2))
    for kw in (dict(), dict(n_covariates=2)):
        np.random.seed(3)
        m0 = models.SparseBernoulliGLM(N, B=B, seed=1, **kw)
        np.random.seed(3)
        m1 = models.SparseBernoulliGLM(N, B=B, seed=1, n_latents=0, **kw)
        assert m1.Q == 0 and m1.K == m0.K == m1.K_obs
        args = (a, W, b, eta, stats) + ((beta,) if kw else ())
        assert m0._pack_rows_host(*args).tobytes() == m1._pack_rows_host(*args).tobytes()
        s0, s1 = m0.get_state(), m1.get_state()
        assert list(s0) == list(s1) and "latents" not in s1
        for k in s0:
            if k != "regressions" and k != "network":
                assert pickle.dumps(s0[k]) == pickle.dumps(s1[k])
        for r0, r1 in zip(s0["regressions"], s1["regressions"]):
            assert r0.a.tobytes() == r1.a.tobytes() and r0.W.tobytes() == r1.W.tobytes() and r0.b.tobytes() == r1.b.tobytes()
    assert models.state_row_layout(N, B, 2) == (80, 88, 96, 152, 152 + 8 + 16)


def test_header_is_a_sixth_table():
    from pyglm_amd import _lib
    assert sorted(_lib.LATENTS_FUNCTIONS) == ["pgl_latent_draw", "pgl_latent_fold", "pgl_latent_max"]
    assert _lib.LATENTS_CONSTANTS == {"PGL_LATENT_MAX": lat.LATENT_MAX, "PGL_LATENT_LDS_COLS": 1024, "PGL_PURPOSE_LATENT": lat.PURPOSE_LATENT}
    for other in (_lib.FUNCTIONS, _lib.DISPERSION_FUNCTIONS, _lib.DIAGNOSTICS_FUNCTIONS, _lib.SBM_FUNCTIONS, _lib.COVARIATES_FUNCTIONS):
        assert not set(_lib.LATENTS_FUNCTIONS) & set(other)
    assert [p for p, _ in _lib.LATENTS_FUNCTIONS["pgl_latent_fold"][1]] == ["Psi", "ldn", "bias", "Omega", "ldo", "Kappa", "ldk", "S", "lds", "col0", "Beta",
                                                                           "ldb", "T", "nloc", "Q", "Lambda", "r", "hip_stream"]
    assert [p for p, _ in _lib.LATENTS_FUNCTIONS["pgl_latent_draw"][1]] == ["Lambda", "r", "z_override", "seed", "sweep", "elem0", "S", "lds", "col0",
                                                                           "status", "T", "Q", "hip_stream"]
    assert _lib.LATENTS_FUNCTIONS["pgl_latent_max"] == (ctypes.c_int, [])
    assert _lib._params("pgl_latent_draw")[2] == "z_override" and _lib.ABI_VERSION == 11
