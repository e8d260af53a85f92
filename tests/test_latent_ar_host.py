"""The latents' temporal prior on the host (pyglm_amd/latents.py: the law pgl_latent_dynamics.hip is held to): the AR(1) prior's precision,
the joint draw's mean and covariance against the dense precision, phi = 0 as the independent bins, the seventh header, the model's side.
Runs without a GPU; tests/test_gpu_latent_ar.py holds the kernels to these functions.  Bounds in units of U = 2^-53 with kappa =
kappa_2(J) from eigvalsh, as there."""
import ctypes

import numpy as np
import pytest

from pyglm_amd import latents as lat
from pyglm_amd import models

LD = np.longdouble
U = 2.0 ** -53
# (T, Q, seg, phi): the shapes of the GPU tests that a unit-z sweep affords here
CASES = [(1, 1, 2, .9), (2, 2, 2, (0, .9)), (3, 1, 2, .9), (37, 2, 2, (0, .9)), (37, 3, 3, .99), (64, 1, 4, .999), (65, 2, 4, .5), (40, 8, 5, .9),
         (96, 2, 32, .9)]


def _inputs(T, Q):
    rng = np.random.default_rng(1000 * T + Q)
    C, om = rng.standard_normal((6, Q)), rng.gamma(1.0, 0.25, size=(T, 6))
    return np.einsum("tn,nj,nk->tjk", om, C, C), rng.standard_normal((T, Q))


def _refined_solve(J, h):
    Jl, hl = J.astype(LD), h.astype(LD)
    x = np.linalg.solve(J, h).astype(LD)
    for _ in range(4):
        x = x + np.linalg.solve(J, (hl - Jl.dot(x)).astype(np.float64))
    return x


@pytest.mark.parametrize("T", [1, 2, 7])
def test_prior_precision_inverts_to_the_stationary_covariance(T):
    """Lambda = 0: J^-1 is the covariance of Q independent stationary AR(1) processes, phi_q^|t - s|, marginal variance 1"""
    phi = np.array([0.0, 0.5, 0.97])
    Q = phi.size
    J = lat.ar_precision_dense(np.zeros((T, Q, Q)), phi)
    assert J.shape == (T * Q, T * Q) and np.array_equal(J, J.T)
    t = np.arange(T)
    want = np.zeros((T * Q, T * Q))
    for q in range(Q):
        want[q::Q, q::Q] = phi[q] ** np.abs(t[:, None] - t[None, :])
    np.testing.assert_allclose(np.linalg.inv(J), want, rtol=0, atol=1e-12)
    d, e = lat.ar_prior_blocks(T, phi)
    assert d.shape == (T, Q) and e.shape == (Q,)
    np.testing.assert_array_equal(d[:, 0], np.ones(T))             # phi = 0: the identity of the independent bins
    if T == 1:
        np.testing.assert_array_equal(d, np.ones((1, Q)))
    else:
        s = 1 - phi ** 2
        np.testing.assert_allclose(d[0], 1 / s), np.testing.assert_allclose(d[T // 2] if T > 2 else (1 + phi ** 2) / s, (1 + phi ** 2) / s)
        np.testing.assert_allclose(e, -phi / s)


def test_check_ar():
    np.testing.assert_array_equal(lat.check_ar(None, 3), np.zeros(3))
    np.testing.assert_array_equal(lat.check_ar(None, 0), np.zeros(0))
    np.testing.assert_array_equal(lat.check_ar(0.5, 2), [0.5, 0.5])
    np.testing.assert_array_equal(lat.check_ar([0.0, 0.9], 2), [0.0, 0.9])
    assert lat.check_ar(0, 1).dtype == np.float64
    for bad, Q in ((1.0, 1), (-0.1, 1), (float("nan"), 1), ([0.5], 2), ([0.5, 0.5, 0.5], 2), ([[0.5, 0.5]], 2), ("slow", 1), ([0.5, 1.5], 2)):
        with pytest.raises(ValueError, match="0 <= phi < 1"):
            lat.check_ar(bad, Q)
    with pytest.raises(ValueError, match="n_latents=0"):
        lat.check_ar(0.5, 0)
    with pytest.raises(ValueError, match="n_latents=0"):
        models.SparseBernoulliGLM(3, B=1, latent_ar=0.0)
    with pytest.raises(ValueError, match="0 <= phi < 1"):
        models.SparseBernoulliGLM(3, B=1, n_latents=2, latent_ar=[0.5, 1.0])
    with pytest.raises(ValueError, match="0 <= phi < 1"):
        models.BernoulliGLM(3, B=1, n_latents=2, latent_ar=[0.5])
    m = models.NegativeBinomialGLM(3, B=1, n_latents=2, latent_ar=0.25)
    np.testing.assert_array_equal(m.latent_ar, [0.25, 0.25])
    np.testing.assert_array_equal(models.SparseBernoulliGLM(3, B=1, n_latents=2).latent_ar, [0.0, 0.0])
    np.testing.assert_array_equal(models.SparseBernoulliGLM(3, B=1).latent_ar, np.zeros(0))


@pytest.mark.parametrize("T, Q, seg, phi", CASES)
def test_draw_is_the_joint_gaussian(T, Q, seg, phi):
    """serially and by segments and separators: at z = 0 the draw is J^-1 h within 8 Q U kappa ||ref||, and the map M of the unit z's
    satisfies max |M M' J - I| <= 8 Q U kappa.  The two orders are different maps of the same law"""
    Lam, r = _inputs(T, Q)
    J = lat.ar_precision_dense(Lam, phi)
    w = np.linalg.eigvalsh(J)
    kappa = float(w[-1] / w[0])
    ref = _refined_solve(J, r.reshape(-1))
    Ms = []
    for sg in (None, seg):
        m = lat.latent_ar_draw_host(Lam, r, np.zeros((T, Q)), phi, seg=sg)
        assert float(np.linalg.norm(m.reshape(-1) - ref)) <= 8 * Q * U * kappa * float(np.linalg.norm(ref))
        M = np.stack([(lat.latent_ar_draw_host(Lam, r, np.eye(T * Q)[i].reshape(T, Q), phi, seg=sg) - m).reshape(-1) for i in range(T * Q)], axis=1)
        assert float(np.abs(M.dot(M.T).dot(J) - np.eye(T * Q)).max()) <= 8 * Q * U * kappa
        Ms.append(M)
    if T >= 2 * seg:
        assert np.abs(Ms[0] - Ms[1]).max() > 1e-3
    else:
        np.testing.assert_array_equal(Ms[0], Ms[1])


def test_phi_zero_is_the_independent_draw():
    rng = np.random.default_rng(3)
    T, Q = 23, 3
    Lam, r = _inputs(T, Q)
    z = rng.standard_normal((T, Q))
    want = lat.latent_draw_host(Lam, r, z)
    for seg in (None, 2, 5):
        np.testing.assert_allclose(lat.latent_ar_draw_host(Lam, r, z, 0.0, seg=seg), want, rtol=0, atol=1e-13)
    np.testing.assert_allclose(lat.latent_ar_draw_host(Lam, r, z, None), want, rtol=0, atol=1e-13)
    with pytest.raises(np.linalg.LinAlgError):
        bad = Lam.copy()
        bad[4] = -50.0 * np.eye(Q)
        lat.latent_ar_draw_host(bad, r, z, 0.9)
    assert lat.latent_ar_draw_host(Lam[:0], r[:0], z[:0], 0.9).shape == (0, Q)


def test_header_is_a_seventh_table():
    from pyglm_amd import _lib
    assert sorted(_lib.LATENT_DYNAMICS_FUNCTIONS) == ["pgl_latent_ar_draw", "pgl_latent_ar_scratch", "pgl_latent_ar_seg"]
    assert _lib.LATENT_DYNAMICS_CONSTANTS == {}
    for other in (_lib.FUNCTIONS, _lib.DISPERSION_FUNCTIONS, _lib.DIAGNOSTICS_FUNCTIONS, _lib.SBM_FUNCTIONS, _lib.COVARIATES_FUNCTIONS,
                  _lib.LATENTS_FUNCTIONS):
        assert not set(_lib.LATENT_DYNAMICS_FUNCTIONS) & set(other)
    assert [p for p, _ in _lib.LATENT_DYNAMICS_FUNCTIONS["pgl_latent_ar_draw"][1]] == [
        "Lambda", "r", "phi", "z_override", "seed", "sweep", "elem0", "S", "lds", "col0", "status", "T", "Q", "seg", "scratch", "scratch_bytes",
        "hip_stream"]
    assert _lib.LATENT_DYNAMICS_FUNCTIONS["pgl_latent_ar_seg"] == (ctypes.c_int, [])
    assert _lib.LATENT_DYNAMICS_FUNCTIONS["pgl_latent_ar_scratch"] == (ctypes.c_size_t, [("T", ctypes.c_int), ("Q", ctypes.c_int), ("seg", ctypes.c_int)])
    assert _lib._params("pgl_latent_ar_draw")[2] == "phi" and _lib._params("pgl_latent_draw")[2] == "z_override" and _lib.ABI_VERSION == 11
    assert _lib.HEADER_LATENT_DYNAMICS.endswith("pyglm_hip_latent_dynamics.h")


def _cpu_data(N=3, T=120):
    rng = np.random.default_rng(4)
    g = np.cumsum(rng.standard_normal(T)) * 0.2
    return (rng.random((T, N)) < 1 / (1 + np.exp(1.0 - g[:, None] * np.array([1.5, -1.5, 1.0])[:N]))).astype(float)


def test_model_hands_latent_ar_to_the_factory_only_when_it_is_not_zero():
    from tests._latent_ar_engine import LatentAROracleEngine
    from tests._latent_engine import LatentOracleEngine
    seen = []

    def factory(N, B, n0, n1, **kw):
        seen.append(dict(kw))
        return LatentAROracleEngine(N, B, n0, n1, **kw)

    Y = _cpu_data()
    for ar in (None, 0.0, [0.0, 0.0]):
        m = models.SparseBernoulliGLM(3, B=1, seed=9, n_latents=2, latent_ar=ar, engine_factory=factory)
        m.add_data(Y)
        assert "latent_ar" not in seen[-1] and seen[-1]["n_latents"] == 2
        # ... so a factory from before the temporal prior keeps working
        models.SparseBernoulliGLM(3, B=1, seed=9, n_latents=2, latent_ar=ar, engine_factory=LatentOracleEngine).add_data(Y)
    m = models.SparseBernoulliGLM(3, B=1, seed=9, n_latents=2, latent_ar=[0.0, 0.9], engine_factory=factory)
    m.add_data(Y)
    np.testing.assert_array_equal(seen[-1]["latent_ar"], [0.0, 0.9])
    np.testing.assert_array_equal(m.engine.latent_ar, [0.0, 0.9])
    old = models.SparseBernoulliGLM(3, B=1, seed=9, n_latents=2, latent_ar=0.9, engine_factory=LatentOracleEngine)
    with pytest.raises(ValueError, match="does not accept the keyword latent_ar"):
        old.add_data(Y)


def test_cpu_chain_replays_through_the_host_law():
    """three sweeps on tests/_latent_ar_engine.py: in every sweep the latents are latent_ar_step_host of what the sweep left, on the stream's
    normals; the state round-trips and does not carry phi"""
    from tests._latent_ar_engine import LatentAROracleEngine
    N, Q, phi = 3, 2, (0.9, 0.5)
    Y = _cpu_data(N)
    T = Y.shape[0]
    m = models.SparseBernoulliGLM(N, B=1, seed=9, n_latents=Q, latent_ar=phi, engine_factory=LatentAROracleEngine)
    m.add_data(Y)
    eng = m.engine
    for sweep in range(3):
        beta_old, x_old = m._beta.copy(), m.latents[0]
        m.resample_model()
        Om, Kp, _ = eng.last
        a, W, b = m._local_state()
        z = lat.latent_normals_host(m.seed, sweep, 0, T, Q)
        want = lat.latent_ar_step_host(beta_old, x_old, Om[0], Kp[0], eng.psi_net(a, W, b, 0), z, phi)
        np.testing.assert_array_equal(m.latents[0], want)
        if sweep == 0:                                               # C = 0: the first draw is the prior's, an AR(1) path per factor
            d, e = lat.ar_prior_blocks(T, np.array(phi))
            np.testing.assert_allclose(want, lat.latent_ar_draw_host(np.zeros((T, Q, Q)), np.zeros((T, Q)), z, phi), rtol=0, atol=0)
    st = m.get_state()
    assert "latent_ar" not in st and "latents" in st
    x = m.latents[0]
    m.resample_model()
    after = (m.latents[0], m._beta.copy())
    m.set_state(st)
    np.testing.assert_array_equal(m.latents[0], x)
    m.resample_model()
    np.testing.assert_array_equal(m.latents[0], after[0]), np.testing.assert_array_equal(m._beta, after[1])


def test_slow_drive_is_followed_better_with_the_temporal_prior():
    """the CPU chain of tests/test_gpu_latent_ar.py's recovery comparison, where its seed was settled: under an AR(1) drive with phi_true =
    .98 the posterior-mean common input correlates with the true drive more under latent_ar = .95 than under independent bins"""
    from tests import _latent_ar_engine as la
    from tests import _latent_engine as le
    Y, drive, load = la.ar_recovery_problem()
    corr = {}
    for ar, factory in ((None, le.LatentOracleEngine), (la.AR_RECOVERY["phi"], la.LatentAROracleEngine)):
        _, common = le.recovery_run(la.ar_recovery_model(ar, engine_factory=factory), Y)
        corr[ar] = la.ar_recovery_corr(common, drive, load)
    print(corr)
    assert corr[la.AR_RECOVERY["phi"]] > corr[None]
