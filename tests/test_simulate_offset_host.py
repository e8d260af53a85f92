"""Free-running simulation of a model with covariates or latent factors, on the host (pyglm_amd/simulate.py: simulate_host(offset=),
simulate_offset_host, latent_prior_host; models.py: simulate(covariates=, latents=), predictive_check(covariates=, latents=)): the law, the
prior paths' stream, recurrence, continuation and moments, the model's side on the oracle engines, the refusals, the eighth header.  Runs
without a GPU; tests/test_gpu_simulate_offset.py holds the kernels to these functions."""
import ctypes
import math

import numpy as np
import pytest

from pyglm_amd import covariates as cov
from pyglm_amd import models, simulate
from pyglm_amd.utils.basis import cosine_basis


def _small_model(N, B, L, seed):
    rng = np.random.default_rng(seed)
    Wm = rng.standard_normal((N, N * B)) * 0.3 * (rng.random((N, N * B)) < 0.5)
    bias = -1.5 + 0.3 * rng.standard_normal(N)
    return Wm, bias, cosine_basis(B, L=L) / L


def test_a_zero_offset_is_no_offset():
    N, B, L, R, T = 5, 2, 30, 3, 200
    Wm, bias, basis = _small_model(N, B, L, 1)
    kind = np.array([0, 2, 3, 0, 1], dtype=np.int32)                 # Bernoulli, negative binomial, binomial, Bernoulli, Gaussian
    par = np.array([0.0, 2.5, 10.0, 0.0, 0.3])
    Wm[:, 2 * B:3 * B] /= 10.0
    hist = np.zeros((R, L, N))
    a = simulate.simulate_host(Wm, bias, basis, kind, par, T, R, 7, 2, hist, 0, True, offset=None)
    for shape in ((R, T, N), (1, T, N)):
        b = simulate.simulate_host(Wm, bias, basis, kind, par, T, R, 7, 2, hist, 0, True, offset=np.zeros(shape))
        for name in ("Y", "sum", "sumsq", "history"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.latents is None and a.latent_last is None and len(tuple(a)) == 4


def test_rates_follow_the_covariate():
    """W = 0, beta = +-2, S a square wave of period 100: per phase every neuron's rate lies within 5 sqrt(p (1 - p) / n) of sigmoid(b +- beta)"""
    N, T, R = 4, 20000, 2
    basis = cosine_basis(1, L=5) / 5
    bias = np.array([-1.0, -0.5, 0.0, -2.0])
    beta = np.array([[2.0], [-2.0], [2.0], [-2.0]])
    S = np.where((np.arange(T) // 50) % 2 == 0, 1.0, -1.0)[:, None]
    off = simulate.simulate_offset_host(S, None, beta)
    assert off.shape == (1, T, N) and np.array_equal(off[0], cov.offset_host(S, beta))
    sim = simulate.simulate_host(np.zeros((N, N)), bias, basis, np.zeros(N, dtype=np.int32), np.zeros(N), T, R, 11, 0, np.zeros((R, 5, N)), 0, True,
                                 offset=off)
    for sign in (1.0, -1.0):
        rows = S[:, 0] == sign
        n = rows.sum() * R
        p = 1.0 / (1.0 + np.exp(-(bias + sign * beta[:, 0])))
        rate = sim.Y[:, rows].mean(axis=(0, 1))
        print(sign, rate, p, np.abs(rate - p) / np.sqrt(p * (1 - p) / n))
        assert np.all(np.abs(rate - p) <= 5.0 * np.sqrt(p * (1 - p) / n))


def _philox_scalar(c, k):
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def _normal_scalar(seed, rep, t, q):
    w = _philox_scalar([q | (7 << 24), t & 0xFFFFFFFF, rep & 0xFFFFFFFF, rep >> 32], [seed & 0xFFFFFFFF, seed >> 32])
    u0 = (((w[0] | (w[1] << 32)) >> 11) + 0.5) / 2.0 ** 53
    u1 = (((w[2] | (w[3] << 32)) >> 11) + 0.5) / 2.0 ** 53
    return math.sqrt(-2.0 * math.log(u0)) * math.cos(2.0 * math.pi * u1)


def test_prior_normals_are_the_scalar_stream():
    seed, t0 = 0x1234567890ABCDEF, 1000
    X = simulate.latent_prior_host(seed, [3, 4, 9], t0, 50, np.zeros(3))
    for r, t, q in ((3, 1000, 0), (9, 1049, 2), (4, 1017, 1)):
        want = _normal_scalar(seed, r, t, q)
        got = X[[3, 4, 9].index(r), t - t0, q]
        assert abs(got - want) <= 4 * 2.0 ** -53 * max(1.0, abs(want)), (r, t, q, got, want)      # (math.log / cos against NumPy's: an ulp or two)
    assert np.unique(X).size == X.size                               # distinct (replicate, t, q): distinct values
    assert simulate.PURPOSE_SIM_LATENT == 7


def test_recurrence_is_the_scalar_loop():
    phi = np.array([0.0, 0.5, 0.9])
    z = simulate.latent_normals_sim_host(5, [0, 1], 0, 300, 3)
    X = simulate.latent_prior_host(5, [0, 1], 0, 300, phi)
    assert np.array_equal(simulate.latent_prior_host(5, [0, 1], 0, 300, np.zeros(3)), z)          # phi = 0: z itself
    assert np.array_equal(X[:, :, 0], z[:, :, 0])
    s = np.sqrt(1.0 - phi * phi)
    for r in range(2):
        for q in range(3):
            x = float(z[r, 0, q])
            assert X[r, 0, q] == x                                   # the stationary start
            for t in range(1, 300):
                a, b = float(phi[q]) * x, float(s[q]) * float(z[r, t, q])
                x = a + b
                assert X[r, t, q] == x, (r, q, t)


def test_a_path_cut_in_two_is_one_path():
    phi = np.array([0.9, 0.0, 0.5])
    whole = simulate.latent_prior_host(9, np.arange(3), 40, 200, phi)
    first = simulate.latent_prior_host(9, np.arange(3), 40, 70, phi)
    second = simulate.latent_prior_host(9, np.arange(3), 110, 130, phi, carry=first[:, -1])
    assert np.array_equal(np.concatenate([first, second], axis=1), whole)
    assert not np.array_equal(simulate.latent_prior_host(9, np.arange(3), 110, 130, phi), second)      # (without the carry: a fresh start)


def test_a_path_does_not_depend_on_the_replicates_beside_it():
    phi = np.array([0.9, 0.5])
    six = simulate.latent_prior_host(3, 0 + np.arange(6), 0, 100, phi)
    one = simulate.latent_prior_host(3, 5 + np.arange(1), 0, 100, phi)
    assert np.array_equal(six[5], one[0])
    assert not np.array_equal(six[4], one[0])


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_prior_paths_have_the_stationary_moments(phi):
    """variance within 5 standard errors sqrt(2 / n_eff) of 1, n_eff = n (1 - phi^2) / (1 + phi^2); lag-1 autocorrelation within 5
    standard errors sqrt((1 - phi^2) / n) of phi"""
    T, R = 20000, 4
    X = simulate.latent_prior_host(2, np.arange(R), 0, T, np.array([phi]))[:, :, 0]
    n = R * T
    var = np.mean(X * X)
    n_eff = n * (1 - phi ** 2) / (1 + phi ** 2)
    rho = np.mean(X[:, 1:] * X[:, :-1]) / var
    print(phi, var, (var - 1) / np.sqrt(2 / n_eff), rho, (rho - phi) / np.sqrt((1 - phi ** 2) / n))
    assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / n_eff)
    assert abs(rho - phi) <= 5.0 * np.sqrt((1.0 - phi ** 2) / n)


# ---------------------------------------------------------------------------------------------------------------- the model's side
def _data(N=4, T=150, K=1):
    rng = np.random.default_rng(0)
    return (rng.random((T, N)) < 0.2).astype(float), rng.standard_normal((T, K))


@pytest.fixture(scope="module")
def cov_model():
    from tests._covariate_engine import CovariateOracleEngine
    Y, S = _data(K=2)
    m = models.SparseBernoulliGLM(4, B=2, seed=3, n_covariates=2, engine_factory=CovariateOracleEngine)
    m.add_data(Y, covariates=S)
    for _ in range(3):
        m.resample_model()
    return m, Y, S


@pytest.fixture(scope="module")
def lat_model():
    from tests._latent_ar_engine import LatentAROracleEngine
    Y, S = _data()
    m = models.SparseBernoulliGLM(4, B=2, seed=3, n_covariates=1, n_latents=2, latent_ar=[0.9, 0.0], engine_factory=LatentAROracleEngine)
    m.add_data(Y, covariates=S)
    for _ in range(3):
        m.resample_model()
    return m, Y, S


def _law(m, T, R, seed, offset, **kw):
    A, W, b = m._adopt_state()
    kind, par = simulate.observation_kinds(m.regressions)
    L = m.basis.shape[0]
    return simulate.simulate_host((W * A[:, :, None]).reshape(m.N, -1), b.ravel(), np.asarray(m.basis, dtype=np.float64), kind, par, T, R, seed,
                                  kw.get("rep0", 0), np.zeros((R, L, m.N)), 0, True, offset=offset)


def test_model_simulate_with_covariates_is_the_law(cov_model):
    m, Y, S = cov_model
    assert np.any(m.covariate_weights != 0)
    sim = m.simulate(100, replicates=3, seed=5, covariates=S[:100])
    ref = _law(m, 100, 3, 5, cov.offset_host(S[:100], m.covariate_weights)[None])
    assert np.array_equal(sim.Y, ref.Y) and np.array_equal(sim.sum, ref.sum) and np.array_equal(sim.history, ref.history)
    assert sim.latents is None and sim.latent_last is None
    assert not np.array_equal(sim.Y, _law(m, 100, 3, 5, None).Y)
    assert np.array_equal(m.simulate(100, replicates=3, seed=5, covariates="data").Y, sim.Y)
    Yk, s, ss, hist = sim
    assert Yk is sim.Y and hist is sim.history


def test_model_simulate_with_latents_is_the_law(lat_model):
    m, Y, S = lat_model
    beta = np.concatenate([m.covariate_weights, m.latent_loadings], axis=1)
    fit = m.simulate(120, replicates=2, seed=6, covariates="data", latents="fitted")
    X = m.latents[0][:120]
    ref = _law(m, 120, 2, 6, cov.offset_host(np.concatenate([S[:120], X], axis=1), beta)[None])
    assert np.array_equal(fit.Y, ref.Y)
    assert fit.latents.shape == (1, 120, 2) and np.array_equal(fit.latents[0], X) and np.array_equal(fit.latent_last, np.tile(X[-1], (2, 1)))
    pri = m.simulate(120, replicates=3, seed=6, covariates=S[:120], latents="prior", first_replicate=4)
    assert pri.latents.shape == (3, 120, 2) and pri.latent_last.shape == (3, 2)
    assert np.array_equal(pri.latents, simulate.latent_prior_host(6, 4 + np.arange(3), 0, 120, m.latent_ar))
    assert np.array_equal(pri.latent_last, pri.latents[:, -1])
    again = m.simulate(120, replicates=3, seed=6, covariates=S[:120], latents=pri.latents, first_replicate=4)
    assert np.array_equal(again.Y, pri.Y)
    off = np.stack([cov.offset_host(np.concatenate([S[:120], pri.latents[r]], axis=1), beta) for r in range(3)])
    assert np.array_equal(pri.Y, _law(m, 120, 3, 6, off, rep0=4).Y)
    assert m.simulate(120, replicates=3, seed=6, covariates=S[:120], latents="prior", keep_paths=False).latents is None
    shared = m.simulate(50, replicates=2, seed=6, covariates=S[:50], latents=pri.latents[0, :50])
    assert shared.latents.shape == (1, 50, 2)


def test_continuation_continues_the_latent_paths(lat_model):
    m, Y, S = lat_model
    whole = m.simulate(130, replicates=3, seed=8, covariates=S[:130], latents="prior")
    first = m.simulate(50, replicates=3, seed=8, covariates=S[:50], latents="prior")
    second = m.simulate(80, replicates=3, seed=8, covariates=S[50:130], latents="prior", history=first)
    assert (second.t0, second.t1) == (50, 130)
    assert np.array_equal(np.concatenate([first.Y, second.Y], axis=1), whole.Y)
    assert np.array_equal(np.concatenate([first.latents, second.latents], axis=1), whole.latents)
    assert np.array_equal(second.latent_last, whole.latent_last) and np.array_equal(second.history, whole.history)


def test_predictive_check_collects_with_covariates_and_latents(lat_model):
    m, Y, S = lat_model
    ppc = m.predictive_check(replicates=2, seed=1, covariates="data", latents="prior", lags=3, isi=8)
    ppc.collect()
    ppc.collect()
    N = m.N
    assert ppc.calls == 2 and ppc.rates.shape == (4, N)
    for stat, shape in (("rate", (N,)), ("fano", (N,)), ("xcorr", (3, N, N)), ("isi", (N, 8)), ("cv", (N,))):
        p = ppc.pvalue(stat)
        assert p.shape == shape, stat
        if stat in ("rate", "fano"):
            assert np.all(np.isfinite(p)) and np.all((p >= 0) & (p <= 1))
    assert np.all(np.isfinite(ppc.pvalue("xcorr")[0]))               # lag 0 is defined wherever a neuron fired
    # the second collect() used fresh replicates of the prior paths too
    assert not np.array_equal(ppc.rates[:2], ppc.rates[2:])
    fitted = m.predictive_check(replicates=2, seed=1, covariates=S, latents="fitted")
    fitted.collect()
    assert fitted.rates.shape == (2, N)


def test_refusals(cov_model, lat_model):
    m, Y, S = cov_model
    ml, _, Sl = lat_model
    T = Y.shape[0]
    for call in (lambda: m.simulate(10), lambda: m.generate(T=10), lambda: m.predictive_check(), lambda: m.generate(T=10)):
        with pytest.raises(ValueError, match="free-running simulation of a model with covariates"):
            call()
    for call in (lambda: ml.simulate(10), lambda: ml.generate(T=10), lambda: ml.predictive_check(), lambda: ml.simulate(10, covariates=Sl[:10]),
                 lambda: ml.predictive_check(covariates="data"), lambda: ml.simulate(10, latents="prior")):
        with pytest.raises(ValueError, match="n_latents=2"):
            call()
    with pytest.raises(ValueError, match="covariates=S"):            # the hint names the keyword
        m.simulate(10)
    from tests._oracle_engine import OracleEngine
    plain = models.SparseBernoulliGLM(4, B=2, seed=1, engine_factory=OracleEngine)
    plain.add_data(Y)
    for call, word in ((lambda: plain.simulate(10, covariates=S[:10]), "n_covariates=0"), (lambda: plain.simulate(10, latents="prior"), "n_latents=0"),
                       (lambda: plain.predictive_check(covariates="data"), "n_covariates=0"), (lambda: m.simulate(10, covariates="data", latents="prior"), "n_latents=0")):
        with pytest.raises(ValueError, match=word):
            call()
    bad = S[:10].copy()
    bad[3, 1] = np.nan
    for call, word in ((lambda: m.simulate(10, covariates=S[:9]), r"\(10, 2\) is required"), (lambda: m.simulate(10, covariates=bad), "finite"),
                       (lambda: m.simulate(10, covariates=S[:10, :1]), r"\(10, 2\) is required"), (lambda: m.simulate(10, covariates="stimulus"), "'data'"),
                       (lambda: m.simulate(T + 1, covariates="data"), "is more"), (lambda: m.predictive_check(covariates=S[:-1]), "is required")):
        with pytest.raises(ValueError, match=word):
            call()
    X = np.zeros((10, 2))
    for call, word in ((lambda: ml.simulate(10, covariates=Sl[:10], latents=X[:9]), r"\(10, 2\) is required"),
                       (lambda: ml.simulate(10, covariates=Sl[:10], latents=np.zeros((10, 3))), "is required"),
                       (lambda: ml.simulate(10, replicates=3, covariates=Sl[:10], latents=np.zeros((2, 10, 2))), "is required"),
                       (lambda: ml.simulate(10, covariates=Sl[:10], latents=np.full((10, 2), np.inf)), "finite"),
                       (lambda: ml.simulate(10, covariates=Sl[:10], latents="posterior"), "'prior', 'fitted'"),
                       (lambda: ml.simulate(T + 1, covariates=np.zeros((T + 1, 1)), latents="fitted"), "is more"),
                       (lambda: ml.predictive_check(covariates="data", latents=np.zeros((T, 2))), "'prior' or 'fitted'")):
        with pytest.raises(ValueError, match=word):
            call()
    first = ml.simulate(10, replicates=2, covariates=Sl[:10], latents="prior")
    with pytest.raises(ValueError, match="carries latents"):
        ml.simulate(10, replicates=3, covariates=Sl[10:20], latents="prior", history=_with_replicates(first, 3))


def _with_replicates(sim, R):
    """the Simulation with its trajectories repeated to R replicates but its latents' carry left as it was"""
    out = simulate.Simulation(None, None, None, np.resize(sim.history, (R,) + sim.history.shape[1:]), sim.t0, sim.t1, sim.seed, 0,
                              latent_last=sim.latent_last)
    return out


def test_header_is_an_eighth_table():
    from pyglm_amd import _lib
    assert sorted(_lib.SIMULATE_OFFSET_FUNCTIONS) == ["pgl_latent_prior_paths", "pgl_simulate_offset", "pgl_simulate_offset_build"]
    assert _lib.SIMULATE_OFFSET_CONSTANTS == {"PGL_PURPOSE_SIM_LATENT": 7, "PGL_SIM_LATENT_MAX": 8}
    assert _lib.PGL_PURPOSE_SIM_LATENT == 7
    for other in (_lib.FUNCTIONS, _lib.DISPERSION_FUNCTIONS, _lib.DIAGNOSTICS_FUNCTIONS, _lib.SBM_FUNCTIONS, _lib.COVARIATES_FUNCTIONS,
                  _lib.LATENTS_FUNCTIONS, _lib.LATENT_DYNAMICS_FUNCTIONS):
        assert not set(_lib.SIMULATE_OFFSET_FUNCTIONS) & set(other)
    sim, off = _lib.PARAMS["pgl_simulate"], _lib._params("pgl_simulate_offset")
    assert off == sim[:-1] + ["Off", "ldo_t", "ldo_r", "hip_stream"]           # pgl_simulate's arguments plus the offset
    assert _lib.SIMULATE_OFFSET_FUNCTIONS["pgl_simulate_offset"][1][-4:] == [("Off", ctypes.c_void_p), ("ldo_t", ctypes.c_long), ("ldo_r", ctypes.c_long),
                                                                              ("hip_stream", ctypes.c_void_p)]
    assert _lib._params("pgl_latent_prior_paths") == ["X", "ldx_r", "R", "rep0", "t0", "Tc", "Q", "phi", "s", "carry", "has_carry", "z_override", "seed",
                                                      "hip_stream"]
    assert _lib._params("pgl_simulate_offset_build") == ["S", "lds", "X", "ldx_r", "Beta", "ldn", "Off", "ldo_t", "ldo_r", "Tc", "N", "K_obs", "Q", "R",
                                                         "hip_stream"]
    assert _lib.ABI_VERSION == 11 and len(_lib.FUNCTIONS) == 65 and _lib.HEADER_SIMULATE_OFFSET.endswith("pyglm_hip_simulate_offset.h")
