"""Learning the negative-binomial dispersion xi on the host: the NumPy definition of the CRT step (pyglm_amd/dispersion.py), its law, the
regression / model plumbing around it and the second header of the C ABI.  No GPU: the population model runs on the oracle-backed engine."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest

from oracle import pyglm_oracle as orc
from pyglm_amd import dispersion as disp
from pyglm_amd import simulate as sim
from tests._oracle_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class XiOracleEngine(OracleEngine):
    """the oracle-backed engine with one xi per local neuron and set_obs_param: what a model that learns xi needs of an engine_factory
    engine.  It is no device engine (no fold_data), so the model folds through dispersion.dispersion_host from psi(...)."""

    def __init__(self, N, B, n0=0, n1=None, obs="bernoulli", xi=1.0, **kw):
        super(XiOracleEngine, self).__init__(N, B, n0, n1, obs=obs, xi=xi, **kw)
        self.pushes = 0
        self.xi_loc = self._local(xi)

    def _local(self, xi):
        v = np.asarray(xi, dtype=np.float64).reshape(-1)
        if v.size == 1:
            return np.full(self.nloc, float(v[0]))
        return (v[self.n0:self.n1] if v.size == self.N else v).copy()

    def set_obs_param(self, xi):
        self.pushes += 1
        self.xi_loc = self._local(xi)
        assert self.xi_loc.shape == (self.nloc,)

    def _reg(self, a, W, b, i, **hyp):
        r = orc.Regression(self.N, self.B, obs=self.obs, xi=float(self.xi_loc[i]), eta=self.eta[i], **hyp)
        r.a, r.W, r.b = np.asarray(a[i]).astype(bool).copy(), np.asarray(W[i], float).copy(), np.atleast_1d(np.asarray(b, float)[i]).copy()
        return r


def nb_counts(rng, xi, psi):
    """y ~ NB(xi, sigma(psi)): mean xi e^psi"""
    return rng.negative_binomial(xi, 1.0 / (1.0 + np.exp(psi))).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the definition on hand-made columns
def test_zero_one_column_draws_nothing(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a 0/1 column must not touch a uniform")
    monkeypatch.setattr(sim, "philox4x32_10", boom)
    y = np.array([0, 1, 1, 0, 1, 0, 0, 1.0])[:, None]
    psi = np.linspace(-3, 2, 8)[:, None]
    L, S = disp.dispersion_host(psi, y, 0.7, seed=3, sweep=2, neuron0=5, elem0=11)
    assert L.dtype == np.int64 and L.tolist() == [4]
    np.testing.assert_allclose(S[0], np.log1p(np.exp(psi[:, 0])).sum(), rtol=1e-14)


def test_count_two_uses_u0_of_the_documented_stream():
    seed, sweep, neuron, elem0, t, xi = 0x1234567890ABCDEF, 7, 9, 1000, 3, 0.8
    y = np.zeros((6, 1))
    y[t, 0] = 2.0
    L, _ = disp.dispersion_host(np.zeros((6, 1)), y, xi, seed, sweep, neuron, elem0)
    # counter words written out: (call 0 | purpose 4 << 24, element elem0 + t, neuron, sweep), key = seed; u0 from words 0, 1
    w = sim.philox4x32_10(np.uint64(4 << 24), np.uint64(elem0 + t), np.uint64(neuron), np.uint64(sweep), seed)
    u0 = ((((int(w[1]) << 32) | int(w[0])) >> 11) + 0.5) / 2.0 ** 53
    assert L[0] == 1 + int(u0 * (xi + 1) < xi)
    # both outcomes occur over the elements, each as its own u0 says
    T = 64
    Y = np.full((T, 1), 2.0)
    L, _ = disp.dispersion_host(np.zeros((T, 1)), Y, xi, seed, sweep, neuron, elem0)
    w = sim.philox4x32_10(np.uint64(4 << 24), elem0 + np.arange(T, dtype=np.uint64), np.uint64(neuron), np.uint64(sweep), seed)
    u = sim._unit(w[0], w[1])
    opened = int(np.count_nonzero(u * (xi + 1) < xi))
    assert 0 < opened < T and L[0] == T + opened


def test_count_rule_nan_negative_fractional():
    y = np.array([np.nan, -3.0, 0.4, 0.999, 1.0, 1.9, 2.5, -0.0, np.inf])
    assert disp.cell_counts(y).tolist() == [0, 0, 0, 0, 1, 1, 2, 0, disp.MAX_COUNT]
    Y = np.array([np.nan, -3.0, 0.4, 1.9, 2.5])[:, None]
    Yi = np.array([0.0, 0.0, 0.0, 1.0, 2.0])[:, None]
    psi = np.zeros((5, 1))
    a, b = disp.dispersion_host(psi, Y, 1.3, 5, 1, 2, 0), disp.dispersion_host(psi, Yi, 1.3, 5, 1, 2, 0)
    assert a[0].tolist() == b[0].tolist() and a[1][0] == b[1][0]


def test_second_data_set_continues_at_elem0_and_columns_are_their_own():
    rng = np.random.default_rng(4)
    T, N = 300, 4
    xi = np.array([0.3, 2.0, 7.0, 50.0])
    psi = rng.standard_normal((T, N)) - 1
    Y = nb_counts(rng, 3.0, rng.standard_normal((T, N)) + 0.5)
    assert (Y >= 2).sum() > 100
    Lw, Sw = disp.dispersion_host(psi, Y, xi, 9, 4, 20, 0)
    # two data sets: the second starts at the element behind the first
    L1, S1 = disp.dispersion_host(psi[:120], Y[:120], xi, 9, 4, 20, 0)
    L2, S2 = disp.dispersion_host(psi[120:], Y[120:], xi, 9, 4, 20, 120)
    assert (L1 + L2).tolist() == Lw.tolist()
    L2w, _ = disp.dispersion_host(psi[120:], Y[120:], xi, 9, 4, 20, 0)
    assert L2w.tolist() != L2.tolist()
    # column j of the wide call is the column alone with neuron0 + j
    for j in range(N):
        Lj, Sj = disp.dispersion_host(psi[:, j:j + 1], Y[:, j:j + 1], xi[j], 9, 4, 20 + j, 0)
        assert Lj[0] == Lw[j] and Sj[0] == Sw[j]
    # another sweep, another stream
    assert disp.dispersion_host(psi, Y, xi, 9, 5, 20, 0)[0].tolist() != Lw.tolist()


def test_softplus_does_not_overflow():
    x = np.array([-800.0, -30.0, 0.0, 30.0, 800.0])
    sp = disp.softplus(x)
    assert np.all(np.isfinite(sp)) and sp[0] == 0.0 and sp[4] == 800.0 and sp[2] == np.log(2.0)


# ------------------------------------------------------------------------------------------------ the law
@pytest.mark.parametrize("m", [1, 2, 7, 200])
@pytest.mark.parametrize("xi", [0.3, 2.0, 50.0])
def test_table_counts_follow_the_crt_law(m, xi):
    """sum of l over 20 000 cells of count m: within 5 binomial standard deviations of 20 000 sum_{i < m} xi / (xi + i)"""
    cells = 20000
    Y = np.full((cells, 1), float(m))
    L, _ = disp.dispersion_host(np.zeros((cells, 1)), Y, xi, seed=100 + m, sweep=1, neuron0=0, elem0=0)
    p = xi / (xi + np.arange(m))
    mean, sd = cells * p.sum(), np.sqrt(cells * np.sum(p * (1 - p)))
    assert abs(L[0] - mean) <= 5 * sd, (L[0], mean, sd)
    assert np.isclose(disp.table_mean(m, xi), p.sum())


def test_conditional_alone_recovers_xi():
    """psi known, only xi | L, S iterated: T = 20 000, psi = -3 + 0.5 N(0, 1), y ~ NB(2, sigma(psi)); from xi = 1, 300 draws, the first 100
    dropped: |mean - 2| <= 4 standard deviations of the chain, and the standard deviation is below 0.1"""
    from pyglm_amd.regression import SparseNegativeBinomialRegression
    rng = np.random.default_rng(12)
    T, truth = 20000, 2.0
    psi = (-3.0 + 0.5 * rng.standard_normal(T))[:, None]
    Y = nb_counts(rng, truth, psi)
    np.random.seed(0)
    reg = SparseNegativeBinomialRegression(1, 1, xi=1.0, xi_prior=(1.0, 1.0))
    chain = []
    for it in range(300):
        L, S = disp.dispersion_host(psi, Y, reg.xi, seed=77, sweep=it, neuron0=0, elem0=0)
        reg.xi = disp.draw_xi(reg, int(L[0]), float(S[0]), 77, it, 0)
        chain.append(reg.xi)
    kept = np.array(chain[100:])
    print("xi chain: mean %.4f sd %.4f" % (kept.mean(), kept.std()))
    assert kept.std() < 0.1
    assert abs(kept.mean() - truth) <= 4 * kept.std()


# ------------------------------------------------------------------------------------------------ regressions and models
def _nb_model(N=4, B=1, T=300, prior=(2.0, 1.0), xi=1.0, seed=3, factory=XiOracleEngine, rseed=0):
    from pyglm_amd.models import SparseNegativeBinomialGLM
    np.random.seed(rseed)
    kw = dict(S_w=2.0, mu_b=-1.5, xi=xi)
    if prior is not None:
        kw["xi_prior"] = prior
    model = SparseNegativeBinomialGLM(N, B=B, basis=np.ones((3, B)) / 3.0, regression_kwargs=kw, seed=seed, engine_factory=factory)
    rng = np.random.default_rng(1)
    Y = nb_counts(rng, 2.0, -1.0 + 0.3 * rng.standard_normal((T, N)))
    return model, Y


def test_fixed_xi_is_untouched():
    from pyglm_amd import regression as R
    np.random.seed(0)
    regs = [R.SparseNegativeBinomialRegression(3, 1, xi=1.5) for _ in range(3)]
    assert all(r.xi_prior is None for r in regs) and not R.learns_xi(regs)
    assert R.device_obs(regs) == ("negbin", 1.5)                      # a scalar, as before
    regs[1].xi = 2.5
    kind, par = R.device_obs(regs)
    assert kind == "negbin" and par.tolist() == [1.5, 2.5, 1.5]
    regs[1].check_data(np.array([0.5, -1.0, 1e30]))                   # no new check without xi_prior
    # the model: no push, no xi step, and _check_obs still refuses a changed xi
    model, Y = _nb_model(prior=None)
    model.add_data(Y)
    model.resample_model()
    model.resample_model()
    assert model.engine.pushes == 0 and all(r.xi == 1.0 for r in model.regressions) and not model._learns_xi()
    plain, _ = _nb_model(prior=None, factory=OracleEngine)            # an engine without set_obs_param runs the same chain
    plain.add_data(Y)
    plain.resample_model()
    plain.resample_model()
    np.testing.assert_array_equal(plain.weights, model.weights)
    np.testing.assert_array_equal(plain.adjacency, model.adjacency)
    model.regressions[0].xi = 3.0
    with pytest.raises(ValueError, match="build a new model"):
        model.resample_model()


def test_xi_prior_validation_and_posterior():
    from pyglm_amd import regression as R
    np.random.seed(0)
    r = R.SparseNegativeBinomialRegression(2, 1, xi=0.5, xi_prior=(3, 0.25))
    assert r.xi_prior == (3.0, 0.25) and r.xi_posterior(10, 2.5) == (13.0, 2.75)
    for bad in [(0.0, 1.0), (1.0, -1.0), (1.0,), "ab"]:
        with pytest.raises((ValueError, TypeError)):
            R.SparseNegativeBinomialRegression(2, 1, xi_prior=bad)
    r.check_data(np.array([0.0, 3.0, 2.0 ** 24 - 1]))
    for bad in [np.array([0.5]), np.array([-1.0]), np.array([2.0 ** 24]), np.array([np.nan])]:
        with pytest.raises(ValueError, match="integers in"):
            r.check_data(bad)
    kind, par = R.device_obs([r, R.SparseNegativeBinomialRegression(2, 1, xi=0.5)])
    assert kind == "negbin" and np.ndim(par) == 1 and par.tolist() == [0.5, 0.5]      # per regression as soon as one of them learns
    model, Y = _nb_model()
    Y[5, 2] = 1.5
    with pytest.raises(ValueError, match="integers in"):
        model.add_data(Y)


def test_xi_prior_in_hooks_mode_is_refused():
    from pyglm_amd import regression as R
    from pyglm_amd.models import NonlinearAutoregressiveModel
    np.random.seed(0)
    mixed = [R.SparseNegativeBinomialRegression(2, 1, xi_prior=(1.0, 1.0)), R.SparseBernoulliRegression(2, 1)]
    with pytest.raises(ValueError, match="hooks mode"):
        R.device_obs(mixed)
    with pytest.raises(ValueError, match="regression 0 learns its xi"):
        NonlinearAutoregressiveModel(2, mixed, B=1, engine_factory=XiOracleEngine).engine
    own = [R.SparseNegativeBinomialRegression(2, 1), R.SparseNegativeBinomialRegression(2, 1, xi_prior=(1.0, 1.0))]
    own[0].b_func = lambda y: y + 2.0                                 # a hook set on an instance puts the list into hooks mode
    with pytest.raises(ValueError, match="regression 1 learns its xi"):
        R.device_obs(own)
    # an engine that cannot take a new xi is refused by name
    model, Y = _nb_model(factory=OracleEngine)
    model.add_data(Y)
    with pytest.raises(ValueError, match="set_obs_param"):
        model.resample_model()


def test_gamma_lanes():
    from pyglm_amd.engine import make_gamma_draws
    eta = make_gamma_draws(5, 3, [0, 7], 2.5)
    assert np.array_equal(eta, make_gamma_draws(5, 3, [0, 7], 2.5, lane=1))
    rng = np.random.Generator(np.random.Philox(key=5, counter=[3, 7, 1, 0]))          # lane 1 keeps its bits
    assert eta[1] == rng.standard_gamma(2.5)
    xi = make_gamma_draws(5, 3, [0, 7], 2.5, lane=disp.XI_LANE)
    assert disp.XI_LANE == 2 and not np.any(xi == eta)
    assert xi[1] == np.random.Generator(np.random.Philox(key=5, counter=[3, 7, 2, 0])).standard_gamma(2.5)


def test_model_step_is_the_definition_and_readers_follow_xi():
    """one sweep of a learning model on the oracle engine: xi is the host draw from dispersion_host at the new state; a second sweep runs;
    log_likelihood, simulate, time rescaling and the summary read the moved xi"""
    model, Y = _nb_model(T=250)
    model.add_data(Y)
    gof = model.time_rescaling(bins=8, seed=2)
    acc = model.summarize(rates=False)
    model.resample_model()
    a, W, b = model._local_state()
    L, S = disp.dispersion_host(model.engine.psi(a, W, b, 0), Y, 1.0, model.seed, 0, 0, 0)
    xi = np.array([r.xi for r in model.regressions])
    want = [disp.draw_xi(r, int(L[i]), float(S[i]), model.seed, 0, i) for i, r in enumerate(model.regressions)]
    assert xi.tolist() == want and np.all(xi != 1.0)
    assert model.engine.xi_loc.tolist() == xi.tolist() and model._engine_mode[1].tolist() == xi.tolist()
    # a fresh fixed-xi model at that state
    fixed, _ = _nb_model(T=250, prior=None)
    for r, x in zip(fixed.regressions, xi):
        r.xi = float(x)
    fixed.add_data(Y)
    fixed._store_rows(0, 4, model.adjacency, model.weights, model.biases)
    assert model.log_likelihood() == fixed.log_likelihood()
    assert model.log_likelihood([Y[:100]]) == fixed.log_likelihood([Y[:100]])
    s1, s2 = model.simulate(40, replicates=2, seed=4, gpu=False), fixed.simulate(40, replicates=2, seed=4, gpu=False)
    np.testing.assert_array_equal(s1.Y, s2.Y)
    gof.collect()
    g2 = fixed.time_rescaling(bins=8, seed=2)
    g2.collect()
    np.testing.assert_array_equal(gof.hist_last, g2.hist_last)
    np.testing.assert_array_equal(gof.zsum_last, g2.zsum_last)
    acc.collect()
    model.resample_model()                                            # _check_obs accepts the moved xi
    xi2 = np.array([r.xi for r in model.regressions])
    assert np.all(xi2 != xi)
    acc.collect()
    np.testing.assert_allclose(acc.xi_mean, (xi + xi2) / 2, rtol=1e-15)
    np.testing.assert_allclose(acc.xi_var, np.var([xi, xi2], axis=0), rtol=1e-12)
    # a user's r.xi = ... and set_state() take effect at the next sweep
    state = model.get_state()
    model.regressions[2].xi = 9.0
    model.resample_model()
    model.set_state(state)
    model.resample_model()
    assert np.all(np.array([r.xi for r in model.regressions]) != xi2)
    # a fixed-xi neuron inside a learning model keeps its xi
    mix, _ = _nb_model(T=250)
    mix.regressions[1].xi_prior = None
    mix.add_data(Y)
    mix.resample_model()
    got = [r.xi for r in mix.regressions]
    assert got[1] == 1.0 and all(g != 1.0 for i, g in enumerate(got) if i != 1)
    bern = __import__("pyglm_amd.models", fromlist=["x"]).SparseBernoulliGLM(2, B=1, engine_factory=OracleEngine)
    bern.add_data((np.random.rand(50, 2) < 0.3).astype(float))
    s = bern.summarize(rates=False)
    s.collect()
    assert np.all(np.isnan(s.xi_mean)) and np.all(np.isnan(s.xi_var))


def test_checks_built_before_xi_moved_follow_it():
    """conditional_check, summarize(pointwise=True) and means of a learning model, each built BEFORE the sweep that moves xi, against the same
    objects of a fresh fixed-xi model at the moved xi and the same state: equal to the last bit (the host paths, on the oracle engine)"""
    model, Y = _nb_model(T=250)
    model.add_data(Y)
    cp = model.conditional_check([1, 3], replicates=3, seed=6, start=20, stop=200, gpu=False)
    acc = model.summarize(rates=True, pointwise=True)
    model.resample_model()
    xi = np.array([r.xi for r in model.regressions])
    assert np.all(xi != 1.0)
    fixed, _ = _nb_model(T=250, prior=None)
    for r, x in zip(fixed.regressions, xi):
        r.xi = float(x)
    fixed.add_data(Y)
    fixed._store_rows(0, 4, model.adjacency, model.weights, model.biases)
    np.testing.assert_array_equal(model.means[0], fixed.means[0])
    cp.collect()
    cp.collect()
    c2 = fixed.conditional_check([1, 3], replicates=3, seed=6, start=20, stop=200, gpu=False)
    c2.collect()
    c2.collect()
    np.testing.assert_array_equal(cp.rate_mean, c2.rate_mean)
    np.testing.assert_array_equal(cp.rate_std, c2.rate_std)
    np.testing.assert_array_equal(cp.log_score()["per_bin"], c2.log_score()["per_bin"])
    stale, _ = _nb_model(T=250, prior=None)                          # ... and they are not what the constructor's xi = 1 gives
    stale.add_data(Y)
    stale._store_rows(0, 4, model.adjacency, model.weights, model.biases)
    c3 = stale.conditional_check([1, 3], replicates=3, seed=6, start=20, stop=200, gpu=False)
    c3.collect()
    assert not np.array_equal(c3.log_score()["per_neuron"], c2.log_score()["per_neuron"])
    a2 = fixed.summarize(rates=True, pointwise=True)
    for a in (acc, a2):
        a.collect()
        a.collect()
    assert acc.log_likelihoods == a2.log_likelihoods
    np.testing.assert_array_equal(acc.lppd()["per_neuron"], a2.lppd()["per_neuron"])
    w1, w2 = acc.waic(), a2.waic()
    assert w1["waic"] == w2["waic"] and w1["p_waic"] == w2["p_waic"]
    np.testing.assert_array_equal(acc.rate_mean[0], a2.rate_mean[0])
    # one sample's lppd is the log-likelihood: the pointwise terms and the returned total use the same xi
    a3 = model.summarize(rates=False, pointwise=True)
    ll = a3.collect()
    np.testing.assert_allclose(a3.lppd()["total"], ll, rtol=1e-12)
    # a user's r.xi = ... reaches means without a sweep
    model.regressions[0].xi, fixed.regressions[0].xi = 3.25, 3.25
    fixed._engine_mode = __import__("pyglm_amd.regression", fromlist=["x"]).device_obs(fixed.regressions)
    np.testing.assert_array_equal(model.means[0], fixed.means[0])


# ------------------------------------------------------------------------------------------------ the second header
def test_second_header_binds():
    from pyglm_amd import _lib
    assert sorted(_lib.DISPERSION_FUNCTIONS) == ["pgl_dispersion_fold", "pgl_dispersion_work_bytes"]
    assert _lib.DISPERSION_CONSTANTS == dict(PGL_PURPOSE_DISPERSION=4, PGL_DISPERSION_ROWS=256, PGL_DISPERSION_COOP=128,
                                             PGL_DISPERSION_MAX_COUNT=2 ** 24)
    assert _lib.PGL_DISPERSION_COOP % 64 == 0 and _lib.PGL_DISPERSION_ROWS == disp.ROWS
    # the tables of pyglm_hip.h describe that header alone
    assert not set(_lib.DISPERSION_FUNCTIONS) & set(_lib.FUNCTIONS) and not set(_lib.DISPERSION_CONSTANTS) & set(_lib.CONSTANTS)
    assert "pgl_dispersion_fold" not in _lib.SIGNATURES and "pgl_dispersion_fold" not in _lib.PARAMS
    restype, params = _lib.DISPERSION_FUNCTIONS["pgl_dispersion_fold"]
    assert restype is ctypes.c_int and [p for p, _ in params] == ["Psi", "ldn", "bias", "Y", "T", "nloc", "xi", "seed", "sweep", "neuron0", "elem0",
                                                                   "L", "S", "accumulate", "work", "hip_stream"]
    assert dict(params)["seed"] is ctypes.c_uint64 and dict(params)["ldn"] is ctypes.c_long and dict(params)["L"] is ctypes.c_void_p
    assert _lib.DISPERSION_FUNCTIONS["pgl_dispersion_work_bytes"] == (ctypes.c_size_t, [("nloc", ctypes.c_int), ("T", ctypes.c_int)])
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "pgl_dispersion_fold") and hasattr(raw, "pgl_dispersion_work_bytes")
    lib = _lib.load()
    assert lib.pgl_dispersion_fold.argtypes == [t for _, t in params] and lib.pgl_dispersion_work_bytes.restype is ctypes.c_size_t
    # host-side arithmetic only: the workgroups' partials, a double and a 64-bit integer per (row block, column)
    assert lib.pgl_dispersion_work_bytes(70, 3 * 256 + 17) == 4 * 70 * 16 and lib.pgl_dispersion_work_bytes(5, 0) == 16
    assert lib.pgl_dispersion_work_bytes(0, 10) == 0 and lib.pgl_dispersion_work_bytes(4, -1) == 0

    class Untouched(object):
        def __getattr__(self, name):
            raise AssertionError("the library was touched: %s" % name)
    keep, _lib._lib = _lib._lib, Untouched()
    try:
        kw = dict.fromkeys(_lib.DISPERSION_PARAMS["pgl_dispersion_fold"])
        with pytest.raises(AssertionError, match="pgl_dispersion_fold"):          # every keyword placed: the call reaches the library
            _lib.call("pgl_dispersion_fold", **kw)
        kw.pop("xi")
        with pytest.raises(TypeError, match="missing parameter 'xi'"):
            _lib.call("pgl_dispersion_fold", **kw)
        with pytest.raises(TypeError, match="has no parameter 'qpar'"):
            _lib.call("pgl_dispersion_fold", qpar=None, **kw)
    finally:
        _lib._lib = keep


def test_refused_arguments_on_the_host():
    """the argument checks run before anything touches a device: PGL_ERR_ARG, with a message, and nothing is written"""
    from pyglm_amd import _lib
    lib = _lib.load()
    L, S = (ctypes.c_longlong * 2)(7, 7), (ctypes.c_double * 2)(7.0, 7.0)
    p = lambda x: ctypes.c_void_p(ctypes.addressof(x))
    base = dict(Psi=None, ldn=2, bias=None, Y=None, T=0, nloc=2, xi=p(S), seed=1, sweep=0, neuron0=0, elem0=0, L=p(L), S=p(S), accumulate=0,
                work=None, hip_stream=None)
    for bad in [dict(nloc=0), dict(T=-1), dict(ldn=1), dict(xi=None), dict(L=None), dict(S=None), dict(accumulate=2), dict(T=5),
                dict(T=2 ** 31 - 100)]:
        with pytest.raises(_lib.PglError, match="argument check failed"):
            _lib.call("pgl_dispersion_fold", **dict(base, **bad))
    assert list(L) == [7, 7] and list(S) == [7.0, 7.0]


# ------------------------------------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_learning_model(world, rank, port, out_path):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    model, Y = _nb_model(N=5, B=2, T=300, seed=11)
    model.regressions[3].xi_prior = None                              # a fixed-xi neuron among the learning ones
    model.regressions[3].xi = 1.7
    model.add_data(Y)
    xis, lls = [], []
    for _ in range(3):
        model.resample_model()
        xis.append([r.xi for r in model.regressions])
        lls.append(model.log_likelihood())
    acc = model.summarize(rates=False)
    acc.collect()
    np.savez(out_path % rank, xi=np.array(xis), lls=np.array(lls), W=model.weights, A=model.adjacency, xi_mean=acc.xi_mean)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _worker(rank, world, port, out_path):
    _run_learning_model(world, rank, port, out_path)


@pytest.mark.timeout(300)
def test_two_ranks_learn_the_same_xi(tmp_path):
    import torch.multiprocessing as mp
    one, two = str(tmp_path / "one%d.npz"), str(tmp_path / "two%d.npz")
    _run_learning_model(1, 0, 0, one)
    mp.spawn(_worker, args=(2, _free_port(), two), nprocs=2, join=True)
    a, r0, r1 = np.load(one % 0), np.load(two % 0), np.load(two % 1)
    for k in a.files:
        np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)            # both ranks hold the same state
    np.testing.assert_array_equal(a["xi"], r0["xi"])                      # ... and it is the one-rank run's
    np.testing.assert_array_equal(a["lls"], r0["lls"])
    np.testing.assert_allclose(a["W"], r0["W"], rtol=1e-12, atol=1e-12)
    assert np.all(a["xi"][:, 3] == 1.7) and np.all(np.delete(a["xi"], 3, axis=1) != 1.0) and a["xi"].shape == (3, 5)
    np.testing.assert_array_equal(a["xi_mean"], a["xi"][-1])
