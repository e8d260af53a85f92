"""Which observation model the device runs for a list of regressions (regression.device_obs), the binomial regression's hooks against
the reference's vectors, the checks of binomial data, and the keyword arguments a user's engine factory receives.  CPU only."""
import numpy as np
import pytest

from pyglm_amd import regression as R
from pyglm_amd import models as M
from tests.test_oracle_binomial import golden_binom  # noqa: F401  (fixture)


def _regs(cls, N=3, B=1, **kw):
    np.random.seed(0)
    return [cls(N, B, **kw) for _ in range(N)]


class _Inherits(R.SparseBernoulliRegression):
    pass


class _InheritsNB(R.SparseNegativeBinomialRegression):
    pass


class _OwnB(R.SparseBernoulliRegression):
    def b_func(self, data):
        return 1.0 + data


class _Free(R._SparsePGRegressionBase):           # a user's model on the base class: _obs is None
    def a_func(self, y):
        return y

    def b_func(self, y):
        return np.ones_like(y, dtype=float)

    def c_func(self, y):
        return 1.0


def test_pure_builtin_lists():
    assert R.device_obs(_regs(R.SparseBernoulliRegression)) == ("bernoulli", 1.0)
    assert R.device_obs(_regs(R.BernoulliRegression)) == ("bernoulli", 1.0)
    assert R.device_obs(_regs(R.SparseNegativeBinomialRegression, xi=2.5)) == ("negbin", 2.5)
    assert R.device_obs(_regs(R.SparseBinomialRegression, n=7)) == ("binomial", 7.0)
    assert R.device_obs(_regs(R.BinomialRegression, n=3)) == ("binomial", 3.0)
    assert R.device_obs(_regs(R.SparseGaussianRegression)) == ("gaussian", 1.0)


def test_per_neuron_parameters():
    regs = [R.SparseNegativeBinomialRegression(3, 1, xi=x) for x in (1.0, 2.0, 1.0)]
    obs, xi = R.device_obs(regs)
    assert obs == "negbin" and isinstance(xi, np.ndarray)
    np.testing.assert_array_equal(xi, [1.0, 2.0, 1.0])
    regs = [R.SparseBinomialRegression(2, 1, n=k) for k in (4, 9)]
    obs, n = R.device_obs(regs)
    assert obs == "binomial"
    np.testing.assert_array_equal(n, [4.0, 9.0])
    assert R.same_obs(("negbin", np.array([2.0, 2.0])), ("negbin", 2.0)) and not R.same_obs(("negbin", 2.0), ("negbin", 3.0))


def test_subclasses_without_override_keep_the_builtin_mode():
    assert R.device_obs(_regs(_Inherits)) == ("bernoulli", 1.0)
    assert R.device_obs(_regs(_InheritsNB, xi=3.0)) == ("negbin", 3.0)


def test_overridden_hooks_run_the_hooks_mode():
    assert R.device_obs(_regs(_OwnB))[0] == "hooks"
    assert R.device_obs(_regs(_Free))[0] == "hooks"
    regs = _regs(R.SparseBernoulliRegression)
    regs[1].c_func = lambda y: 2.0                  # a hook set on one instance
    assert R.device_obs(regs)[0] == "hooks"
    assert R.device_obs(regs[:1])[0] == "bernoulli"
    mixed = _regs(R.SparseBernoulliRegression, N=2) + _regs(R.SparseBinomialRegression, N=2, n=4)
    assert R.device_obs(mixed)[0] == "hooks"
    assert R.device_obs(_regs(R.SparseBernoulliRegression) + _regs(R.SparseNegativeBinomialRegression, xi=2.0))[0] == "hooks"


def test_gaussian_with_pg_raises_and_unknown_types_raise():
    with pytest.raises(ValueError):
        R.device_obs(_regs(R.SparseGaussianRegression, N=2) + _regs(R.SparseBernoulliRegression, N=2))
    with pytest.raises(TypeError):
        R.device_obs([object()])


@pytest.mark.parametrize("tag", ["b0", "b1"])
def test_binomial_hooks_reproduce_the_reference(golden_binom, tag):  # noqa: F811
    g = golden_binom
    N, B = g[tag + "_mu_w"].shape
    n = int(g[tag + "_n"])
    r = R.SparseBinomialRegression(N, B, n=n)
    y, psi = g[tag + "_y"], g[tag + "_psi"]
    np.testing.assert_array_equal(r.b_func(y), g[tag + "_pg_b"])
    np.testing.assert_allclose(r.kappa(None, y), g[tag + "_kappa"], rtol=1e-15, atol=0)
    # log c = ll - a psi + b log(1 + e^psi), from the reference's per-bin log-likelihood
    logc = g[tag + "_ll"] - y * psi + n * np.log1p(np.exp(psi))
    np.testing.assert_allclose(np.log(r.c_func(y)), logc, rtol=1e-11, atol=1e-11)
    A, Bv, logC = R.obs_terms([r], y[:, None])
    np.testing.assert_array_equal(A[:, 0], y)
    np.testing.assert_array_equal(Bv[:, 0], g[tag + "_pg_b"])


def test_binomial_rejects_invalid_data():
    from tests._oracle_engine import OracleEngine
    with pytest.raises(ValueError):
        R.SparseBinomialRegression(2, 1, n=2.5)
    np.random.seed(1)
    model = M.SparseBinomialGLM(3, B=2, regression_kwargs=dict(n=3), engine_factory=OracleEngine, seed=1)
    Y = np.zeros((50, 3))
    Y[4, 1] = 4.0                                   # y > n
    with pytest.raises(ValueError):
        model.add_data(Y)
    Y[4, 1] = 1.5                                   # not an integer
    with pytest.raises(ValueError):
        model.add_data(Y)
    Y[4, 1] = -1.0
    with pytest.raises(ValueError):
        model.add_data(Y)
    r = R.SparseBinomialRegression(3, 2, n=3)
    with pytest.raises(ValueError):
        r.resample([(np.zeros((50, 3, 2)), Y[:, 1])])
    with pytest.raises(ValueError):                 # hooks that are not finite on the data
        R.obs_terms([r], np.full((5, 1), 7.0))


def test_binomial_rvs_and_mean():
    r = R.SparseBinomialRegression(2, 1, n=6)
    np.random.seed(3)
    y = r.rvs(psi=np.array([-1.0, 0.0, 2.0, 30.0]))
    assert y.dtype == float and np.all((y >= 0) & (y <= 6) & (y == np.floor(y))) and y[3] == 6.0


def _recording_factory(log):
    from tests._oracle_engine import OracleEngine

    class Rec(OracleEngine):
        def add_data(self, Y, X=None, basis=None, **kw):
            log.append(("add_data", sorted(kw)))
            return super(Rec, self).add_data(Y, X=X, basis=basis)

    def factory(N, B, n0, n1, **kw):
        log.append(("init", dict(kw)))
        return Rec(N, B, n0, n1, **kw)
    return factory


@pytest.mark.parametrize("cls,kw,want", [(M.SparseBernoulliGLM, {}, dict(obs="bernoulli", xi=1.0)),
                                         (M.SparseNegativeBinomialGLM, dict(xi=2.5), dict(obs="negbin", xi=2.5)),
                                         (M.SparseGaussianGLM, {}, dict(obs="gaussian", xi=1.0)),
                                         (M.SparseBinomialGLM, dict(n=4), dict(obs="binomial", xi=4.0))])
def test_engine_factory_receives_the_builtin_arguments(cls, kw, want):
    log = []
    np.random.seed(2)
    model = cls(3, B=2, regression_kwargs=kw, engine_factory=_recording_factory(log), seed=1)
    model.add_data(np.zeros((40, 3)))
    assert log[0] == ("init", want) and type(log[0][1]["xi"]) is float
    assert log[1] == ("add_data", [])                # no obs_terms outside the hooks mode


def test_engine_factory_in_hooks_mode_gets_the_terms():
    log = []
    np.random.seed(2)
    regs = [_OwnB(3, 2) for _ in range(3)]
    model = M.GLM(3, regs, B=2, engine_factory=_recording_factory(log), seed=1)
    model.add_data(np.zeros((40, 3)))
    assert log[0] == ("init", dict(obs="hooks", xi=1.0)) and log[1] == ("add_data", ["obs_terms"])
    assert model.engine_obs() == "hooks"


def test_swapping_in_another_model_raises():
    from tests._oracle_engine import OracleEngine
    np.random.seed(2)
    model = M.SparseBernoulliGLM(3, B=2, engine_factory=OracleEngine, seed=1)
    model.add_data((np.random.rand(60, 3) < 0.2).astype(float))
    model.resample_model()
    model.regressions[1] = R.SparseNegativeBinomialRegression(3, 2, xi=2.0)
    with pytest.raises(ValueError, match="observation model"):
        model.resample_model()
