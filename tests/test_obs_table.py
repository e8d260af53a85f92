"""The table of the built-in observation models (regression.MODELS) against the literal codes of include/pyglm_hip.h, and what derives from it."""
import types

import numpy as np
import pytest

from pyglm_amd import regression, rescale, simulate
from pyglm_amd.models import NonlinearAutoregressiveModel
from pyglm_amd.regression import (MODELS, BernoulliRegression, SparseBernoulliRegression, SparseBinomialRegression, SparseGaussianRegression,
                                  SparseNegativeBinomialRegression, is_builtin)
from pyglm_amd.utils.utils import logistic

N, B = 4, 2
#           name         class                             device  sim kind  link  generate
LITERALS = [("bernoulli", SparseBernoulliRegression,        0,      0,        0,    0),
            ("negbin",    SparseNegativeBinomialRegression, 1,      2,        2,    None),
            ("gaussian",  SparseGaussianRegression,         2,      1,        1,    1),
            ("binomial",  SparseBinomialRegression,         3,      3,        3,    None)]


def test_the_table_holds_the_four_models_with_the_codes_of_the_header():
    assert sorted(MODELS) == ["bernoulli", "binomial", "gaussian", "negbin"]
    for name, cls, device, sim_kind, link, generate in LITERALS:
        m = MODELS[name]
        assert (m.name, m.cls, m.device, m.sim_kind, m.link, m.generate) == (name, cls, device, sim_kind, link, generate)
    assert [MODELS[k].param for k, *_ in LITERALS] == [None, "xi", None, "n"]
    assert [MODELS[k].events for k, *_ in LITERALS] == [True, True, False, True]
    with pytest.raises(AttributeError):
        MODELS["bernoulli"].device = 5


def test_the_names_that_derive_from_the_table_keep_their_values():
    from pyglm_amd.engine import GibbsEngine
    assert GibbsEngine.OBS == {"bernoulli": 0, "negbin": 1, "gaussian": 2, "binomial": 3, "hooks": 4}
    assert (regression.OBS_BERNOULLI, regression.OBS_NEGBIN, regression.OBS_GAUSSIAN, regression.OBS_BINOMIAL, regression.OBS_HOOKS) == (0, 1, 2, 3, 4)
    assert (simulate.KIND_BERNOULLI, simulate.KIND_GAUSSIAN, simulate.KIND_NEGBIN, simulate.KIND_BINOMIAL) == (0, 1, 2, 3)
    assert simulate.KINDS == ("bernoulli", "gaussian", "negbin", "binomial")
    assert (simulate.OBS_BERNOULLI, simulate.OBS_GAUSSIAN) == (0, 1)


def test_the_means_are_the_classes_own_formulas_to_the_bit():
    psi = np.random.RandomState(0).standard_normal(64)
    xi, n = 2.5, 7
    np.testing.assert_array_equal(MODELS["bernoulli"].mean(psi, 1.0), logistic(psi))
    np.testing.assert_array_equal(MODELS["negbin"].mean(psi, xi), xi * np.exp(psi))
    np.testing.assert_array_equal(MODELS["gaussian"].mean(psi, 1.0), psi)
    np.testing.assert_array_equal(MODELS["binomial"].mean(psi, float(n)), n * logistic(psi))
    # the parameter the table reads off a regression, and the simulator's
    np.random.seed(0)
    nb, bi, ga = SparseNegativeBinomialRegression(N, B, xi=xi), SparseBinomialRegression(N, B, n=n), SparseGaussianRegression(N, B, eta=0.25)
    assert (MODELS["negbin"].par(nb), MODELS["binomial"].par(bi), MODELS["bernoulli"].par(None), MODELS["gaussian"].par(ga)) == (2.5, 7.0, 1.0, 1.0)
    assert (MODELS["negbin"].sim_par(nb), MODELS["binomial"].sim_par(bi), MODELS["gaussian"].sim_par(ga)) == (2.5, 7.0, 0.5)


@pytest.mark.parametrize("method", ["a_func", "rvs", "mean"])
def test_the_helper_tells_a_built_in_method_from_an_override(method):
    class Empty(SparseBernoulliRegression):
        pass

    class Overrides(SparseBernoulliRegression):
        pass
    setattr(Overrides, method, lambda self, *args, **kw: None)
    np.random.seed(0)
    model = MODELS["bernoulli"]
    for cls in (SparseBernoulliRegression, BernoulliRegression, Empty):
        assert is_builtin(cls(N, B), model, method)
        assert regression.builtin_model(cls(N, B), method) is model
    assert not is_builtin(Overrides(N, B), model, method)
    assert regression.builtin_model(Overrides(N, B), method) is None
    reg = SparseBernoulliRegression(N, B)
    setattr(reg, method, types.MethodType(getattr(SparseBernoulliRegression, method), reg))       # the same function, but set on the instance
    assert method in vars(reg) and not is_builtin(reg, model, method)


def _mixed():
    np.random.seed(0)
    return [SparseBernoulliRegression(N, B), SparseBernoulliRegression(N, B), SparseBinomialRegression(N, B, n=4),
            SparseNegativeBinomialRegression(N, B, xi=2.5)]


def test_a_mixed_list_reads_kind_and_parameter_from_the_table():
    regs = _mixed()
    kind, par = simulate.observation_kinds(regs)
    assert kind.dtype == np.int32 and par.dtype == np.float64
    np.testing.assert_array_equal(kind, [0, 0, 3, 2])
    np.testing.assert_array_equal(par, [0, 0, 4, 2.5])
    ipar = rescale.interval_par(regs)
    assert ipar.dtype == np.float64
    np.testing.assert_array_equal(ipar, [1, 1, 4, 2.5])


def test_a_gaussian_in_the_list_is_refused_where_events_are_needed():
    regs = _mixed()
    regs[1] = SparseGaussianRegression(N, B, eta=0.1)
    kind, par = simulate.observation_kinds(regs)
    np.testing.assert_array_equal(kind, [0, 1, 3, 2])
    np.testing.assert_array_equal(par, [0, np.sqrt(0.1), 4, 2.5])
    with pytest.raises(ValueError, match="time rescaling: neuron 1 is Gaussian"):
        rescale.interval_par(regs)
    model = NonlinearAutoregressiveModel(N, regs, B=B)
    with pytest.raises(ValueError, match=r"simulate\(isi=8\): neuron 1 is Gaussian"):
        model.simulate(10, gpu=False, isi=8)
