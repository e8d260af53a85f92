"""generate()'s choice between the device path and the host loop, and the premise the device path rests on: NumPy's legacy generator gives
the same numbers, and ends in the same state, whether a chunk of bins is drawn in one call or bin by bin.  No GPU needed."""
import inspect
import os
import re

import numpy as np
import pytest

from pyglm_amd import simulate
from pyglm_amd._lib import PglError
from pyglm_amd.models import NonlinearAutoregressiveModel, SparseGaussianGLM
from pyglm_amd.regression import (BernoulliRegression, SparseBernoulliRegression, SparseGaussianRegression,
                                  SparseNegativeBinomialRegression)
from pyglm_amd.utils.basis import cosine_basis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _states_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("N", [1, 4, 7, 1024])
@pytest.mark.parametrize("chunks", [[5], [3, 4], [1, 2, 1, 7]])
def test_chunked_draws_equal_per_bin_draws(N, chunks):
    for one, many in ((np.random.rand, lambda c: np.random.rand(c, N)), (np.random.randn, lambda c: np.random.randn(c, N))):
        np.random.seed(17)
        np.random.randn()                    # an odd count first: a cached second Gaussian is pending
        per_bin = np.array([one(N) for _ in range(sum(chunks))])
        s1 = np.random.get_state()
        np.random.seed(17)
        np.random.randn()
        chunked = np.concatenate([many(c) for c in chunks])
        assert np.array_equal(per_bin, chunked)
        assert _states_equal(np.random.get_state(), s1)


def _model(cls, N=3, B=2, **kw):
    np.random.seed(5)
    return NonlinearAutoregressiveModel(N, [cls(N, B, **kw) for _ in range(N)], basis=cosine_basis(B, L=8) / 8)


class _Inherits(SparseBernoulliRegression):
    pass


class _Overrides(SparseBernoulliRegression):
    def rvs(self, X=None, size=[], psi=None):
        return super(_Overrides, self).rvs(X=X, size=size, psi=psi)


def test_which_observation_models_take_the_device():
    assert _model(SparseBernoulliRegression)._generate_obs(True) == simulate.OBS_BERNOULLI
    assert _model(BernoulliRegression)._generate_obs(True) == simulate.OBS_BERNOULLI
    assert _model(_Inherits)._generate_obs(True) == simulate.OBS_BERNOULLI
    assert _model(SparseGaussianRegression, eta=0.5)._generate_obs(True) == simulate.OBS_GAUSSIAN
    for m in (_model(SparseNegativeBinomialRegression), _model(_Overrides)):
        assert m._generate_obs(None) is None and m._generate_obs(False) is None
        with pytest.raises(ValueError):
            m._generate_obs(True)
    m = _model(SparseBernoulliRegression)
    m.regressions[0].rvs = lambda X=None, size=[], psi=None: np.zeros_like(psi)      # an override on the instance
    assert m._generate_obs(None) is None
    with pytest.raises(ValueError):
        m._generate_obs(True)
    assert _model(SparseBernoulliRegression)._generate_obs(False) is None


def test_an_engine_factory_keeps_the_host_loop():
    m = _model(SparseBernoulliRegression)
    m._engine_factory = lambda *a, **k: None
    assert m._generate_obs(None) is None
    with pytest.raises(ValueError):
        m._generate_obs(True)


@pytest.mark.parametrize("gaussian", [False, True])
def test_without_a_gpu_none_takes_the_host_loop_and_true_raises(monkeypatch, gaussian):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    if gaussian:
        np.random.seed(5)
        m = SparseGaussianGLM(3, basis=cosine_basis(2, L=8) / 8, regression_kwargs=dict(eta=0.5))
    else:
        m = _model(SparseBernoulliRegression)
    out = []
    for gpu in (None, False):
        np.random.seed(6)
        X, Y = m.generate(keep=False, T=200, gpu=gpu)
        out.append((X, Y, np.random.get_state()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and _states_equal(out[0][2], out[1][2])
    with pytest.raises(PglError):
        m.generate(keep=False, T=200, gpu=True)


def test_arguments_are_checked_as_before_on_every_path():
    m = _model(SparseBernoulliRegression)
    for gpu in (None, True, False):
        assert m.generate(T=0, gpu=gpu).shape == (0, 3)
        with pytest.raises(AssertionError):
            m.generate(T=10.0, gpu=gpu)


def test_chunk_sizes():
    assert simulate.chunk_bins(4, 1) == simulate.MAX_CHUNK_BINS
    assert simulate.chunk_bins(1024, 5) == 1638
    assert simulate.chunk_bins(4096, 8) == 64
    assert simulate.chunk_bins(10 ** 5, 8) == 1


def test_the_header_declares_the_simulation_entry():
    text = open(os.path.join(ROOT, "include", "pyglm_hip.h")).read()
    assert re.search(r"\bint pgl_generate\(", text) and re.search(r"\bsize_t pgl_generate_work_bytes\(", text)
    assert "gpu" in inspect.signature(NonlinearAutoregressiveModel.generate).parameters
