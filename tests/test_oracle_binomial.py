"""The oracle's observation hooks (a_func / b_func / log_c_func of oracle.pyglm_oracle.Regression) pinned for a binomial model against
vectors captured from the reference's own _SparsePGRegressionBase (tests/golden/make_binomial_fixture.py).  CPU only."""
import os

import numpy as np
import pytest
from scipy.special import gammaln

from oracle import pyglm_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class OracleHooks(orc.Regression):
    """an oracle regression whose observation model is given by three functions of y (the hooks of regression.py:479-489)"""

    def __init__(self, N, B, a, b, log_c, **kw):
        super(OracleHooks, self).__init__(N, B, **kw)
        self._a, self._b, self._log_c = a, b, log_c

    def a_func(self, y):
        return self._a(y)

    def b_func(self, y):
        return self._b(y)

    def log_c_func(self, y):
        return self._log_c(y)


def binomial_hooks(n):
    return dict(a=lambda y: y, b=lambda y: n * np.ones_like(y, dtype=float),
                log_c=lambda y: gammaln(n + 1) - gammaln(y + 1) - gammaln(n - y + 1))


def regression_hooks(reg):
    """the oracle hooks of a package regression: its own a_func, b_func and log(c_func)"""
    return dict(a=lambda y: np.broadcast_to(np.asarray(reg.a_func(y), dtype=float), y.shape),
                b=lambda y: np.broadcast_to(np.asarray(reg.b_func(y), dtype=float), y.shape),
                log_c=lambda y: np.broadcast_to(np.log(np.asarray(reg.c_func(y), dtype=float)), y.shape))


@pytest.fixture(scope="session")
def golden_binom():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_vectors_binomial.npz"))


def make_oracle(g, tag):
    N, B = g[tag + "_mu_w"].shape
    r = OracleHooks(N, B, rho=g[tag + "_rho"], mu_w=g[tag + "_mu_w"], S_w=g[tag + "_S_w"], mu_b=g[tag + "_mu_b"], S_b=g[tag + "_S_b"],
                    **binomial_hooks(int(g[tag + "_n"])))
    r.a, r.W, r.b = g[tag + "_a0"].copy(), g[tag + "_W0"].copy(), g[tag + "_b0"].copy()
    return r


@pytest.mark.parametrize("tag", ["b0", "b1"])
def test_oracle_binomial_statistics(golden_binom, tag):
    g = golden_binom
    r = make_oracle(g, tag)
    X, y = g[tag + "_X"], g[tag + "_y"]
    np.testing.assert_allclose(r.activation(X), g[tag + "_psi"], rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(r.b_func(y), g[tag + "_pg_b"])                  # the b the reference hands to pgdrawvpar
    np.testing.assert_allclose(r.kappa(y), g[tag + "_kappa"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r.log_likelihood(X, y), g[tag + "_ll"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("tag", ["b0", "b1"])
def test_oracle_binomial_resample(golden_binom, tag):
    g = golden_binom
    r = make_oracle(g, tag)
    X, y = g[tag + "_X"], g[tag + "_y"]
    r.resample([(X, y)], [g[tag + "_om"]], g[tag + "_perm"], g[tag + "_u"], g[tag + "_z"])
    np.testing.assert_array_equal(r.a, g[tag + "_a1"])
    np.testing.assert_allclose(r.W, g[tag + "_W1"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(r.b, g[tag + "_b1"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(r.log_likelihood(X, y).sum(), g[tag + "_ll1"], rtol=1e-10)


def test_oracle_binomial_model_sweep(golden_binom):
    g = golden_binom
    N, _, B = g["M_W0"].shape
    n = int(g["M_n"])
    X, Y = g["M_X"], g["M_Y"]
    np.testing.assert_allclose(orc.convolve_with_basis(Y, g["M_basis"]), X, rtol=1e-10, atol=1e-13)
    regs = [OracleHooks(N, B, S_w=4.0, mu_b=-1.0, **binomial_hooks(n)) for _ in range(N)]
    for k, r in enumerate(regs):
        r.a, r.W, r.b = g["M_A0"][k].copy(), g["M_W0"][k].copy(), g["M_b0"][k:k + 1].copy()
    np.testing.assert_allclose(sum(r.log_likelihood(X, Y[:, k]).sum() for k, r in enumerate(regs)), g["M_ll0"], rtol=1e-11)
    for k, r in enumerate(regs):
        r.resample([(X, Y[:, k])], [g["M_omegas"][k]], g["M_perms"][k], g["M_us"][k], g["M_zs"][k])
    np.testing.assert_array_equal(np.array([r.a for r in regs]), g["M_A1"])
    np.testing.assert_allclose(np.array([r.W for r in regs]), g["M_W1"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(np.array([r.b[0] for r in regs]), g["M_b1"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(sum(r.log_likelihood(X, Y[:, k]).sum() for k, r in enumerate(regs)), g["M_ll1"], rtol=1e-10)
