"""Every Polya-gamma observation model on the device: the fused binomial mode (obs 3), the hooks mode (obs 4: a, b, log c from the host),
per-neuron xi / n, against the reference's vectors (tests/golden/reference_vectors_binomial.npz) and the oracle."""
import numpy as np
import pytest
from scipy.special import gammaln

from oracle import pyglm_oracle as orc
from tests._pg_agree import assert_pg_agree
from tests.test_oracle_binomial import OracleHooks, binomial_hooks, regression_hooks, golden_binom  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _hyp(regs):
    from pyglm_amd.engine import prior_terms
    rho = np.array([r.rho for r in regs])
    return (rho,) + prior_terms(np.array([r.S_w for r in regs]), np.array([r.mu_w for r in regs]), np.array([r.S_b[0, 0] for r in regs]),
                                np.array([r.mu_b[0] for r in regs]))


def _binom_terms(n, Y):
    Y = np.asarray(Y, dtype=float)
    return Y, np.full(Y.shape, float(n)), gammaln(n + 1) - gammaln(Y + 1) - gammaln(n - Y + 1)


def _engine(N, B, mode, n, lo=0, hi=None, **kw):
    from pyglm_amd.engine import GibbsEngine
    return GibbsEngine(N, B, lo, hi, obs=mode, xi=(n if mode == "binomial" else 1.0), **kw)


def _omega_kappa(eng, i=0):
    ds = eng.datasets[i]
    OK = ds.OK[:ds.T].cpu().numpy()
    return OK[:, :eng.nloc], OK[:, eng.ldn:eng.ldn + eng.nloc]


# ----------------------------------------------------------------------------------------------- 1. golden
@pytest.mark.parametrize("mode", ["binomial", "hooks"])
@pytest.mark.parametrize("tag", ["b0", "b1"])
def test_binomial_regression_golden(torch_dev, golden_binom, tag, mode):
    g = golden_binom
    N, B = g[tag + "_mu_w"].shape
    n = int(g[tag + "_n"])
    X, y = g[tag + "_X"], g[tag + "_y"]
    eng = _engine(N, B, mode, n, 0, 1)
    Y = np.zeros((len(y), N))
    Y[:, 0] = y
    kw = dict(obs_terms=[v[:, :1] for v in _binom_terms(n, Y)]) if mode == "hooks" else {}
    eng.add_data(Y, X=X, **kw)
    a0, W0, b0 = g[tag + "_a0"][None], g[tag + "_W0"][None], g[tag + "_b0"]
    np.testing.assert_allclose(eng.psi(a0, W0, b0)[:, 0], g[tag + "_psi"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(eng.log_likelihood(a0, W0, b0)[0], g[tag + "_ll"].sum(), rtol=1e-11)
    r = OracleHooks(N, B, rho=g[tag + "_rho"], mu_w=g[tag + "_mu_w"], S_w=g[tag + "_S_w"], mu_b=g[tag + "_mu_b"], S_b=g[tag + "_S_b"],
                    **binomial_hooks(n))
    a1, W1, b1, ll = eng.sweep(a0, W0, b0, *_hyp([r]), g[tag + "_perm"][None], g[tag + "_u"][None], g[tag + "_z"][None], seed=1, sweep=0,
                               omega_override=[g[tag + "_om"][:, None]])
    np.testing.assert_allclose(ll[0], g[tag + "_ll"].sum(), rtol=1e-11)
    np.testing.assert_array_equal(a1[0], g[tag + "_a1"])
    np.testing.assert_allclose(W1[0], g[tag + "_W1"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(b1, g[tag + "_b1"], rtol=1e-8, atol=1e-10)
    _, kappa = _omega_kappa(eng)
    np.testing.assert_allclose(kappa[:, 0], g[tag + "_kappa"], rtol=1e-15, atol=0)


@pytest.mark.parametrize("mode", ["binomial", "hooks"])
def test_binomial_model_sweep_golden(torch_dev, golden_binom, mode):
    g = golden_binom
    N, _, B = g["M_W0"].shape
    n = int(g["M_n"])
    eng = _engine(N, B, mode, n, batch=3)
    kw = dict(obs_terms=_binom_terms(n, g["M_Y"])) if mode == "hooks" else {}
    eng.add_data(g["M_Y"], basis=g["M_basis"], **kw)
    np.testing.assert_allclose(eng.design_matrix(), g["M_X"], rtol=1e-10, atol=1e-13)
    regs = [OracleHooks(N, B, S_w=4.0, mu_b=-1.0, **binomial_hooks(n)) for _ in range(N)]
    a1, W1, b1, llb = eng.sweep(g["M_A0"], g["M_W0"], g["M_b0"], *_hyp(regs), g["M_perms"], g["M_us"], g["M_zs"], seed=5, sweep=0,
                                omega_override=[g["M_omegas"].T])
    np.testing.assert_allclose(llb.sum(), g["M_ll0"], rtol=1e-11)
    np.testing.assert_array_equal(a1, g["M_A1"])
    np.testing.assert_allclose(W1, g["M_W1"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(b1, g["M_b1"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(eng.log_likelihood(a1, W1, b1).sum(), g["M_ll1"], rtol=1e-10)


# ----------------------------------------------------------------------------------------------- 2. binomial vs the oracle
def _sweep_problem(Y, N, B, seed=4):
    rng = np.random.default_rng(seed)
    basis = orc.cosine_basis(B, L=15) / 15
    X = orc.convolve_with_basis(Y, basis)
    a = rng.random((N, N)) < 0.3
    W = rng.standard_normal((N, N, B)) * 0.2 * a[:, :, None]
    b = np.full(N, -1.5)
    return X, a, W, b


def _check_vs_oracle(orcs, X, Y, a, W, b, a1, W1, b1, ll, om, perm, u, z, seed, tol=1e-12):
    for k, r in enumerate(orcs):
        r.a, r.W, r.b = a[k].copy(), W[k].copy(), b[k:k + 1].copy()
        np.testing.assert_allclose(ll[k], r.log_likelihood(X, Y[:, k]).sum(), rtol=1e-10)
        want = orc.pg_draw(r.b_func(Y[:, k]), r.activation(X), seed, orc.stream_id(k, 0))
        assert_pg_agree(om[:, k], want, tol=tol)
        r.resample([(X, Y[:, k])], [om[:, k]], perm[k], u[k], z[k])
        np.testing.assert_array_equal(a1[k], r.a)
        np.testing.assert_allclose(W1[k], r.W, rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(b1[k], r.b[0], rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("gram", ["fp64", "int8"])
@pytest.mark.parametrize("n,tol", [(1, 1e-12), (7, 1e-12), (80, 1e-8)])
def test_binomial_sweep_vs_oracle(torch_dev, n, tol, gram):
    """PG(n, psi): n Devroye draws, n = 80 the series branch (1e-8: the series' remainder moments are computed differently on the two sides)"""
    from pyglm_amd.engine import make_draws
    N, B, T = 10, 2, 900
    Y = np.random.default_rng(11).binomial(n, 0.3, size=(T, N)).astype(float)
    X, a, W, b = _sweep_problem(Y, N, B)
    eng = _engine(N, B, "binomial", n, gram=gram)
    eng.add_data(Y, X=X)
    assert eng.datasets[0].int8 == (gram == "int8")
    orcs = [OracleHooks(N, B, rho=0.5, S_w=2.0, mu_w=0.0, mu_b=-1.0, S_b=1.0, **binomial_hooks(n)) for _ in range(N)]
    perm, u, z = make_draws(8, 0, range(N), N, N * B)
    a1, W1, b1, ll = eng.sweep(a, W, b, *_hyp(orcs), perm, u, z, seed=8, sweep=0)
    om, _ = _omega_kappa(eng)
    _check_vs_oracle(orcs, X, Y, a, W, b, a1, W1, b1, ll, om, perm, u, z, 8, tol)


# ----------------------------------------------------------------------------------------------- 3. hooks mode == fused modes, bit for bit
@pytest.mark.parametrize("model", ["bernoulli", "negbin"])
def test_hooks_mode_is_bit_equal_to_the_fused_mode(torch_dev, model):
    from pyglm_amd import regression as R
    from pyglm_amd.engine import GibbsEngine, make_draws
    N, B, T, xi = 12, 3, 700, 2.5
    rng = np.random.default_rng(3)
    Y = (rng.random((T, N)) < 0.2).astype(float) if model == "bernoulli" else rng.negative_binomial(xi, 0.7, size=(T, N)).astype(float)
    X, a, W, b = _sweep_problem(Y, N, B)

    class Restated(R.SparseBernoulliRegression if model == "bernoulli" else R.SparseNegativeBinomialRegression):
        def a_func(self, data):
            return super(Restated, self).a_func(data)

    np.random.seed(0)
    regs = [Restated(N, B) if model == "bernoulli" else Restated(N, B, xi=xi) for _ in range(N)]
    assert R.device_obs(regs)[0] == "hooks"
    orcs = [orc.Regression(N, B, rho=0.5, S_w=2.0, mu_b=-1.0) for _ in range(N)]
    perm, u, z = make_draws(6, 1, range(N), N, N * B)
    out = {}
    for mode in ("hooks", model):
        eng = GibbsEngine(N, B, obs=mode, xi=xi if mode == "negbin" else 1.0)
        eng.add_data(Y, X=X, **(dict(obs_terms=R.obs_terms(regs, Y)) if mode == "hooks" else {}))
        res = eng.sweep(a, W, b, *_hyp(orcs), perm, u, z, seed=6, sweep=1)
        out[mode] = res + _omega_kappa(eng)
        if mode == "hooks":
            assert eng.obs == 4
    h, f = out["hooks"], out[model]
    for k, what in enumerate(["a", "W", "b", "ll", "omega", "kappa"]):
        if what == "ll" and model == "negbin":        # log(exp(gammaln ...)) on the host against lgamma on the device
            np.testing.assert_allclose(h[k], f[k], rtol=1e-12)
            continue
        np.testing.assert_array_equal(h[k], f[k], err_msg=what)


# ----------------------------------------------------------------------------------------------- 4./5. the model API vs the oracle
def _model_vs_oracle(regs, Y, B, tol=1e-12):
    from pyglm_amd import models as M
    from pyglm_amd.engine import make_draws
    N = len(regs)
    basis = orc.cosine_basis(B, L=15) / 15
    model = M.GLM(N, regs, basis=basis, seed=12)
    model.add_data(Y)
    A0, W0, b0 = model.adjacency, model.weights, model.biases
    hyp = [(r.rho.copy(), r.mu_w.copy(), r.S_w.copy(), r.mu_b.copy(), r.S_b.copy()) for r in regs]
    model.resample_model()
    X = model.engine.design_matrix(0)
    om, _ = _omega_kappa(model.engine)
    perm, u, z = make_draws(12, 0, range(N), N, N * B)
    orcs = [OracleHooks(N, B, rho=h[0], mu_w=h[1], S_w=h[2], mu_b=h[3], S_b=h[4], **regression_hooks(r)) for r, h in zip(regs, hyp)]
    _check_vs_oracle(orcs, X, Y, A0, W0, b0, model.adjacency, model.weights, model.biases, model.last_loglik_local, om, perm, u, z, 12, tol)
    return model


def test_user_model_and_heterogeneous_list_through_the_model_api(torch_dev):
    from pyglm_amd import regression as R

    class PlusOne(R.SparseBernoulliRegression):       # b = 1 + y with its own c: a negative binomial with xi = 1 written as hooks
        def b_func(self, data):
            return 1.0 + data

        def c_func(self, data):
            return np.ones_like(data, dtype=float)

    N, B, T = 8, 2, 800
    rng = np.random.default_rng(21)
    np.random.seed(21)
    regs = [PlusOne(N, B, mu_b=-1.0) for _ in range(N)]
    Y = rng.negative_binomial(1.0, 0.7, size=(T, N)).astype(float)
    m = _model_vs_oracle(regs, Y, B)
    assert m.engine_obs() == "hooks" and m.engine.obs == 4
    # Bernoulli, binomial (n = 4) and negative binomial with two xi in one model
    np.random.seed(22)
    regs = ([R.SparseBernoulliRegression(N, B, mu_b=-1.0) for _ in range(3)] + [R.SparseBinomialRegression(N, B, n=4, mu_b=-1.0) for _ in range(2)]
            + [R.SparseNegativeBinomialRegression(N, B, xi=2.0, mu_b=-1.0) for _ in range(2)] + [R.SparseNegativeBinomialRegression(N, B, xi=3.5, mu_b=-1.0)])
    Y = np.column_stack([(rng.random(T) < 0.2)] * 3 + [rng.binomial(4, 0.3, T) for _ in range(2)] + [rng.negative_binomial(2.0, 0.7, T) for _ in range(2)]
                        + [rng.negative_binomial(3.5, 0.7, T)]).astype(float)
    m = _model_vs_oracle(regs, Y, B)
    assert m.engine_obs() == "hooks"
    mus = m.means[0]
    psi = m.engine.psi(m.adjacency, m.weights, m.biases)
    np.testing.assert_allclose(mus[:, 3], 4.0 / (1.0 + np.exp(-psi[:, 3])), rtol=1e-14)
    np.testing.assert_allclose(mus[:, 7], 3.5 * np.exp(psi[:, 7]), rtol=1e-14)


def test_per_neuron_xi_through_the_fused_mode(torch_dev):
    from pyglm_amd import regression as R
    N, B, T = 6, 2, 900
    xis = [1.0, 2.0, 3.0, 2.5, 4.0, 1.0]
    np.random.seed(31)
    regs = [R.SparseNegativeBinomialRegression(N, B, xi=x, mu_b=-1.0) for x in xis]
    rng = np.random.default_rng(31)
    Y = np.column_stack([rng.negative_binomial(x, 0.75, T) for x in xis]).astype(float)
    m = _model_vs_oracle(regs, Y, B)
    assert m.engine.obs == 1 and m.engine.obs_param is not None
    np.testing.assert_array_equal(m.engine.obs_param.cpu().numpy(), xis)


# ----------------------------------------------------------------------------------------------- 6. sharding
def test_hooks_mode_sharded_equals_unsharded(torch_dev):
    from pyglm_amd import regression as R
    from pyglm_amd.engine import GibbsEngine, make_draws
    N, B, T = 11, 2, 600
    rng = np.random.default_rng(5)
    np.random.seed(5)
    regs = [R.SparseBernoulliRegression(N, B) for _ in range(5)] + [R.SparseBinomialRegression(N, B, n=3) for _ in range(6)]
    Y = np.column_stack([rng.random(T) < 0.2 for _ in range(5)] + [rng.binomial(3, 0.2, T) for _ in range(6)]).astype(float)
    X, a, W, b = _sweep_problem(Y, N, B)
    terms = R.obs_terms(regs, Y)
    hyp = _hyp([orc.Regression(N, B, rho=0.4, S_w=3.0, mu_b=-1.0) for _ in range(N)])
    res = {}
    for lo, hi in [(0, N), (0, 5), (5, N)]:
        eng = GibbsEngine(N, B, lo, hi, obs="hooks")
        eng.add_data(Y, X=X, obs_terms=[v[:, lo:hi] for v in terms])
        perm, u, z = make_draws(9, 2, range(lo, hi), N, N * B)
        sl = slice(lo, hi)
        res[(lo, hi)] = eng.sweep(a[sl], W[sl], b[sl], *[h[sl] for h in hyp], perm, u, z, seed=9, sweep=2) + _omega_kappa(eng)
    for k in range(6):
        np.testing.assert_array_equal(np.concatenate([res[(0, 5)][k], res[(5, N)][k]], axis=1 if k >= 4 else 0), res[(0, N)][k])


# ----------------------------------------------------------------------------------------------- 7. stand-alone regressions
def test_standalone_binomial_and_custom_regressions(torch_dev):
    from pyglm_amd import regression as R

    class Twice(R._SparsePGRegressionBase):          # a user's model on the base class (its _obs is None)
        def a_func(self, y):
            return y

        def b_func(self, y):
            return 2.0 * np.ones_like(y, dtype=float)

        def c_func(self, y):
            return np.exp(gammaln(3) - gammaln(y + 1) - gammaln(3 - y))

        def mean(self, X):
            return 2.0 / (1.0 + np.exp(-self.activation(X)))

    N, B, T = 4, 2, 500
    rng = np.random.default_rng(7)
    X = np.abs(rng.standard_normal((T, N, B))) * 0.3
    for reg, y in [(R.SparseBinomialRegression(N, B, n=5), rng.binomial(5, 0.3, T).astype(float)), (Twice(N, B), rng.binomial(2, 0.3, T).astype(float))]:
        for s in range(2):
            reg.resample([(X, y)], seed=3, sweep=s)
        assert np.all(np.isfinite(reg.W)) and np.isfinite(reg.b[0])
        om = reg.omega(X, y, seed=3, sweep=0)
        want = orc.pg_draw(reg.b_func(y), reg.activation(X), 3, orc.stream_id(0, 0))
        assert_pg_agree(om, want)
        psi = reg.activation(X)
        np.testing.assert_allclose(reg.log_likelihood((X, y)), np.log(reg.c_func(y)) + y * psi - reg.b_func(y) * np.log1p(np.exp(psi)), rtol=1e-13)


# ----------------------------------------------------------------------------------------------- 8. held-out data
def test_heldout_binomial_log_likelihood(torch_dev):
    from pyglm_amd import models as M
    N, B, n = 6, 2, 5
    rng = np.random.default_rng(8)
    np.random.seed(8)
    basis = orc.cosine_basis(B, L=15) / 15
    model = M.SparseBinomialGLM(N, basis=basis, regression_kwargs=dict(n=n, mu_b=-1.0), seed=3)
    model.add_data(rng.binomial(n, 0.2, size=(700, N)).astype(float))
    model.resample_model()
    held = rng.binomial(n, 0.2, size=(400, N)).astype(float)
    X = orc.convolve_with_basis(held, basis)
    want = 0.0
    for k in range(N):
        r = OracleHooks(N, B, **binomial_hooks(n))
        r.a, r.W, r.b = model.adjacency[k], model.weights[k], model.biases[k:k + 1]
        want += r.log_likelihood(X, held[:, k]).sum()
    np.testing.assert_allclose(model.log_likelihood(datas=[held]), want, rtol=1e-10)
    with pytest.raises(ValueError):
        model.log_likelihood(datas=[held + n])


# ----------------------------------------------------------------------------------------------- 9. a mode change after the engine is built
def test_mode_change_after_build_raises(torch_dev):
    from pyglm_amd import models as M, regression as R
    N, B = 4, 2
    np.random.seed(9)
    model = M.SparseBinomialGLM(N, B=B, regression_kwargs=dict(n=3), seed=3)
    model.add_data(np.random.default_rng(9).binomial(3, 0.2, size=(300, N)).astype(float))
    model.resample_model()
    model.regressions[2] = R.SparseBernoulliRegression(N, B)
    with pytest.raises(ValueError, match="observation model"):
        model.resample_model()
