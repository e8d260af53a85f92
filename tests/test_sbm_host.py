"""The block-model law in NumPy (pyglm_amd/sbm.py) against brute force, the learned networks, and a model chain on the CPU test engine."""
import copy

import numpy as np
import pytest

from pyglm_amd import networks as NW
from pyglm_amd import sbm
from tests import _sbm_cases as C


def brute_log_joint(A, z, P, pi):
    """log p(A off the diagonal, z | P, pi)"""
    N = len(z)
    total = np.log(pi[z]).sum()
    for n in range(N):
        for m in range(N):
            if n != m:
                p = P[z[n], z[m]]
                total += np.log(p) if A[n, m] else np.log1p(-p)
    return total


def test_scan_lp_is_the_conditional_of_the_joint():
    N, K = 7, 3
    rng = np.random.default_rng(0)
    A = rng.random((N, N)) < 0.4
    P, pi = rng.uniform(0.05, 0.95, size=(K, K)), rng.dirichlet(np.ones(K))
    z0 = rng.integers(0, K, size=N)
    u = rng.random(N)
    t = sbm.tables(P, pi)
    z1, lp = sbm.sbm_scan_host(A, z0, *t, u, return_lp=True)
    z = z0.copy()
    for n in range(N):
        joint = np.empty(K)
        for k in range(K):
            z[n] = k
            joint[k] = brute_log_joint(A, z, P, pi)
        assert np.max(np.abs((lp[n] - lp[n, 0]) - (joint - joint[0]))) <= 1e-9
        # the draw: the categorical of the normalised lp, by inversion
        p = np.exp(joint - joint.max())
        c = np.cumsum(p / p.sum())
        assert z1[n] == min(int(np.searchsorted(c, u[n], side="right")), K - 1) == sbm.decide(lp[n], u[n])
        z[n] = z1[n]
    assert np.array_equal(z, z1)
    # the replay along the path taken is the same arithmetic
    assert np.array_equal(sbm.replay_lp(A, z0, z1, t), lp)


@pytest.mark.parametrize("N, K", [(1, 1), (9, 1), (9, 4), (40, 32)])
def test_block_counts_against_einsum(N, K):
    rng = np.random.default_rng(N + K)
    A = rng.random((N, N)) < 0.3
    z = rng.integers(0, K, size=N)
    Z = np.eye(K, dtype=np.int64)[z]
    off = A.astype(np.int64) * (1 - np.eye(N, dtype=np.int64))
    M, nk, d = sbm.block_counts_host(A, z, K)
    assert M.dtype == nk.dtype == np.int64
    assert np.array_equal(M, np.einsum("nk,nm,ml->kl", Z, off, Z)) and np.array_equal(nk, Z.sum(axis=0)) and d == np.trace(A.astype(int))
    assert M.sum() + d == A.sum()


def _fixed_adjacency():
    N = 12
    rng = np.random.default_rng(5)
    A = np.zeros((N, N), dtype=bool)
    off = np.flatnonzero(~np.eye(N, dtype=bool).ravel())
    A.ravel()[rng.choice(off, size=40, replace=False)] = True
    A[np.arange(5), np.arange(5)] = True
    assert A.sum() == 45 and np.trace(A) == 5
    return A


@pytest.mark.parametrize("special", [True, False])
def test_K1_is_beta_bernoulli(special):
    """the mean of 4000 conjugate draws on a fixed A against the Beta posterior's, within 4 standard errors"""
    A, a_0, b_0, draws = _fixed_adjacency(), 2.0, 3.0, 4000
    N = A.shape[0]
    np.random.seed(11)
    net = NW._IndependentBernoulliMixin(N, 1, a_0=a_0, b_0=b_0, is_diagonal_conn_special=special)
    assert net.K == 1 and net.rho.shape == (N, N)
    W = np.zeros((N, N, 1))
    p, ps = np.empty(draws), np.empty(draws)
    for i in range(draws):
        net.resample((A, W))
        rho = net.rho
        assert np.all(rho[~np.eye(N, dtype=bool)] == net.p) and np.all(np.diag(rho) == net.rho_diag) and np.all(net.z == 0)
        p[i], ps[i] = net.p, net.rho_diag

    def check(x, a, b):
        mean, var = a / (a + b), a * b / ((a + b) ** 2 * (a + b + 1))
        print("mean %.5f  posterior mean %.5f  se %.5f" % (x.mean(), mean, np.sqrt(var / draws)))
        assert abs(x.mean() - mean) <= 4 * np.sqrt(var / draws)
    if special:
        assert (a_0 + 40) / (a_0 + b_0 + 132) == (a_0 + 40) / (a_0 + 40 + b_0 + 92)
        check(p, a_0 + 40, b_0 + 132 - 40)
        check(ps, a_0 + 5, b_0 + 12 - 5)
    else:
        check(p, a_0 + 45, b_0 + 144 - 45)            # the pooled count
        assert np.array_equal(p, ps)


def test_sbm_host_with_K1_draws_what_the_mixin_draws():
    A = _fixed_adjacency()
    out = sbm.sbm_host(A, np.zeros(12, dtype=int), 1, np.random.RandomState(3), a_0=2.0, b_0=3.0, a_self=2.0, b_self=3.0)
    rs = np.random.RandomState(3)
    assert out["P"][0, 0] == rs.beta(2.0 + 40, 3.0 + 92) and out["rho_self"] == rs.beta(2.0 + 5, 3.0 + 7) and out["pi"][0] == 1.0
    assert np.array_equal(out["z"], np.zeros(12)) and out["M"][0, 0] == 40 and out["n"][0] == 12 and out["d"] == 5
    pinned = sbm.sbm_host(A, np.zeros(12, dtype=int), 1, np.random.RandomState(3), rho_self=0.25)
    assert pinned["rho_self"] == 0.25


def test_clamps_keep_every_logarithm_finite():
    P = np.array([[0.0, 1.0, 1e-320], [1.0, 0.0, 0.5], [1e-320, 1e-320, 1.0]])
    LP, LQ, logpi = sbm.tables(P, np.array([0.0, 1e-320, 1.0]))
    assert all(np.isfinite(v).all() for v in (LP, LQ, logpi))
    assert LP.min() == np.log(2.0 ** -1000) and LQ.min() == np.log(2.0 ** -53) and logpi.min() == np.log(2.0 ** -1000)
    N = 30
    rng = np.random.default_rng(2)
    A = rng.random((N, N)) < 0.3
    z, lp = sbm.sbm_scan_host(A, rng.integers(0, 3, size=N), LP, LQ, logpi, rng.random(N), return_lp=True)
    assert np.isfinite(lp).all() and z.min() >= 0 and z.max() < 3
    for bad in (0, 33, 2.5):
        with pytest.raises(ValueError, match="K ="):
            sbm.check_blocks(bad)
    with pytest.raises(ValueError, match="label"):
        sbm.sbm_scan_host(A, np.full(N, 3), LP, LQ, logpi, rng.random(N))


@pytest.mark.parametrize("N", [65, 1025, 2500])
@pytest.mark.parametrize("K", [2, 3, 32])
def test_no_draw_of_the_scan_cases_hangs_on_the_last_bit_of_exp(N, K):
    """the device tests excuse a draw that a one-ulp difference in exp could turn; on the inputs they use the host rule meets none: the
    decisions under NumPy's exp and under a long-double exp rounded once agree, and no draw lies within the excuse's margin"""
    A = C.adjacency(N)
    for clamps in (False, True):
        z0, t, u = C.scan_case(N, K, clamps)
        z1, lp = sbm.sbm_scan_host(A, z0, *t, u, return_lp=True)
        assert np.array_equal(sbm.replay_lp(A, z0, z1, t), lp)
        labels, turnable = C.host_decisions(lp, u)
        labels_ld, _ = C.host_decisions(lp, u, exp=C.exp_long_double)
        assert np.array_equal(labels, z1) and np.array_equal(labels_ld, z1) and not turnable.any()


def test_adjusted_rand_and_components():
    a = np.array([0, 0, 1, 1, 2, 2])
    assert sbm.adjusted_rand(a, a) == 1.0 and sbm.adjusted_rand(a, np.array([5, 5, 3, 3, 9, 9])) == 1.0
    assert abs(sbm.adjusted_rand(a, np.array([0, 0, 1, 2, 2, 2])) - 0.4444444444444444) < 1e-12       # by hand: (2 - 0.8) / (3.5 - 0.8)
    assert sbm.adjusted_rand(np.zeros(4), np.zeros(4)) == 1.0
    adj = np.zeros((5, 5), dtype=bool)
    adj[0, 3] = adj[3, 0] = adj[1, 4] = True
    assert sbm.connected_components(adj).tolist() == [0, 1, 2, 0, 1]


RECOVERY_SEED = 0        # a seed at which the uncollapsed sampler leaves its starting point for the planted partition (most do; some stay in a merged mode)


def _planted(N=60, blocks=3, p_in=0.6, p_out=0.05, seed=RECOVERY_SEED):
    rng = np.random.default_rng(seed)
    truth = np.repeat(np.arange(blocks), N // blocks)
    A = rng.random((N, N)) < np.where(truth[:, None] == truth[None, :], p_in, p_out)
    return A, truth, rng


def test_recovery_of_a_planted_partition():
    A, truth, rng = _planted()
    N, K = len(truth), 6
    z = rng.integers(0, K, size=N)
    rs = np.random.RandomState(RECOVERY_SEED)
    fold = sbm._HostFold(N, K)
    for it in range(60):
        out = sbm.sbm_host(A, z, K, rs, seed=RECOVERY_SEED, sweep=it)
        z = out["z"]
        if it >= 30:
            fold.fold(z, out["P"], out["rho_self"])
    coassign = fold.read()[0] / 30.0
    same = (truth[:, None] == truth[None, :]).astype(float)
    consensus = sbm.connected_components(coassign > 0.5)
    ari, err = sbm.adjusted_rand(consensus, truth), np.abs(coassign - same).mean()
    print("adjusted Rand %.4f  mean |coassign - truth| %.4f" % (ari, err))
    assert ari >= 0.95 and err <= 0.02


# ---- the networks and a model chain on the CPU test engine -----------------------------------------------------------------------------------
def _model(network, N=8, B=2, T=300, seed=1):
    from pyglm_amd import models as M
    from tests._oracle_engine import OracleEngine
    model = M.SparseBernoulliGLM(N, B=B, network=network, regression_kwargs=dict(S_w=3.0, mu_b=-1.0), engine_factory=OracleEngine, seed=seed)
    model.add_data((np.random.default_rng(3).random((T, N)) < 0.2).astype(float))
    return model


def _sbm_network(N=8, B=2, **kw):
    np.random.seed(4)
    return NW.SBMSparseNetwork(N, B, K=3, **kw)


def test_model_chain_pushes_the_block_prior_and_replays():
    N = 8
    model = _model(_sbm_network())
    assert model._network_device() is None
    blocks = model.block_structure()
    assert not blocks.on_device
    for _ in range(3):
        model.resample_model()
        blocks.collect()
    net = model.network
    want = net.P[net.z][:, net.z]
    want[np.diag_indices(N)] = net.rho_self
    for n, reg in enumerate(model.regressions):
        assert np.array_equal(np.asarray(reg.rho), want[n])
    assert np.array_equal(net.rho, want) and net.block_sizes.sum() == N and net.pi.shape == (3,) and 0 < net.rho_self < 1
    assert blocks.count == 3 and len(blocks.occupied) == 3 and np.all(np.diag(blocks.coassign) == 1.0)
    assert np.array_equal(blocks.coassign, blocks.coassign.T) and blocks.consensus().shape == (N,)
    # set_state(get_state()) replays the chain exactly, the network's z, P and pi with it
    state = model.get_state()
    assert all(np.array_equal(getattr(state["network"], k), getattr(net, k)) for k in ("z", "P", "pi"))

    def two_more():
        for _ in range(2):
            model.resample_model()
        nw = model.network
        return [model.adjacency, model.weights, model.biases, nw.z.copy(), nw.P.copy(), nw.pi.copy(), np.float64(nw.rho_self)]
    first = two_more()
    model.set_state(state)
    assert np.array_equal(model.network.z, state["network"].z)
    second = two_more()
    assert all(np.array_equal(u, v) for u, v in zip(first, second))
    with pytest.raises(TypeError, match="learns no partition"):
        _model(NW.NIWSparseNetwork(N, 2)).block_structure()


@pytest.mark.parametrize("cls, kw", [(NW.SBMSparseNetwork, dict(K=3)), (NW.BetaBernoulliSparseNetwork, dict(a_0=2.0))])
def test_weight_draws_are_those_of_the_NIW_network(cls, kw):
    """fed the same (A, W) from the same generator, the learned networks leave the NIW parameters a NIWSparseNetwork draws: the adjacency
    update comes after the weights' draws and takes nothing from before them"""
    N, B = 8, 2
    rng = np.random.default_rng(8)
    np.random.seed(2)
    nets = [cls(N, B, **kw), NW.NIWSparseNetwork(N, B, rho=0.5)]
    for it in range(3):
        A = rng.random((N, N)) < 0.5
        W = rng.standard_normal((N, N, B))
        for net in nets:
            net._set_rng(np.random.RandomState(100 + it))
            if hasattr(net, "_set_scan"):
                net._set_scan(9, it, None)
            net.resample((A, W))
            net._set_rng(None)
        for u, v in zip(nets[0].weight_blocks(), nets[1].weight_blocks()):
            assert np.array_equal(u, v)
    assert nets[0]._rng is None and nets[0]._gaussian.rng is None


def test_networks_keywords_and_the_existing_four():
    import warnings
    N, B = 5, 2
    np.random.seed(0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        net = NW.SBMSparseNetwork(N, B, K=4, alpha=2.0, rho_self=0.3, z=[0, 1, 2, 3, 0], nu_0=9.0)
    assert len(w) == 1 and "nu_0" in str(w[0].message)                   # the weight keyword is dropped as for NIWSparseNetwork ...
    assert (net.K, net.alpha, net.rho_self) == (4, 2.0, 0.3) and net.z.tolist() == [0, 1, 2, 3, 0]      # ... the adjacency keywords arrive
    assert net.rho.shape == (N, N) and np.all(np.diag(net.rho) == 0.3) and net.rho[0, 4] == net.P[0, 0]
    bb = NW.BetaBernoulliSparseNetwork(N, B, a_0=3.0, is_diagonal_conn_special=False)
    assert bb.a_0 == 3.0 and bb.K == 1 and not bb.is_diagonal_conn_special and np.all(bb.rho == bb.p)
    cp = copy.deepcopy(net)
    assert cp is not net and np.array_equal(cp.z, net.z) and cp.z is not net.z and cp._driver is None
    # called outside a model: u from NumPy's global generator, the scan on the host
    A, W = np.random.random((N, N)) < 0.5, np.zeros((N, N, B))
    np.random.seed(1)
    net.resample((A, W))
    z1 = net.z.copy()
    np.random.seed(1)
    net2 = copy.deepcopy(cp)
    net2.resample((A, W))
    assert np.array_equal(z1, net2.z) and net.rho_self == 0.3
    # the existing four are what they were
    assert [c.__mro__[1:3] for c in (NW.FixedMeanDenseNetwork, NW.FixedMeanSparseNetwork, NW.NIWDenseNetwork, NW.NIWSparseNetwork)] == [
        (NW._DenseAdjacencyMixin, NW._FixedWeightsMixin), (NW._FixedAdjacencyMixin, NW._FixedWeightsMixin),
        (NW._DenseAdjacencyMixin, NW._IndependentGaussianMixin), (NW._FixedAdjacencyMixin, NW._IndependentGaussianMixin)]
    old = NW.NIWSparseNetwork(N, B, rho=0.25, rho_self=0.75)
    assert np.all(np.diag(old.rho) == 0.75) and old.rho[0, 1] == 0.25 and not hasattr(old, "_set_scan")
