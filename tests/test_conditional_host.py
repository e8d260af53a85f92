"""model.conditional_simulate() / model.conditional_check() on the NumPy path (no GPU): the conditional law of pyglm_amd/simulate.py against
simulate_host where the two must coincide, against closed forms where there are some, its replicate, window and history semantics, the
argument errors, and one statistical check that conditioning on the population predicts a coupled neuron better than its mean rate."""
import numpy as np
import pytest

from oracle import pyglm_oracle as orc
from pyglm_amd import regression, simulate
from pyglm_amd.models import NonlinearAutoregressiveModel
from pyglm_amd.regression import (SparseBernoulliRegression, SparseBinomialRegression, SparseGaussianRegression,
                                  SparseNegativeBinomialRegression)
from pyglm_amd.utils.basis import cosine_basis


class PsiEngine(object):
    """NumPy stand-in for GibbsEngine where only psi is needed: X by the oracle's basis convolution (or the caller's), psi = X (a * W)' + b"""

    def __init__(self, N, B, n0=0, n1=None, **kw):
        self.N, self.B, self.n0, self.n1 = N, B, n0, N if n1 is None else n1
        self.datasets = []

    def add_data(self, Y, X=None, basis=None, **kw):
        self.datasets.append(orc.convolve_with_basis(Y, basis) if X is None else np.asarray(X))

    def design_matrix(self, i=0):
        return self.datasets[i]

    def psi(self, a, W, b, i=0):
        X = self.datasets[i]
        return X.reshape(X.shape[0], -1).dot((np.asarray(a)[:, :, None] * np.asarray(W)).reshape(len(b), -1).T) + np.asarray(b).reshape(-1)


_MAKE = {
    "bernoulli": lambda N, B, i: SparseBernoulliRegression(N, B, mu_b=-2.0, S_b=0.1),
    "negbin": lambda N, B, i: SparseNegativeBinomialRegression(N, B, xi=(1.0, 2.5)[i % 2], mu_b=-1.0, S_b=0.1),
    "binomial": lambda N, B, i: SparseBinomialRegression(N, B, n=(1, 10, 64)[i % 3], mu_b=-1.0, S_b=0.1),
    "gaussian": lambda N, B, i: SparseGaussianRegression(N, B, eta=(0.3, 0.05)[i % 2], mu_b=0.0, S_b=0.1),
}


def _model(N, B, L, kinds, seed, basis=None):
    """a model on the stub engine whose neuron i is of kind kinds[i % len(kinds)], at a random sparse state"""
    np.random.seed(seed)
    regs = [_MAKE[kinds[i % len(kinds)]](N, B, i) for i in range(N)]
    model = NonlinearAutoregressiveModel(N, regs, basis=cosine_basis(B, L=L) / L if basis is None else basis, engine_factory=PsiEngine)
    A, W, b = model._adopt_state()
    rng = np.random.default_rng(seed)
    A[...] = rng.random((N, N)) < 0.5
    W[...] = rng.standard_normal(W.shape) * 0.5 / np.sqrt(N)
    W /= np.array([getattr(r, "n", 4.0 if hasattr(r, "xi") else 1.0) for r in regs], dtype=float)[None, :, None]
    base = {"bernoulli": -2.0, "negbin": -0.5, "binomial": -1.0, "gaussian": 0.1}
    b[:, 0] = [base[kinds[i % len(kinds)]] for i in range(N)] + 0.3 * rng.standard_normal(N)
    return model


def _with_recording(model, T, seed):
    Y = model.simulate(T, seed=seed, gpu=False).Y[0]
    model.add_data(Y)
    return Y


def _same(c, d):
    for name in ("Y", "sum", "sumsq", "history"):
        assert np.array_equal(getattr(c, name), getattr(d, name)), name


def test_every_neuron_free_is_simulate_host_bit_for_bit():
    N, T, R = 7, 300, 3
    model = _model(N, 3, 12, ("bernoulli", "negbin", "binomial"), seed=3)
    _with_recording(model, T, seed=90)
    c = model.conditional_simulate(np.arange(N), replicates=R, seed=5, first_replicate=2, gpu=False)
    s = model.simulate(T, replicates=R, seed=5, first_replicate=2, gpu=False)
    assert np.array_equal(c.base, np.broadcast_to(model.biases, (T, N)))
    _same(c, s)
    assert (c.t0, c.t1) == (0, T) and c.Y.shape == (R, T, N) and c.Y.sum() > 0
    np.testing.assert_array_equal(c.rate(), s.rate())
    np.testing.assert_array_equal(c.fano(), s.fano())


def test_without_input_from_the_clamped_neurons_the_recording_does_not_matter():
    N, T = 8, 200
    free = np.array([1, 4, 6])
    model = _model(N, 2, 10, ("bernoulli", "negbin"), seed=4)
    A, _, _ = model._adopt_state()
    clamped = np.setdiff1d(np.arange(N), free)
    A[np.ix_(free, clamped)] = False
    A[np.ix_(free, free)] = True
    Y0, Y1 = _with_recording(model, T, seed=1), _with_recording(model, T, seed=2)
    assert not np.array_equal(Y0, Y1)
    c0 = model.conditional_simulate(free, data=0, replicates=2, seed=6, gpu=False)
    c1 = model.conditional_simulate(free, data=1, replicates=2, seed=6, gpu=False)
    _same(c0, c1)
    assert c0.Y.sum() > 0
    # ... and with input from them it does
    A[np.ix_(free, clamped)] = True
    model._adopt_state()[1][np.ix_(free, clamped)] = -1.5
    assert not np.array_equal(model.conditional_simulate(free, data=0, seed=6, gpu=False).Y, model.conditional_simulate(free, data=1, seed=6, gpu=False).Y)


def _two_neuron_model(w=1.7, bias=-0.8):
    """L = B = 1: neuron 1 is Bernoulli, has no self-coupling and is driven by the previous bin of neuron 0 with weight w"""
    np.random.seed(0)
    model = NonlinearAutoregressiveModel(2, [SparseBernoulliRegression(2, 1) for _ in range(2)], basis=np.ones((1, 1)), engine_factory=PsiEngine)
    A, W, b = model._adopt_state()
    A[...] = [[True, False], [True, False]]
    W[...] = [[[0.3], [0.0]], [[w], [5.0]]]          # (the self-weight is masked by its edge)
    b[:, 0] = [-1.0, bias]
    return model


def test_one_driven_bernoulli_neuron_has_the_closed_form():
    w, bias, T = 1.7, -0.8, 400
    model = _two_neuron_model(w, bias)
    Y = _with_recording(model, T, seed=11)
    cp = model.conditional_check([1], replicates=3, seed=2, gpu=False)
    cp.collect()
    cp.collect()
    prev = np.concatenate(([0.0], Y[:-1, 0]))
    p = 1.0 / (1.0 + np.exp(-(bias + w * prev)))
    assert cp.count == 6 and cp.rate_mean.shape == (T, 1)
    np.testing.assert_allclose(cp.rate_mean[:, 0], p, rtol=0, atol=1e-15)
    np.testing.assert_allclose(cp.rate_std, 0.0, atol=1e-15)
    y = Y[:, 1]
    ll = y * np.log(p) + (1 - y) * np.log1p(-p)
    score = cp.log_score()
    np.testing.assert_allclose(score["per_bin"][:, 0], ll, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(score["total"], ll.sum(), rtol=1e-12)
    np.testing.assert_allclose(score["per_neuron"], [ll.sum()], rtol=1e-12)
    assert 0 < y.sum() < T and 0 < prev.sum()


@pytest.mark.parametrize("kinds", [("bernoulli", "negbin", "binomial"), ("gaussian",)])
def test_one_replicate_one_collect_scores_that_paths_activation(kinds):
    N, T = 6, 150
    free = np.array([0, 2, 5])
    model = _model(N, 2, 8, kinds, seed=8)
    Y = _with_recording(model, T, seed=12)
    cp = model.conditional_check(free, replicates=1, seed=3, gpu=False)
    cp.collect()
    inp = model._conditional_inputs(free, 0, 0, T)
    sim = simulate.conditional_simulate(inp["Wff"], inp["base"], inp["basis"], inp["kind"], inp["par"], free, 1, 3, 0, inp["hist"], 0, True, False,
                                        None, want_psi=True)
    psi = sim.psi[0]
    regs = [model.regressions[n] for n in free]
    if kinds == ("gaussian",):
        eta = np.array([r.eta for r in regs])
        l = -0.5 * np.log(2 * np.pi * eta) - (Y[:, free] - psi) ** 2 / (2 * eta)
        rate = psi
    else:
        A, Bv, logC = regression.obs_terms(regs, Y[:, free])
        l = logC + A * psi - Bv * np.log1p(np.exp(psi))
        rate = np.column_stack([regression.MODELS[regression._kind(r)].mean(psi[:, j], regression.MODELS[regression._kind(r)].par(r))
                                for j, r in enumerate(regs)])
    np.testing.assert_allclose(cp.log_score()["per_bin"], l, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(cp.rate_mean, rate, rtol=1e-12, atol=1e-15)
    # the activation is the law's: base + the free block against the path's own history
    X = orc.convolve_with_basis(sim.Y[0], inp["basis"])
    np.testing.assert_allclose(psi, inp["base"] + X.reshape(T, -1).dot(inp["Wff"].T), rtol=1e-12, atol=1e-13)


def test_replicates_are_independent_of_the_call_and_depend_on_the_seed():
    model = _model(9, 2, 10, ("bernoulli", "negbin", "binomial"), seed=5)
    _with_recording(model, 250, seed=13)
    free = [0, 3, 8]
    c = model.conditional_simulate(free, replicates=5, seed=9, first_replicate=10, gpu=False)
    for r in range(5):
        one = model.conditional_simulate(free, replicates=1, seed=9, first_replicate=10 + r, gpu=False)
        assert np.array_equal(one.Y[0], c.Y[r]) and np.array_equal(one.sum[0], c.sum[r]) and np.array_equal(one.history[0], c.history[r])
    assert len(np.unique(c.sum, axis=0)) == 5
    assert not np.array_equal(model.conditional_simulate(free, replicates=1, seed=10, first_replicate=10, gpu=False).Y[0], c.Y[0])


def test_a_free_neuron_sees_the_uniforms_of_simulate():
    """where the activations coincide -- no coupling at all -- a free neuron's path IS its path in simulate(seed, replicate): the stream is
    keyed by the global neuron index and the bin's index in the recording"""
    model = _model(6, 2, 10, ("bernoulli", "negbin"), seed=6)
    model._adopt_state()[0][...] = False
    Y = _with_recording(model, 200, seed=14)
    c = model.conditional_simulate([1, 4], replicates=2, seed=14, start=50, stop=180, gpu=False)
    s = model.simulate(200, replicates=2, seed=14, gpu=False)
    assert np.array_equal(c.Y, s.Y[:, 50:180][:, :, [1, 4]])
    assert np.array_equal(c.Y[0], Y[50:180][:, [1, 4]])          # (the recording is replicate 0 of that seed)


def test_window_and_history_semantics(monkeypatch):
    N, L, T = 8, 10, 260
    free = np.array([2, 3, 7])
    model = _model(N, 2, L, ("bernoulli", "negbin"), seed=7)
    Y = _with_recording(model, T, seed=15)
    c = model.conditional_simulate(free, replicates=2, seed=4, start=37, stop=201, gpu=False)
    assert (c.t0, c.t1, c.T) == (37, 201, 164) and c.Y.shape == (2, 164, 3) and c.base.shape == (164, 3)
    # the inputs are rows start:stop of the whole recording's and the recording's own rows before start, nothing else
    inp = model._conditional_inputs(free, 0, 37, 201)
    whole = model._conditional_inputs(free, 0, 0, T)
    assert np.array_equal(inp["base"], whole["base"][37:201]) and np.array_equal(inp["hist"], Y[37 - L:37][:, free])
    assert np.array_equal(c.base, inp["base"])
    # a window that starts within the first L bins has silence in front of the recording
    early = model._conditional_inputs(free, 0, 4, 50)["hist"]
    assert np.array_equal(early[:L - 4], np.zeros((L - 4, 3))) and np.array_equal(early[L - 4:], Y[:4][:, free])
    # the history returned is the last L bins of every path; a longer window continues a shorter one bin for bin
    assert np.array_equal(c.history, c.Y[:, -L:])
    short = model.conditional_simulate(free, replicates=2, seed=4, start=37, stop=120, gpu=False)
    assert np.array_equal(short.Y, c.Y[:, :83])
    # paths(r): the recording in every clamped column
    p = c.paths(1)
    clamped = np.setdiff1d(np.arange(N), free)
    assert p.shape == (164, N) and np.array_equal(p[:, clamped], Y[37:201][:, clamped]) and np.array_equal(p[:, free], c.Y[1])
    # without the paths: the same sums and history, also when the rolling buffer is shorter than the window
    monkeypatch.setattr(simulate, "HOST_BLOCK_BINS", 23)
    bare = model.conditional_simulate(free, replicates=2, seed=4, start=37, stop=201, keep_paths=False, gpu=False)
    assert bare.Y is None
    for name in ("sum", "sumsq", "history"):
        assert np.array_equal(getattr(bare, name), getattr(c, name)), name
    assert np.array_equal(c.sum, c.Y.sum(axis=1))
    with pytest.raises(ValueError, match="not kept"):
        bare.paths(0)
    empty = model.conditional_simulate(free, start=40, stop=40, gpu=False)
    assert empty.Y.shape == (1, 0, 3) and np.array_equal(empty.history[0], Y[30:40][:, free])


def test_the_check_folds_block_by_block_as_in_one_piece(monkeypatch):
    model = _model(6, 2, 8, ("bernoulli", "negbin"), seed=9)
    _with_recording(model, 120, seed=16)
    outs = []
    for block in (4096, 17):
        monkeypatch.setattr(simulate, "HOST_BLOCK_BINS", block)
        cp = model.conditional_check([1, 2], replicates=3, seed=5, start=10, gpu=False)
        cp.collect()
        cp.collect()
        outs.append((cp.rate_mean, cp.rate_std, cp.log_score()["per_bin"]))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert outs[0][0].shape == (110, 2) and outs[0][1].max() > 0


def test_a_callers_own_regressors_feed_the_clamped_part():
    model = _model(5, 2, 8, ("bernoulli",), seed=10)
    Y = model.simulate(100, seed=17, gpu=False).Y[0]
    X = np.random.default_rng(0).standard_normal((100, 5, 2))
    model.add_data(Y, X=X)
    free = np.array([1, 3])
    A, W, b = model._adopt_state()
    Wm = (A[:, :, None] * W)
    clamped = [0, 2, 4]
    want = b[free, 0] + np.einsum("tmb,jmb->tj", X[:, clamped], Wm[free][:, clamped])
    np.testing.assert_allclose(model.conditional_simulate(free, gpu=False).base, want, rtol=1e-12, atol=1e-13)


def test_argument_errors_name_the_offender():
    model = _model(300, 1, 4, ("bernoulli",), seed=1)
    model.add_data(np.zeros((20, 300)))
    for call in (model.conditional_simulate, model.conditional_check):
        with pytest.raises(ValueError, match="empty"):
            call([], gpu=False)
        with pytest.raises(ValueError, match="257 free neurons"):
            call(np.arange(257), gpu=False)
        with pytest.raises(ValueError, match="neuron 5 is listed more than once"):
            call([3, 5, 9, 5], gpu=False)
        with pytest.raises(ValueError, match="index 300 is outside"):
            call([0, 300], gpu=False)
        with pytest.raises(ValueError, match="index -1 is outside"):
            call([-1, 2], gpu=False)
        with pytest.raises(ValueError, match=r"window \[5, 21\)"):
            call([0], start=5, stop=21, gpu=False)
        with pytest.raises(ValueError, match=r"window \[7, 3\)"):
            call([0], start=7, stop=3, gpu=False)
        with pytest.raises(ValueError, match="engine_factory"):
            call([0], gpu=True)
    assert model.conditional_simulate(np.arange(256), gpu=False).Y.shape == (1, 20, 256)
    assert list(model.conditional_simulate([9, 2, 4], gpu=False).free) == [2, 4, 9]


def test_an_exploding_free_neuron_names_the_global_index():
    model = _model(6, 1, 4, ("negbin",), seed=2)
    _with_recording(model, 30, seed=18)
    _, _, b = model._adopt_state()
    keep = b[4, 0]
    b[4, 0] = 40.0
    with pytest.raises(simulate.PglError, match=r"neuron 4 in replicate 6 at bin 3 "):
        model.conditional_simulate([1, 4], replicates=2, first_replicate=6, seed=1, start=3, gpu=False)
    b[4, 0] = keep
    assert model.conditional_simulate([1, 4], replicates=2, first_replicate=6, seed=1, start=3, gpu=False).Y.shape == (2, 27, 2)


# ---- a sharded model: base is gathered as `means` gathers, then every rank simulates the same thing
def _sharded(rank, world, port, out):
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    model = _model(5, 2, 8, ("bernoulli", "negbin"), seed=12)
    assert (model.n1 - model.n0 < 5) == (world > 1)
    _with_recording(model, 120, seed=3)
    c = model.conditional_simulate([1, 3], replicates=2, seed=4, start=9, gpu=False)
    np.savez(out % rank, Y=c.Y, base=c.base, history=c.history, sum=c.sum)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_simulate_what_one_does(tmp_path):
    import socket
    import torch.multiprocessing as mp
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    _sharded(0, 1, 0, str(tmp_path / "one%d.npz"))
    mp.spawn(_sharded, args=(2, port, str(tmp_path / "two%d.npz")), nprocs=2, join=True)
    one = np.load(str(tmp_path / "one0.npz"))
    for rank in range(2):
        two = np.load(str(tmp_path / ("two%d.npz" % rank)))
        np.testing.assert_allclose(two["base"], one["base"], rtol=1e-12, atol=1e-13)
        for k in ("Y", "history", "sum"):
            assert np.array_equal(two[k], one[k]), (rank, k)
    assert one["Y"].shape == (2, 111, 2) and one["Y"].sum() > 0


# ---- statistical sense
STAT_SEED = 1          # of the state's noise and of the recording (tried 1 first: it meets the check)


def test_conditioning_on_the_population_beats_the_mean_rate():
    """the recording is simulated from the model itself; neuron 0 has strong inputs from the five clamped neurons: its conditional log score is
    strictly above the score of the constant predictor at its recorded mean rate"""
    N, B, L, T = 6, 2, 10, 3000
    np.random.seed(STAT_SEED)
    model = NonlinearAutoregressiveModel(N, [SparseBernoulliRegression(N, B) for _ in range(N)], basis=cosine_basis(B, L=L), engine_factory=PsiEngine)
    A, W, b = model._adopt_state()
    rng = np.random.default_rng(STAT_SEED)
    A[...] = False
    A[0, 1:] = True
    W[0, 1:] = np.array([2.5, -2.5, 2.0, -2.0, 3.0])[:, None] * (1.0 + 0.1 * rng.standard_normal((5, B)))
    b[:, 0] = [-1.5, -1.0, -1.0, -1.2, -0.8, -1.0]
    Y = _with_recording(model, T, seed=STAT_SEED)
    cp = model.conditional_check([0], replicates=4, seed=STAT_SEED + 1, gpu=False)
    cp.collect()
    y = Y[:, 0]
    pbar = y.mean()
    assert 0.02 < pbar < 0.98
    constant = (y * np.log(pbar) + (1 - y) * np.log1p(-pbar)).sum()
    score = cp.log_score()["total"]
    print("conditional log score %.1f, constant predictor %.1f" % (score, constant))
    assert score > constant
