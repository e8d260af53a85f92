"""The posterior accumulator on the real engine (pgl_summary_fold / pgl_summary_state / pgl_summary_colsum) against brute force over stacked
samples, against model.log_likelihood() bit for bit, against its own host fallback, over two processes, and once at the headline size.

Tolerances: quantities without a transcendental (state moments) as in tests/test_summary_host.py -- means rtol 1e-12 / atol 1e-12 max|x|,
variances atol 1e-12 max(x^2).  Where the device's exp / log1p meet NumPy's (rates, the log-likelihood term) the values themselves may differ by
rtol 1e-10 (the tolerance tests/test_gpu_model.py uses for means), so: means rtol 1e-10, variances atol 1e-10 max(x^2) (a relative change e of
the values moves their variance by at most 2 e max(x^2)), lppd / p_waic rtol 1e-10."""
import numpy as np
import pytest
from scipy.special import logsumexp

pytestmark = pytest.mark.gpu


def _terms(model, Y, psi, lo=0):
    """the per-cell log-likelihood term from psi (T, n) of neurons lo.., by the regressions' own hooks (eta for Gaussian observations)"""
    from pyglm_amd import regression as R
    out = np.empty_like(psi)
    for j in range(psi.shape[1]):
        r, y, p = model.regressions[lo + j], Y[:, lo + j], psi[:, j]
        if isinstance(r, R.SparseGaussianRegression):
            out[:, j] = -0.5 * np.log(2 * np.pi * r.eta) - (y - p) ** 2 / (2 * r.eta)
        else:
            out[:, j] = np.log(r.c_func(y)) + r.a_func(y) * p - r.b_func(y) * np.log1p(np.exp(p))
    return out


def _close(x, ref, rtol, scale=None):
    ref = np.asarray(ref, dtype=float)
    if scale is None:          # a mean
        np.testing.assert_allclose(x, ref, rtol=rtol, atol=1e-12 * np.max(np.abs(ref)))
    else:                      # a variance of values `scale`
        np.testing.assert_allclose(x, ref, rtol=0, atol=rtol * np.max(np.asarray(scale, dtype=float) ** 2))


def _check_pointwise(acc, ls):
    """ls: per data set, the stacked (S, T_i, N) terms"""
    S = ls[0].shape[0]
    per = sum((logsumexp(l, axis=0) - np.log(S)).sum(axis=0) for l in ls)
    p = sum(l.var(axis=0, ddof=1).sum(axis=0) for l in ls)
    got, w = acc.lppd(), acc.waic()
    np.testing.assert_allclose(got["per_neuron"], per, rtol=1e-10)
    np.testing.assert_allclose(got["total"], per.sum(), rtol=1e-10)
    np.testing.assert_allclose(w["lppd"], per.sum(), rtol=1e-10)
    np.testing.assert_allclose(w["p_waic"], p.sum(), rtol=1e-10)
    np.testing.assert_allclose(w["waic"], -2 * (per.sum() - p.sum()), rtol=1e-10)


def _model(obs, N, B=2, Ts=(300, 200), **kw):
    from pyglm_amd import models as M
    from pyglm_amd import regression as R
    np.random.seed(0)
    rng = np.random.default_rng(3)
    rk = dict(S_w=1.0, mu_b=-1.0)
    if obs == 0:
        model = M.SparseBernoulliGLM(N, B=B, regression_kwargs=rk, seed=1, **kw)
        draw = lambda T: (rng.random((T, N)) < 0.2).astype(float)
    elif obs == 1:
        model = M.SparseNegativeBinomialGLM(N, B=B, regression_kwargs=dict(xi=2.5, **rk), seed=1, **kw)
        draw = lambda T: np.floor(3 * rng.random((T, N)))
    elif obs == 2:
        model = M.SparseGaussianGLM(N, B=B, seed=1, **kw)
        draw = lambda T: rng.standard_normal((T, N))
    elif obs == 3:
        model = M.SparseBinomialGLM(N, B=B, regression_kwargs=dict(n=3, **rk), seed=1, **kw)
        draw = lambda T: np.floor(2.2 * rng.random((T, N)))
    else:
        regs = [(R.SparseBernoulliRegression(N, B, **rk), R.SparseBinomialRegression(N, B, n=4, **rk),
                 R.SparseNegativeBinomialRegression(N, B, xi=2.0, **rk))[n % 3] for n in range(N)]
        model = M.GLM(N, regs, B=B, seed=1, **kw)

        def draw(T):
            Y = np.floor(2 * rng.random((T, N)))
            Y[:, 0::3] = Y[:, 0::3] > 0
            return Y
    Ys = [draw(T) for T in Ts]
    for Y in Ys:
        model.add_data(Y)
    return model, Ys


@pytest.mark.parametrize("N", [70, 6])
@pytest.mark.parametrize("obs", [0, 1, 2, 3, 4])
def test_readouts_against_stacked_samples(obs, N):
    """two data sets in one model, a wide (N >= 64) and a narrow shard; the rates fed from the device's own model.means per sweep, so that
    the comparison isolates the accumulation; collect() equals log_likelihood() bit for bit"""
    model, Ys = _model(obs, N)
    assert model.engine.obs == obs
    acc = model.summarize(rates=True, pointwise=True)
    A, W, b, mus, ls = [], [], [], [[], []], [[], []]
    for it in range(8):
        model.resample_model()
        if it < 2:
            continue
        assert acc.collect() == model.log_likelihood()
        A.append(model.adjacency)
        W.append(model.adjacency[:, :, None] * model.weights)
        b.append(model.biases)
        means = model.means
        st = model._local_state()
        for i, Y in enumerate(Ys):
            mus[i].append(means[i])
            ls[i].append(_terms(model, Y, model.engine.psi(*st, i)))
    assert acc.count == 6 and len(acc.log_likelihoods) == 6
    A, W, b = np.array(A, dtype=float), np.array(W), np.array(b)
    _close(acc.edge_prob, A.mean(0), 1e-12)
    _close(acc.weight_mean, W.mean(0), 1e-12)
    _close(acc.weight_var, W.var(0), 1e-12, scale=W)
    _close(acc.bias_mean, b.mean(0), 1e-12)
    _close(acc.bias_var, b.var(0), 1e-12, scale=b)
    rm, rs = acc.rate_mean, acc.rate_std
    for i in range(2):
        mu = np.array(mus[i])
        assert rm[i].shape == Ys[i].shape
        _close(rm[i], mu.mean(0), 1e-10)
        _close(rs[i] ** 2, mu.var(0), 1e-10, scale=mu)
    _check_pointwise(acc, [np.array(l) for l in ls])


@pytest.mark.parametrize("N", [70, 6])
@pytest.mark.parametrize("obs", [0, 2])
def test_heldout_collect_equals_log_likelihood_and_pointwise(obs, N):
    model, Ys = _model(obs, N, Ts=(300,))
    Y2 = Ys[0][::-1][:250].copy()
    acc = model.summarize(rates=False, pointwise=True, datas=[Y2])
    assert acc._eng.likelihood_only
    ls = []
    for it in range(4):
        model.resample_model()
        assert acc.collect() == model.log_likelihood([Y2])
        eng = model._heldout_engine([Y2])
        ls.append(_terms(model, Y2, eng.psi(*model._local_state(), 0)))
    _check_pointwise(acc, [np.array(ls)])


@pytest.mark.parametrize("obs,N", [(0, 6), (0, 70), (1, 6), (2, 6)])
def test_device_accumulators_against_the_host_fallback(obs, N):
    """the same states through the kernels and through the NumPy formulas that specify them (not bit-equality: hipcc contracts to fma).
    On the observation models the oracle engine knows (it has no binomial log-likelihood)."""
    from tests._oracle_engine import OracleEngine
    dev, Ys = _model(obs, N, Ts=(200,))
    host, _ = _model(obs, N, Ts=(200,), engine_factory=OracleEngine)
    acc_d, acc_h = dev.summarize(rates=True, pointwise=True), host.summarize(rates=True, pointwise=True)
    for it in range(5):
        dev.resample_model()
        A, W, b = dev.adjacency, dev.weights, dev.biases
        for n, (r, rd) in enumerate(zip(host.regressions, dev.regressions)):
            r.a, r.W, r.b = A[n], W[n], b[n:n + 1]
            if obs == 2:
                r.eta = rd.eta
        ll_d, ll_h = acc_d.collect(), acc_h.collect()
        np.testing.assert_allclose(ll_d, ll_h, rtol=1e-10)
    # (the 5 folded values of an entry lie within sqrt(5) standard deviations of their mean: |mean| + 3 sd bounds them)
    bound = lambda mean, var: np.abs(mean) + 3 * np.sqrt(var)
    np.testing.assert_array_equal(acc_d.edge_prob, acc_h.edge_prob)
    _close(acc_d.weight_mean, acc_h.weight_mean, 1e-12)
    _close(acc_d.weight_var, acc_h.weight_var, 1e-12, scale=bound(acc_h.weight_mean, acc_h.weight_var))
    _close(acc_d.bias_mean, acc_h.bias_mean, 1e-12)
    _close(acc_d.rate_mean[0], acc_h.rate_mean[0], 1e-10)
    _close(acc_d.rate_std[0] ** 2, acc_h.rate_std[0] ** 2, 1e-10, scale=bound(acc_h.rate_mean[0], acc_h.rate_std[0] ** 2))
    np.testing.assert_allclose(acc_d.lppd()["per_neuron"], acc_h.lppd()["per_neuron"], rtol=1e-10)
    wd, wh = acc_d.waic(), acc_h.waic()
    np.testing.assert_allclose([wd["lppd"], wd["p_waic"], wd["waic"]], [wh["lppd"], wh["p_waic"], wh["waic"]], rtol=1e-10)


def test_memory_error_before_anything_is_allocated(monkeypatch):
    import torch
    model, Ys = _model(0, 70)
    model.resample_model()
    eng = model.engine
    from pyglm_amd.summary import _DeviceAccumulators
    need = _DeviceAccumulators.bytes(eng, True, True)
    assert need >= 8 * 6 * 500 * 70
    monkeypatch.setattr(type(eng), "_free_bytes", lambda self: need - 1)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(MemoryError, match=r"%d bytes, %d are free" % (need, need - 1)):
        model.summarize(rates=True, pointwise=True)
    assert torch.cuda.memory_allocated() == before
    model.resample_model()
    monkeypatch.setattr(type(eng), "_free_bytes", lambda self: need)
    acc = model.summarize(rates=True, pointwise=True)
    assert acc.collect() == model.log_likelihood()


def test_add_data_after_summarize_invalidates():
    model, Ys = _model(0, 6, Ts=(200,))
    acc = model.summarize()
    acc.collect()
    model.add_data(Ys[0][:100])
    with pytest.raises(RuntimeError, match="after summarize"):
        acc.collect()


@pytest.mark.parametrize("obs,N", [(0, 70), (2, 6)])
def test_the_chain_is_untouched(obs, N):
    runs = []
    for summarise in (False, True):
        model, _ = _model(obs, N)
        acc = model.summarize(rates=True, pointwise=True) if summarise else None
        trace = []
        for _ in range(5):
            model.resample_model()
            trace.append(acc.collect() if summarise else model.log_likelihood())
        runs.append((model.adjacency, model.weights, model.biases, np.array(trace)))
    for x, y in zip(*runs):
        np.testing.assert_array_equal(x, y)


def test_reset_then_the_same_folds_gives_the_same_bits():
    model, _ = _model(0, 6)
    acc = model.summarize(rates=True, pointwise=True)
    read = lambda: [acc.edge_prob, acc.weight_mean, acc.weight_var, acc.bias_var, acc.rate_mean[1], acc.rate_std[0], acc.lppd()["per_neuron"],
                    acc.waic()["per_neuron"], np.array(acc.log_likelihoods)]
    states = []
    for _ in range(3):
        model.resample_model()
        states.append(model.get_state())
        acc.collect()
    first = read()
    acc.reset()
    assert acc.count == 0 and acc.log_likelihoods == []
    with pytest.raises(RuntimeError):
        acc.edge_prob
    for st in states:
        model.set_state(st)
        acc.collect()
    for x, y in zip(first, read()):
        np.testing.assert_array_equal(x, y)


# ---- several ranks
def _rank_worker(rank, world, port, out_path, backend="gloo", force_group=False):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import torch
    import torch.distributed as dist
    from pyglm_amd.models import SparseBernoulliGLM
    from pyglm_amd.utils.basis import cosine_basis
    dev = "cuda:0"
    if backend == "nccl":
        dev = "cuda:%d" % rank
        torch.cuda.set_device(rank)
    if world > 1 or force_group:
        kw = dict(device_id=torch.device(dev)) if backend == "nccl" else {}
        dist.init_process_group(backend, init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world, **kw)
    np.random.seed(0)
    N, B, T = 9, 2, 1200
    basis = cosine_basis(B, L=10) / 10
    Y = (np.random.rand(T, N) < 0.2).astype(float)
    Y2 = (np.random.RandomState(3).rand(300, N) < 0.2).astype(float)
    model = SparseBernoulliGLM(N, basis=basis, regression_kwargs=dict(S_w=5.0, mu_b=-1.0), seed=11, device=dev)
    model.add_data(Y)
    acc = model.summarize(rates=True, pointwise=True)
    held = model.summarize(rates=False, pointwise=True, datas=[Y2])
    lls = []
    for _ in range(4):
        model.resample_model()
        c0 = model.collectives
        lls.append(acc.collect())
        assert model.collectives == c0 + (1 if (world > 1 or force_group) else 0)      # exactly the all-reduce log_likelihood() has
        lls.append(held.collect())
    c0 = model.collectives
    out = dict(lls=np.array(lls), edge_prob=acc.edge_prob, weight_mean=acc.weight_mean, weight_var=acc.weight_var, bias_mean=acc.bias_mean,
               bias_var=acc.bias_var)
    c1 = model.collectives
    out.update(rate_mean=acc.rate_mean[0], rate_std=acc.rate_std[0])
    c2 = model.collectives
    lp, w, hw = acc.lppd(), acc.waic(), held.waic()
    c3 = model.collectives
    out.update(lppd=lp["total"], lppd_n=lp["per_neuron"], waic=np.array([w["lppd"], w["p_waic"], w["waic"]]), waic_n=w["per_neuron"],
               held=np.array([hw["lppd"], hw["p_waic"], hw["waic"]]), held_n=hw["per_neuron"])
    if world > 1 or force_group:
        assert (c1 - c0, c2 - c1, c3 - c2) == (5, 2, 3)        # one gather per per-neuron read-out, one all-reduce per lppd() / waic()
    else:
        assert c3 == c0
    if rank == 0:
        np.savez(out_path, **out)
    if world > 1 or force_group:
        dist.barrier()
        dist.destroy_process_group()


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.timeout(600)
def test_two_processes_sharing_the_gpu_equal_one(tmp_path):
    """two processes (gloo, both on cuda:0) shard the neurons 5 + 4: every read-out, the lppd / WAIC totals included, equals the
    one-process run bit for bit"""
    import torch.multiprocessing as mp
    one, two = str(tmp_path / "one.npz"), str(tmp_path / "two.npz")
    mp.spawn(_rank_worker, args=(1, 0, one), nprocs=1, join=True)
    mp.spawn(_rank_worker, args=(2, _free_port(), two), nprocs=2, join=True)
    a, b = np.load(one), np.load(two)
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.timeout(600)
def test_one_rank_over_rccl_equals_no_process_group(tmp_path):
    import torch.multiprocessing as mp
    one, rccl = str(tmp_path / "one.npz"), str(tmp_path / "rccl.npz")
    mp.spawn(_rank_worker, args=(1, 0, one), nprocs=1, join=True)
    mp.spawn(_rank_worker, args=(1, _free_port(), rccl, "nccl", True), nprocs=1, join=True)
    a, b = np.load(one), np.load(rccl)
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- the headline size, once
@pytest.mark.timeout(900)
def test_full_size_fold_on_a_likelihood_only_engine():
    """N = 1024, B = 5, T = 100 000 on random spikes, rates + pointwise, three folds of perturbed weights; 64 sampled cells against NumPy
    (psi of a sampled cell from its row of the device's design matrix)"""
    import gc
    import torch
    from pyglm_amd.engine import GibbsEngine
    from pyglm_amd.summary import _DeviceAccumulators
    from pyglm_amd.utils.basis import cosine_basis
    N, B, T = 1024, 5, 100000
    rng = np.random.default_rng(0)
    basis = cosine_basis(B, L=100) / 100
    Y = (rng.random((T, N)) < 0.08).astype(np.float64)
    eng = GibbsEngine(N, B, likelihood_only=True)
    eng.add_data(Y, basis=basis)
    s = _DeviceAccumulators(eng, rates=True, pointwise=True)
    ts, ns = rng.integers(0, T, 64), rng.integers(0, N, 64)
    ts[0], ns[0], ts[1], ns[1] = T - 1, N - 1, 0, 0
    Xs = eng.datasets[0].Xt[:N * B, torch.from_numpy(ts).to(eng.dev)].cpu().numpy().T         # (64, D)
    a = rng.random((N, N)) < 0.1
    W0 = 0.2 * rng.standard_normal((N, N, B))
    b = -2.0 + 0.1 * rng.standard_normal(N)
    mu, l = [], []
    for k in range(1, 4):
        W = W0 + 0.05 * rng.standard_normal((N, N, B))
        ll = s.fold(eng, a, W, b, k)
        np.testing.assert_array_equal(ll, eng.log_likelihood(a, W, b))
        aw = (a[:, :, None] * W).reshape(N, N * B)
        psi = np.einsum("cd,cd->c", Xs, aw[ns]) + b[ns]
        mu.append(1.0 / (1.0 + np.exp(-psi)))
        l.append(Y[ts, ns] * psi - np.log1p(np.exp(psi)))
    mu, l = np.array(mu), np.array(l)
    t_dev, n_dev = torch.from_numpy(ts).to(eng.dev), torch.from_numpy(ns).to(eng.dev)
    cell = lambda x: x[t_dev, n_dev].cpu().numpy()
    # psi is a 5120-term fp64 sum formed in another order on the device: |d psi| <= 5120 eps sum|terms|, far inside 1e-9 here
    np.testing.assert_allclose(cell(s.rate[0][0]), mu.mean(0), rtol=1e-9)
    np.testing.assert_allclose(cell(s.rate[0][1]) / 3, mu.var(0), rtol=0, atol=1e-9 * np.max(mu ** 2))
    np.testing.assert_allclose(cell(s.pw[0][0]), l.mean(0), rtol=1e-9)
    np.testing.assert_allclose(cell(s.pw[0][1]) / 2, l.var(0, ddof=1), rtol=0, atol=1e-9 * np.max(l ** 2))
    np.testing.assert_allclose(cell(s.pw[0][2]) + np.log(cell(s.pw[0][3])), logsumexp(l, axis=0), rtol=1e-9)
    st = s.state(3)
    np.testing.assert_array_equal(st["edge_prob"], a.astype(float))
    lp = s.pointwise_sums(3)
    assert lp.shape == (N,) and np.all(np.isfinite(lp)) and np.all(lp < 0)
    del s, eng
    gc.collect()
    torch.cuda.empty_cache()
