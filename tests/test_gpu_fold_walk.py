"""The walk over the data sets that every read-out of the chain shares (GibbsEngine.fold_data), seen from outside: which library entries one
fold of each read-out reaches, in which order and with which accumulate / elem0 / T, and under which stage names the engine times them.

The shape is the smallest that takes every branch of the walk: N = 4, B = 2, the shard n0 = 1, n1 = 4 (nloc = 3, neuron0 != 0), two data
sets of T = 70 and T = 33 bins (neither a multiple of 64), negative-binomial observations with one xi per neuron (what the dispersion fold asks
for).  What the folds compute is held to the NumPy definitions by the tests of each read-out; here only one identity is checked on the way,
the summary fold's return value against log_likelihood(), bit for bit, as its docstring promises."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, B, N0, N1, TS = 4, 2, 1, 4, (70, 33)
NLOC = N1 - N0


def test_one_fold_of_every_read_out_reaches_the_entries_its_docstring_promises(monkeypatch):
    from oracle import pyglm_oracle as orc
    from pyglm_amd import _lib, diagnostics, dispersion, engine, rescale, summary
    rng = np.random.default_rng(11)
    basis = orc.cosine_basis(B, L=20) / 20
    eng = engine.GibbsEngine(N, B, N0, N1, device="cuda:0", obs="negbin", xi=np.array([2.0, 1.5, 3.0, 2.5]))
    for T in TS:
        eng.add_data(rng.poisson(0.3, (T, N)).astype(float), basis=basis)
    eng.keep_logodds = True
    a = rng.random((NLOC, N)) < 0.5
    W = rng.standard_normal((NLOC, N, B)) * a[:, :, None]
    b = rng.standard_normal(NLOC) - 1.5

    acc = summary._DeviceAccumulators(eng, rates=True, pointwise=True)
    gof = rescale._DeviceFold(eng, 8, [2.0, 1.5, 3.0], seed=3)
    diag = diagnostics._DeviceDiag(eng, 3, diagnostics.SECTIONS)
    sl = slice(N0, N1)
    hyp = engine.prior_terms(np.tile(np.eye(B) * 4.0, (N, N, 1, 1)), np.zeros((N, N, B)), np.full(N, 2.0), np.full(N, -1.5))
    perm, u, z = engine.make_draws(1, 1, range(N0, N1), N, N * B)
    a, W, b, _ = eng.sweep(a, W, b, np.full((NLOC, N), 0.5), *[h[sl] for h in hyp], perm, u, z, seed=1, sweep=1)

    log = []

    def recorded(name, *args, **by_name):
        log.append((name, by_name))
        return _lib.call(name, *args, **by_name)
    for module in (engine, summary, rescale, diagnostics, dispersion):   # every module calls the library through its own binding of _lib.call
        monkeypatch.setattr(module, "call", recorded)

    def entries(fn):
        del log[:]
        out = fn()
        return [name for name, _ in log], [kw for _, kw in log], out
    eng.profile = True                                           # (after the sweep: its own stages stay out of the timings)
    walk = lambda fold: ["pgl_activation", fold] * 2
    psi = [ds.Psi.data_ptr() for ds in eng.datasets]

    def check_walk(kws, visited, elem0=True):
        """the fold launches in kws: data sets `visited` in order, accumulate 0 then 1, elem0 = the bins in front"""
        assert [kw["Psi"].value for kw in kws] == [psi[i] for i in visited]
        assert [kw["T"] for kw in kws] == [TS[i] for i in visited]
        assert [kw["accumulate"] for kw in kws] == [0, 1][:len(visited)]
        if elem0:
            assert [kw["elem0"] for kw in kws] == [(0, 70)[i] for i in visited]

    names, kws, ll = entries(lambda: acc.fold(eng, a, W, b, 1))
    assert names == walk("pgl_summary_fold") + ["pgl_summary_state"]
    check_walk(kws[1:4:2], (0, 1), elem0=False)
    assert [kw["T"] for kw in kws[0:4:2]] == list(TS)            # the activations, in data-set order

    names, kws, _ = entries(lambda: gof.fold(eng, a, W, b, 1))
    assert names == walk("pgl_rescale_fold") + ["pgl_rescale_ks"]
    check_walk(kws[1:4:2], (0, 1))
    assert [kw["neuron0"] for kw in kws[1:4:2]] == [N0, N0]

    names, kws, _ = entries(lambda: gof.fold(eng, a, W, b, 2, only=1))
    assert names == ["pgl_activation", "pgl_rescale_fold", "pgl_rescale_ks"]
    check_walk(kws[1:2], (1,))
    assert kws[0]["T"] == TS[1]

    names, kws, _ = entries(lambda: dispersion._DeviceStep(eng).stats(a, W, b, 1, 1))
    assert names == walk("pgl_dispersion_fold")
    check_walk(kws[1:4:2], (0, 1))

    names, kws, _ = entries(lambda: diag.fold(a, W, b, 1))
    assert names == ["pgl_diag_edge_conditional", "pgl_diag_fold"] and kws[1]["what"] == _lib.PGL_DIAG_ALL

    names, kws, ll_ref = entries(lambda: eng.log_likelihood(a, W, b))
    assert names == walk("pgl_pg_loglik_ex")
    check_walk(kws[1:4:2], (0, 1))
    np.testing.assert_array_equal(ll, ll_ref)

    times = eng.collect_timings()
    cells = float(sum(TS)) * NLOC
    assert {k: (v["calls"], v["work"]) for k, v in times.items()} == dict(
        activation=(9, 2.0 * N * B * (4 * cells + TS[1] * NLOC)), summary_fold=(2, cells), rescale_fold=(3, cells + TS[1] * NLOC),
        dispersion_fold=(2, cells), diag_fold=(1, float(diag.entries)), pg_loglik=(2, cells))


@pytest.mark.parametrize("kw, n0, n1", [(dict(n_covariates=1, n_latents=2), 0, 4), (dict(n_covariates=1, n_latents=2, latent_ar=0.5), 0, 4),
                                        (dict(n_covariates=2), 1, 4)], ids=["latents", "latent_ar", "covariates_on_a_shard"])
def test_the_gibbs_steps_go_through_the_walk(monkeypatch, kw, n0, n1):
    """the latent and the covariate step (latents._DeviceStep, covariates._DeviceStep) on a Bernoulli engine after one sweep: the entries
    they reach through fold_data -- without the offset, which only the walk's default adds (log_likelihood) --, the stages they time and
    the work they book, and their scratch: kept from call to call, regrown when a longer data set arrives"""
    from oracle import pyglm_oracle as orc
    from pyglm_amd import _lib, covariates, engine, latents
    rng = np.random.default_rng(12)
    basis = orc.cosine_basis(B, L=20) / 20
    nloc = n1 - n0
    eng = engine.GibbsEngine(N, B, n0, n1, device="cuda:0", **kw)
    K_obs, Q, K = eng.K_obs, eng.Q, eng.K

    def add(T):
        eng.add_data((rng.random((T, N)) < 0.3).astype(float), basis=basis, covariates=rng.standard_normal((T, K_obs)))
        if Q:
            eng.set_latents(len(eng.datasets) - 1, rng.standard_normal((T, Q)) * 0.3)
    for T in TS:
        add(T)
    eng.set_covariate_weights(rng.standard_normal((nloc, K)) * 0.5)
    a = rng.random((nloc, N)) < 0.5
    W = rng.standard_normal((nloc, N, B)) * a[:, :, None]
    b = rng.standard_normal(nloc) - 1.5
    hyp = engine.prior_terms(np.tile(np.eye(B) * 4.0, (N, N, 1, 1)), np.zeros((N, N, B)), np.full(N, 2.0), np.full(N, -1.5))
    perm, u, z = engine.make_draws(1, 1, range(n0, n1), N, N * B)
    a, W, b, _ = eng.sweep(a, W, b, np.full((nloc, N), 0.5), *[h[n0:n1] for h in hyp], perm, u, z, seed=1, sweep=1)
    lstep, cstep = latents._DeviceStep(eng), covariates._DeviceStep(eng)

    log = []

    def recorded(name, *args, **by_name):
        log.append((name, by_name))
        return _lib.call(name, *args, **by_name)
    for module in (engine, covariates, latents):
        monkeypatch.setattr(module, "call", recorded)

    def entries(fn):
        """-> the entries fn reaches, their keywords, and the stages timed meanwhile as {stage: (calls, work)}"""
        del log[:]
        eng.collect_timings()
        fn()
        return [name for name, _ in log], [kw for _, kw in log], {k: (v["calls"], v["work"]) for k, v in eng.collect_timings().items()}
    eng.profile = True
    bins = float(sum(TS))
    act = (2, 2.0 * N * B * bins * nloc)
    tensors = lambda step: {k: v.data_ptr() for k, v in vars(step.scratch).items() if hasattr(v, "data_ptr")}

    if Q:
        draw = "pgl_latent_ar_draw" if "latent_ar" in kw else "pgl_latent_draw"
        names, kws, times = entries(lambda: lstep.latent_step(a, W, b, 1, 1))
        assert names == ["pgl_activation", "pgl_latent_fold", draw] * 2
        for first in (1, 2):                                       # the folds, then the draws
            assert [(k["T"], k["col0"], k["lds"]) for k in kws[first::3]] == [(TS[0], K_obs, K), (TS[1], K_obs, K)]
        assert [k["elem0"] for k in kws[2::3]] == [0, TS[0]]
        assert K_obs == 1 and K == 3
        if "latent_ar" in kw:
            assert [k["scratch_bytes"] for k in kws[2::3]] == [_lib.load().pgl_latent_ar_scratch(TS[0], Q, 0)] * 2
        assert times == {"activation": act, "latent_fold": (2, bins * nloc), draw[4:]: (2, bins)}
        held = tensors(lstep)
        assert "Lam" in held and "r" in held
        lstep.latent_step(a, W, b, 1, 2)
        assert tensors(lstep) == held

    fold_draw_offset = ["pgl_covariate_draw"] + ["pgl_covariate_offset"] * 2
    stages = dict(covariate_fold=(2, bins * nloc), covariate_draw=(1, 0.0), covariate_offset=(1, 0.0))
    names, kws, times = entries(lambda: cstep.covariate_step(a, W, b, 1, 1, psi_ready=True))      # (only the sequence is looked at)
    assert names == ["pgl_covariate_fold"] * 2 + fold_draw_offset
    assert [(k["T"], k["accumulate"], k["nloc"]) for k in kws[:2]] == [(TS[0], 0, nloc), (TS[1], 1, nloc)]
    assert times == stages
    names, kws, times = entries(lambda: cstep.covariate_step(a, W, b, 1, 1))
    assert names == ["pgl_activation", "pgl_covariate_fold"] * 2 + fold_draw_offset
    assert [(k["T"], k["accumulate"], k["nloc"]) for k in kws[1:4:2]] == [(TS[0], 0, nloc), (TS[1], 1, nloc)]
    assert times == dict(stages, activation=act)
    held = tensors(cstep)
    assert "work" in held and "Lam" in held
    cstep.covariate_step(a, W, b, 1, 2)
    assert tensors(cstep) == held

    names, kws, _ = entries(lambda: eng.log_likelihood(a, W, b))   # the walk's default still adds the offset
    assert names == ["pgl_activation", "pgl_covariate_add_offset", "pgl_pg_loglik_ex"] * 2

    if Q:
        add(130)
        lstep.latent_step(a, W, b, 1, 3)
        assert lstep.scratch.Lam.shape[0] >= 130 and lstep.scratch.r.shape[0] >= 130
