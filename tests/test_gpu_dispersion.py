"""The dispersion fold on the GPU (pgl_dispersion_fold, pyglm_amd/csrc/pgl_dispersion.hip) against its definition, dispersion.dispersion_host:
rows on, before and after the edges of a workgroup's row block R = PGL_DISPERSION_ROWS, shards of 1, 63, 64, 65 and 70 columns, counts on,
before and after the threshold PGL_DISPERSION_COOP above which a wave finishes a cell together, data sets that add up, a shard with offset
pointers, refused arguments; then one step of a model that learns xi, and the chain against the same chain on the oracle engine.

What is compared how:
  L   exactly: integers, and every trial `u * (xi + i) < xi` is one addition, one multiplication and one comparison on both sides.
  S   |S - S_ref| <= (T + 8) 2^-53 S_ref, S_ref summed in long double from long-double terms of the SAME psi + bias (rounded to fp64 once,
      on both sides).  Derivation, in units of 2^-53 relative to S: the terms are positive, so a sum of T of them in ANY order makes at
      most T - 1 roundings of a partial sum that is at most S: T - 1.  A term max(x, 0) + log1p(exp(-|x|)): HIP documents 1 ulp (2 units)
      each for fp64 exp and log1p -- the relative error of exp passes through log1p undiminished at worst --, and the final addition
      rounds once: 5 units of the term, at most 5 of S.  T + 4 <= T + 8.
  The fold is called directly on uploaded psi, bias apart (what pgl_activation leaves); the model step reads psi back with engine.psi.

The fixed-xi path -- a model without xi_prior -- is covered by the existing GPU suite, which this file leaves as it is: tests/test_gpu_model.py,
test_gpu_parity.py and test_gpu_obs_hooks.py run negative-binomial models with scalar and per-neuron xi against the oracle.

Every call through _fold also checks that nothing was written behind L, S or work."""
import ctypes
import functools

import numpy as np
import pytest

from pyglm_amd import dispersion as disp
from tests.test_dispersion_host import XiOracleEngine, nb_counts

pytestmark = pytest.mark.gpu

R, COOP = disp.ROWS, disp.COOP_COUNT
GUARD, GARBAGE = 1024, 12345
SEED, SWEEP = 2 ** 40 + 99, 6
PLANTED = (1.0, 2.0, COOP - 1.0, float(COOP), COOP + 1.0, 5000.0)
TS = (0, 1, R - 1, R, R + 1, 3 * R + 17)
NLOCS = (1, 63, 64, 65, 70)


@functools.lru_cache(maxsize=None)
def _series(T, N, salt=0):
    """(psi, bias, Y, xi): psi + bias uniform on [-8, 3]; xi per column spread over [0.05, 40]; counts NB with a mean near 0.3; the planted
    counts in the first, the last and a mid-block row of columns 0, 63 and 64 (where they exist), all six in consecutive rows of ONE batch
    of eight rows of the first and of the last column (several large cells of one lane), and a row of large cells across every column"""
    rng = np.random.default_rng(1000 * T + N + salt)
    bias = rng.uniform(-1.0, 1.0, size=N)
    psi = rng.uniform(-8.0, 3.0, size=(T, N)) - bias
    xi = np.geomspace(0.05, 40.0, 70)[rng.permutation(70)[:N]]
    Y = nb_counts(rng, 1.0, np.full((T, N), np.log(0.3)))
    k = 0
    for row in sorted({0, T - 1, min(T - 1, R // 2 + 3)} if T else ()):
        for col in (0, 63, 64):
            if col < N:
                Y[row, col] = PLANTED[(k + salt) % 6]
                k += 1
    if T >= R:
        for col in {0, N - 1}:
            Y[R // 2 + 8:R // 2 + 14, col] = PLANTED
        Y[R - 9, :] = COOP + 1.0 + np.arange(N)
    for a in (psi, bias, Y, xi):
        a.setflags(write=False)
    return psi, bias, Y, xi


def _reference(psi, bias, Y, xi, neuron0, elem0):
    """(L, S_ref): L of the definition; S in long double"""
    x = psi + (0.0 if bias is None else bias)
    L, S = disp.dispersion_host(x, Y, xi, SEED, SWEEP, neuron0, elem0)
    xl = x.astype(np.longdouble)
    S_ref = (np.maximum(xl, 0) + np.log1p(np.exp(-np.abs(xl)))).sum(axis=0)
    assert np.all(np.abs(S - S_ref.astype(np.float64)) <= (x.shape[0] + 8) * 2.0 ** -53 * S_ref)      # (the host definition keeps the bound too)
    return L, S_ref


def _fold(sets, xi, ldn=None, cols=None, first_accumulate=0, start=None):
    """pgl_dispersion_fold on the data sets `sets` = [(psi (T, N), bias (N,) or None, Y (T, N), elem0), ...], accumulate = 1 after the first
    -> (L (nloc,) int64, S (nloc,)).  The outputs hold GARBAGE before the first call (or `start` = (L, S)).  ldn > N: rows of ldn doubles,
    the cells that are no part of psi and Y hold 1e6 (read, Y would be a million trials).  cols = (lo, hi): the shard of those columns,
    through pointers offset by lo and neuron0 = lo."""
    import torch
    from pyglm_amd._lib import call, load, ptr
    N = sets[0][0].shape[1]
    ldn = N if ldn is None else ldn
    lo, hi = cols or (0, N)
    nloc = hi - lo
    L = torch.full((nloc + GUARD,), GARBAGE, dtype=torch.int64, device="cuda")
    S = torch.full((nloc + GUARD,), float(GARBAGE), dtype=torch.float64, device="cuda")
    if start is not None:
        L[:nloc], S[:nloc] = torch.from_numpy(np.array(start[0])).cuda(), torch.from_numpy(np.array(start[1])).cuda()
    xid = torch.from_numpy(np.array(xi[lo:hi], dtype=np.float64)).cuda()
    tails = []
    for i, (psi, bias, Y, elem0) in enumerate(sets):
        T = psi.shape[0]
        wp, wy = np.full((T, ldn), 1e6), np.full((T, ldn), 1e6)
        wp[:, :N], wy[:, :N] = psi, Y
        P, Yd = torch.from_numpy(wp).cuda(), torch.from_numpy(wy).cuda()
        bd = None if bias is None else torch.from_numpy(np.array(bias[lo:hi])).cuda()
        nbytes = load().pgl_dispersion_work_bytes(nloc, T)
        assert nbytes == max(16, 16 * -(-T // R) * nloc)
        work = torch.empty(nbytes + GUARD, dtype=torch.uint8, device="cuda")
        work[nbytes:] = 0xA5
        tails.append(work[nbytes:])
        off = lambda t: ctypes.c_void_p(t.data_ptr() + 8 * lo) if T else None
        call("pgl_dispersion_fold", Psi=off(P), ldn=ldn, bias=ptr(bd), Y=off(Yd), T=T, nloc=nloc, xi=ptr(xid), seed=SEED, sweep=SWEEP, neuron0=lo,
             elem0=elem0, L=ptr(L), S=ptr(S), accumulate=1 if i else first_accumulate, work=ptr(work), hip_stream=None)
        torch.cuda.synchronize()
    assert all(bool((t == 0xA5).all()) for t in tails), "bytes behind `work` were written"
    assert bool((L[nloc:] == GARBAGE).all()) and bool((S[nloc:] == float(GARBAGE)).all()), "elements behind L or S were written"
    return L[:nloc].cpu().numpy(), S[:nloc].cpu().numpy()


def _check(got, want, T):
    (L, S), (L_ref, S_ref) = got, want
    err = np.abs(S.astype(np.longdouble) - S_ref)
    bound = (T + 8) * 2.0 ** -53 * S_ref
    print("T = %d: max |S - S_ref| / bound = %.3f; L total %d" % (T, float(np.max(err / np.maximum(bound, 1e-300))) if T else 0.0, int(L.sum())))
    np.testing.assert_array_equal(L, L_ref)
    assert np.all(err <= bound)


@pytest.mark.parametrize("nloc", NLOCS)
@pytest.mark.parametrize("T", TS)
def test_fold_is_the_definition(T, nloc):
    psi, bias, Y, xi = _series(T, nloc)
    got = _fold([(psi, bias, Y, 0)], xi)
    if T == 0:
        assert got[0].tolist() == [0] * nloc and got[1].tolist() == [0.0] * nloc
        return
    if T >= R:
        assert (Y > COOP).sum() >= nloc and Y.max() == 5000.0
    _check(got, _reference(psi, bias, Y, xi, 0, 0), T)


@pytest.mark.parametrize("T", [R, 3 * R + 17])
@pytest.mark.parametrize("salt", [1, 2, 3, 4, 5])
def test_every_planted_count_in_every_named_cell(T, salt):
    """the nine named cells -- first, last and a mid-block row of columns 0, 63 and 64 -- take PLANTED[(k + salt) % 6], k the cell's index:
    with salt 0 (test_fold_is_the_definition) and these five every planted count has been in every one of them"""
    psi, bias, Y, xi = _series(T, 70, salt)
    rows, cols = sorted({0, T - 1, R // 2 + 3}), (0, 63, 64)
    assert [Y[r, c] for r in rows for c in cols] == [PLANTED[(k + salt) % 6] for k in range(9)]
    _check(_fold([(psi, bias, Y, 0)], xi), _reference(psi, bias, Y, xi, 0, 0), T)


def test_layouts_bias_and_stream_offsets():
    T, N = 3 * R + 17, 70
    psi, bias, Y, xi = _series(T, N)
    want = _reference(psi, bias, Y, xi, 0, 0)
    _check(_fold([(psi, bias, Y, 0)], xi, ldn=N + 6), want, T)                       # padded rows
    _check(_fold([(psi, None, Y, 0)], xi), _reference(psi, None, Y, xi, 0, 0), T)      # no bias
    base = _fold([(psi, bias, Y, 0)], xi)
    moved = _fold([(psi, bias, Y, 12345)], xi)                                         # the element offset moves the uniforms, not S
    _check(moved, _reference(psi, bias, Y, xi, 0, 12345), T)
    assert moved[0].tolist() != base[0].tolist() and moved[1].view(np.uint64).tolist() == base[1].view(np.uint64).tolist()


def test_shard_has_the_bits_of_the_whole():
    """columns 64 .. 69 folded alone with neuron0 = 64: S as raw 64-bit words, L exactly; and so for a shard that starts inside a group"""
    T, N = 3 * R + 17, 70
    psi, bias, Y, xi = _series(T, N)
    L, S = _fold([(psi, bias, Y, 0)], xi)
    for lo, hi in [(64, 70), (0, 64), (3, 37), (69, 70)]:
        Ls, Ss = _fold([(psi, bias, Y, 0)], xi, cols=(lo, hi))
        np.testing.assert_array_equal(Ls, L[lo:hi])
        np.testing.assert_array_equal(Ss.view(np.uint64), S[lo:hi].view(np.uint64))


def test_data_sets_add_up():
    T, N = 3 * R + 17, 70
    psi, bias, Y, xi = _series(T, N)
    psi2, bias2, Y2, _ = _series(R + 5, N, salt=1)
    got = _fold([(psi, bias, Y, 0), (psi2, bias, Y2, T)], xi)
    L1, S1 = _reference(psi, bias, Y, xi, 0, 0)
    L2, S2 = _reference(psi2, bias, Y2, xi, 0, T)
    np.testing.assert_array_equal(got[0], L1 + L2)
    assert np.all(np.abs(got[1].astype(np.longdouble) - (S1 + S2)) <= (T + R + 5 + 9) * 2.0 ** -53 * (S1 + S2))     # (one more addition)
    first = _fold([(psi, bias, Y, 0)], xi)
    one = _fold([(psi2, bias, Y2, T)], xi, first_accumulate=1, start=first)            # accumulate = 1 on what an earlier call left
    np.testing.assert_array_equal(one[0], got[0])
    np.testing.assert_array_equal(one[1].view(np.uint64), got[1].view(np.uint64))
    empty = _fold([(psi[:0], bias, Y[:0], 0)], xi, first_accumulate=1, start=first)    # T = 0 adds nothing
    np.testing.assert_array_equal(empty[0], first[0])
    np.testing.assert_array_equal(empty[1], first[1])


def test_refused_arguments_write_nothing():
    import torch
    from pyglm_amd._lib import load, ptr
    lib = load()
    T, N = 40, 5
    P, Yd = torch.zeros(T, N, dtype=torch.float64, device="cuda"), torch.ones(T, N, dtype=torch.float64, device="cuda")
    xi = torch.ones(N, dtype=torch.float64, device="cuda")
    L = torch.full((N,), GARBAGE, dtype=torch.int64, device="cuda")
    S = torch.full((N,), float(GARBAGE), dtype=torch.float64, device="cuda")
    work = torch.zeros(lib.pgl_dispersion_work_bytes(N, T) + 8, dtype=torch.uint8, device="cuda")
    good = dict(Psi=ptr(P), ldn=N, bias=None, Y=ptr(Yd), T=T, nloc=N, xi=ptr(xi), seed=1, sweep=0, neuron0=0, elem0=0, L=ptr(L), S=ptr(S),
                accumulate=0, work=ptr(work), hip_stream=None)
    from pyglm_amd import _lib
    names = _lib.DISPERSION_PARAMS["pgl_dispersion_fold"]
    for bad in [dict(nloc=0), dict(T=-1), dict(ldn=N - 1), dict(xi=None), dict(L=None), dict(S=None), dict(accumulate=2), dict(accumulate=-1),
                dict(Psi=None), dict(Y=None), dict(work=None), dict(work=ctypes.c_void_p(work.data_ptr() + 4))]:
        kw = dict(good, **bad)
        assert lib.pgl_dispersion_fold(*[kw[k] for k in names]) == 1, bad                # PGL_ERR_ARG
        assert b"argument check failed" in lib.pgl_last_error()
    torch.cuda.synchronize()
    assert bool((L == GARBAGE).all()) and bool((S == float(GARBAGE)).all())
    assert lib.pgl_dispersion_fold(*[good[k] for k in names]) == 0
    torch.cuda.synchronize()
    assert L.tolist() == [T] * N


# ------------------------------------------------------------------------------------------------ the model
def _basis():
    from pyglm_amd.utils.basis import cosine_basis
    return cosine_basis(B=1, L=50) / 50


@functools.lru_cache(maxsize=None)
def _recording():
    """T = 10 000 bins of N = 4 self-inhibiting negative-binomial neurons at xi* = 2"""
    from pyglm_amd.models import SparseNegativeBinomialGLM
    np.random.seed(11)
    N = 4
    true = SparseNegativeBinomialGLM(N, basis=_basis(), regression_kwargs=dict(S_w=10.0, mu_b=-2., xi=2.0), seed=1, engine_factory=XiOracleEngine)
    for n in range(N):
        r = true.regressions[n]
        r.a[:] = False
        r.W[:] = 0
        r.a[n] = True
        r.W[n, :] = -2.0
        r.b[:] = -1.0
    _, Y = true.generate(T=10000, keep=False)
    Y.setflags(write=False)
    return Y


def _model(prior=(1.0, 1.0), xis=None, seed=21, factory=None):
    """the model on the recording; xis: one fixed xi per neuron, set before the engine is built"""
    from pyglm_amd.models import SparseNegativeBinomialGLM
    np.random.seed(5)
    kw = dict(S_w=10.0, mu_b=-2., xi=1.0)
    if prior is not None:
        kw["xi_prior"] = prior
    m = SparseNegativeBinomialGLM(4, basis=_basis(), regression_kwargs=kw, seed=seed, engine_factory=factory)
    for r, x in zip(m.regressions, xis if xis is not None else ()):
        r.xi = float(x)
    m.add_data(np.array(_recording()))
    return m


def test_one_model_step():
    Y = _recording()
    T = Y.shape[0]
    m = _model()
    gof = m.time_rescaling(bins=16, seed=3)
    m.resample_model()
    a, W, b = m._local_state()
    L, S = disp.dispersion_host(m.engine.psi(a, W, b, 0), Y, 1.0, m.seed, 0, 0, 0)
    xi = np.array([r.xi for r in m.regressions])
    want = np.array([disp.draw_xi(r, int(L[i]), float(S[i]), m.seed, 0, i) for i, r in enumerate(m.regressions)])
    print("xi after one sweep", xi, "relative error / bound", np.abs(xi - want) / want / ((T + 10) * 2.0 ** -53))
    assert np.all(xi != 1.0) and np.all(np.abs(xi - want) <= (T + 10) * 2.0 ** -53 * want)
    np.testing.assert_array_equal(m.engine.obs_param.cpu().numpy(), xi)
    # the readers of xi: each against a fresh fixed-xi model built at that xi and put at the same state
    fixed = _model(prior=None, xis=xi, seed=33)
    fixed._store_rows(0, 4, m.adjacency, m.weights, m.biases)
    assert m.log_likelihood() == fixed.log_likelihood()
    held = np.array(Y[:500])
    assert m.log_likelihood([held]) == fixed.log_likelihood([held])
    s1, s2 = m.simulate(200, replicates=2, seed=4), fixed.simulate(200, replicates=2, seed=4)
    np.testing.assert_array_equal(s1.Y, s2.Y)
    gof.collect()                                                 # built BEFORE xi moved: the parameter is read again
    g2 = fixed.time_rescaling(bins=16, seed=3)
    g2.collect()
    np.testing.assert_array_equal(gof.hist_last, g2.hist_last)
    np.testing.assert_array_equal(gof.zsum_last.view(np.uint64), g2.zsum_last.view(np.uint64))
    acc = m.summarize(rates=False)
    assert acc.collect() == fixed.log_likelihood()
    np.testing.assert_array_equal(acc.xi_mean, xi)
    m.resample_model()                                            # a second sweep: _check_obs accepts the moved xi
    assert np.all(np.array([r.xi for r in m.regressions]) != xi)
    # the stand-alone regression takes the same step through its one-neuron engine
    from pyglm_amd.regression import SparseNegativeBinomialRegression
    np.random.seed(2)
    reg = SparseNegativeBinomialRegression(4, 1, xi=1.0, xi_prior=(1.0, 1.0), S_w=10.0, mu_b=-2.0)
    X = np.asarray(m.data_list[0][0])[:2000]
    reg.resample([(X, Y[:2000, 0])], seed=9, sweep=0)
    eng = reg._engine([(X, Y[:2000, 0])])
    Lr, Sr = disp.dispersion_host(eng.psi(reg.a[None], reg.W[None], reg.b), Y[:2000, :1], 1.0, 9, 0, 0, 0)
    want = disp.draw_xi(reg, int(Lr[0]), float(Sr[0]), 9, 0, 0)
    assert reg.xi != 1.0 and abs(reg.xi - want) <= (2000 + 10) * 2.0 ** -53 * want
    reg.resample([(X, Y[:2000, 0])], seed=9, sweep=1)
    # an engine built from a scalar xi cannot change it
    with pytest.raises(ValueError, match="scalar"):
        _model(prior=None).engine.set_obs_param(np.full(4, 2.0))


def test_checks_built_before_xi_moved_follow_it_on_the_device():
    """conditional_check, summarize(pointwise=True) and means of a learning model, built BEFORE the sweep that moves xi, against the same
    objects of a fresh fixed-xi model at the moved xi and the same state, all on the device: bit for bit"""
    m = _model()
    cp = m.conditional_check([0, 2], replicates=3, seed=6, start=100, stop=1100)
    acc = m.summarize(rates=True, pointwise=True)
    m.resample_model()
    xi = np.array([r.xi for r in m.regressions])
    assert np.all(xi != 1.0)
    fixed = _model(prior=None, xis=xi, seed=33)
    fixed._store_rows(0, 4, m.adjacency, m.weights, m.biases)
    np.testing.assert_array_equal(m.means[0], fixed.means[0])
    c2 = fixed.conditional_check([0, 2], replicates=3, seed=6, start=100, stop=1100)
    for c in (cp, c2):
        c.collect()
        c.collect()
    np.testing.assert_array_equal(cp.rate_mean, c2.rate_mean)
    np.testing.assert_array_equal(cp.rate_std, c2.rate_std)
    np.testing.assert_array_equal(cp.log_score()["per_bin"], c2.log_score()["per_bin"])
    stale = _model(prior=None, seed=34)                               # ... and not what the constructor's xi = 1 gives
    stale._store_rows(0, 4, m.adjacency, m.weights, m.biases)
    c3 = stale.conditional_check([0, 2], replicates=3, seed=6, start=100, stop=1100)
    c3.collect()
    c3.collect()
    assert not np.array_equal(c3.log_score()["per_neuron"], c2.log_score()["per_neuron"])
    a2 = fixed.summarize(rates=True, pointwise=True)
    for a in (acc, a2):
        a.collect()
        a.collect()
    assert acc.log_likelihoods == a2.log_likelihoods
    np.testing.assert_array_equal(acc.lppd()["per_neuron"], a2.lppd()["per_neuron"])
    assert acc.waic()["waic"] == a2.waic()["waic"]
    np.testing.assert_array_equal(acc.rate_mean[0], a2.rate_mean[0])


def test_chain_agrees_with_the_host_chain():
    """two chains of 300 sweeps (the first 100 dropped) on the recording at xi* = 2, independent seeds: one on the GPU, one on the CPU through
    the oracle engine and dispersion_host.  The measure is the CPU chain, built on the NumPy definition: the posterior means of xi agree
    within 4 x the larger of the two chains' standard deviations, and xi* lies inside the CPU chain's central 99 % range"""
    chains = []
    for factory, seed in [(None, 21), (XiOracleEngine, 22)]:
        m = _model(seed=seed, factory=factory)
        xs = []
        for it in range(300):
            m.resample_model()
            if it >= 100:
                xs.append([r.xi for r in m.regressions])
        chains.append(np.array(xs))
    gpu, cpu = chains
    sd = np.maximum(gpu.std(axis=0), cpu.std(axis=0))
    lo, hi = np.percentile(cpu, [0.5, 99.5], axis=0)
    print("GPU chain xi mean", gpu.mean(axis=0).round(3), "sd", gpu.std(axis=0).round(3))
    print("CPU chain xi mean", cpu.mean(axis=0).round(3), "sd", cpu.std(axis=0).round(3), "99 % range", lo.round(3), hi.round(3))
    assert np.all(np.abs(gpu.mean(axis=0) - cpu.mean(axis=0)) <= 4 * sd)
    assert np.all((lo <= 2.0) & (2.0 <= hi))
