"""The chain diagnostics (model.diagnose, pyglm_amd/diagnostics.py) on the host: the NumPy statement of the dyadic batch means against brute
force, the laws of the effective sample size and of R-hat, the conditional edge probabilities, the model-level class on the oracle engine,
and the third header.  CPU only.

What is compared how.  The brute force stacks the samples in longdouble, reshapes them to the level's batches, takes the batch means and
np.var(ddof = 1).  With n samples of magnitude max|x|, a running mean and a running sum of squared deviations differ from the two-pass
values by a few n eps max|x| and n eps max|x|^2 (eps = 2^-53): the bounds are 8 n eps max|x| for the means and 8 n eps max|x|^2 for M2 --
at values of mean 1e4 and spread 1, the cancellation case, that is ~1e-8 of an M2 of order n.  `pending` is a sum of 2^l values added
pairwise, the earlier half first: the same tree in float64 gives the same bits."""
import ctypes
import os

import numpy as np
import pytest

from pyglm_amd import diagnostics as D
from pyglm_amd import models as M
from tests._oracle_engine import OracleEngine

EPS = 2.0 ** -53


def tree_sum(x):
    """the pairwise sum of 2^l stacked values, the earlier half first, in float64"""
    return x[0] if len(x) == 1 else tree_sum(x[:len(x) // 2]) + tree_sum(x[len(x) // 2:])


def brute(x, levels):
    """pending (exact), mean, M2 of every level, (levels,) + x.shape[1:], from the stacked samples x (n, ...)"""
    x = np.asarray(x, dtype=np.float64)
    n, shape = x.shape[0], x.shape[1:]
    pending, mean, M2 = (np.zeros((levels,) + shape) for _ in range(3))
    xl = x.astype(np.longdouble)
    for l in range(levels):
        size, m = 1 << l, n >> l
        if m >= 1:
            bmeans = xl[:m * size].reshape((m, size) + shape).mean(axis=1)
            mean[l] = bmeans.mean(axis=0)
            if m >= 2:
                M2[l] = np.var(bmeans, axis=0, ddof=1) * (m - 1)
            j = m if m % 2 else m - 1                  # the last batch with an odd number: the first half that awaits (or awaited) its sibling
            if j >= 1:
                pending[l] = tree_sum(x[(j - 1) * size: j * size])
    return pending, mean, M2


def bounds(n, x):
    big = float(np.max(np.abs(x))) if np.size(x) else 0.0
    return 8 * n * EPS * big, 8 * n * EPS * big * big


def check_accumulators(pending, mean, M2, x, levels):
    """the three planes after folding the stacked samples x against brute force: pending bit-equal, (mean, M2) within the bounds"""
    n = len(x)
    p_ref, m_ref, M2_ref = brute(x, levels)
    tol_m, tol_M2 = bounds(n, x)
    assert np.array_equal(np.asarray(pending), p_ref)
    assert np.max(np.abs(np.asarray(mean) - m_ref), initial=0.0) <= tol_m
    assert np.max(np.abs(np.asarray(M2) - M2_ref), initial=0.0) <= tol_M2


def brute_readouts(x, levels, level=None):
    """dict(mean, mcse, ess, var) from the brute-force moments, by the definition's formulas"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    _, mean, M2 = brute(x, levels)
    l = D.reporting_level(n, levels) if level is None else level
    m = n >> l
    bv = (1 << l) * M2[l] / (m - 1)
    v0 = M2[0] / (n - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return dict(mean=mean[0], mcse=np.sqrt(bv / (m << l)), ess=n * v0 / bv, var=v0, bv=bv, M2_0=M2[0], M2_l=M2[l], level=l)


def check_readouts(got, x, levels, level=None):
    """got: an object with mean / mcse(level) / ess(level) of one read-out (a BatchMeans); x: the stacked samples.  The bounds on mean and M2
    carried through the formulas: mcse^2 = 2^l M2_l / ((m - 1) m 2^l) inherits M2's bound over (m - 1) m; ess = n v0 / bv is a ratio -- where
    both M2 are at least 1e4 of their bound it is compared at rtol 4 bound / min(M2), elsewhere only its NaN pattern (a constant entry)"""
    n = len(x)
    ref = brute_readouts(x, levels, level)
    tol_m, tol_M2 = bounds(n, x)
    l = ref["level"]
    m = n >> l
    assert np.max(np.abs(got.mean - ref["mean"]), initial=0.0) <= tol_m
    assert np.max(np.abs(got.mcse(level) ** 2 - ref["mcse"] ** 2), initial=0.0) <= tol_M2 / ((m - 1) * m)
    ess = np.asarray(got.ess(level), dtype=np.float64)
    const = (ref["M2_0"] == 0) & (ref["M2_l"] == 0)
    assert np.array_equal(np.isnan(ess), const)          # (a constant entry's deviations are exact zeros in every formulation)
    safe = np.minimum(ref["M2_0"], ref["M2_l"]) >= 1e4 * tol_M2
    if tol_M2 == 0:
        safe = ~const
    if np.any(safe):
        rtol = 4 * tol_M2 / np.minimum(ref["M2_0"], ref["M2_l"])[safe] + 8 * EPS
        assert np.all(np.abs(ess[safe] - ref["ess"][safe]) <= rtol * np.abs(ref["ess"][safe]))


# ------------------------------------------------------------------------------------------------ BatchMeans against brute force
@pytest.mark.parametrize("levels", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 64, 100])
def test_batch_means_against_brute_force(n, levels):
    rng = np.random.default_rng(100 * n + levels)
    x = 1e4 + rng.standard_normal((n, 3, 5))              # mean 1e4, spread 1: the cancellation case
    bm = D.batch_means_host(x, levels)
    assert bm.n == n and bm.M2.shape == (levels, 3, 5)
    check_accumulators(bm.pending, bm.mean_, bm.M2, x, levels)
    # pushing one by one is the same thing, and the counts are derived from n
    one = D.BatchMeans((3, 5), levels)
    for row in x:
        one.push(row)
    assert all(np.array_equal(u, v) for u, v in ((one.pending, bm.pending), (one.mean_, bm.mean_), (one.M2, bm.M2)))
    assert [bm.count(l) for l in range(levels)] == [n >> l for l in range(levels)]
    assert bm.level() == min(levels - 1, int(np.floor(np.log2(n) / 2)))
    for l in range(levels):
        if n >> l >= 2:
            np.testing.assert_allclose(bm.batch_var(l), (1 << l) * bm.M2[l] / ((n >> l) - 1), rtol=0, atol=0)
        else:
            with pytest.raises(RuntimeError, match="needs at least 2"):
                bm.batch_var(l)
            with pytest.raises(RuntimeError, match="needs at least 2"):
                bm.mcse(l)
            with pytest.raises(RuntimeError, match="needs at least 2"):
                bm.ess(l)
    if n >= 2:
        check_readouts(bm, x, levels)
        for l in range(levels):
            if n >> l >= 2:
                check_readouts(bm, x, levels, l)
    else:
        with pytest.raises(RuntimeError):
            bm.mcse()


def test_levels_are_checked_and_a_constant_entry_has_no_ess():
    for bad in (0, 17, 2.5):
        with pytest.raises(ValueError, match="levels"):
            D.BatchMeans((2,), bad)
    assert D.BatchMeans((), D.MAX_LEVELS).levels == 16
    bm = D.batch_means_host(np.stack([np.array([1.0, 2.0])] * 9 + [np.array([1.0, 3.0])] * 7), 3)
    assert np.isnan(bm.ess()[0]) and bm.ess()[1] > 0 and bm.mcse()[0] == 0
    with pytest.raises(ValueError, match="level 3"):
        bm.mcse(3)
    with pytest.raises(RuntimeError, match="no sample"):
        D.BatchMeans((2,), 3).mean
    part = D.BatchMeans.from_arrays(bm.pending[[0, 2]], bm.mean_[[0, 2]], bm.M2[[0, 2]], bm.n, 3, held=(0, 2))
    assert np.array_equal(part.mcse(2), bm.mcse(2)) and np.array_equal(part.ess(2), bm.ess(2), equal_nan=True)
    with pytest.raises(RuntimeError, match="not read back"):
        part.mcse(1)


# ------------------------------------------------------------------------------------------------ laws
# Seed 7 was chosen on the development machine so that the BRUTE-FORCE reference alone meets both laws below (it does, with room: the
# medians over 256 lanes are 1.01 and 1.19 times the true ratio; the second is the known bias of batches of 64 on an AR(1) chain of
# phi = 0.9, whose batch means still correlate); BatchMeans is then held to the same intervals and to the reference.
LAW_SEED, LANES, LAW_N, PHI = 7, 256, 4096, 0.9


@pytest.fixture(scope="module")
def law_chains():
    rng = np.random.default_rng(LAW_SEED)
    iid = rng.standard_normal((LAW_N, LANES))
    e = rng.standard_normal((LAW_N, LANES))
    ar = np.empty_like(e)
    ar[0] = e[0] / np.sqrt(1 - PHI ** 2)                   # stationary start
    for t in range(1, LAW_N):
        ar[t] = PHI * ar[t - 1] + e[t]
    iid.setflags(write=False), ar.setflags(write=False)
    return iid, ar


@pytest.mark.parametrize("kind, truth", [("iid", 1.0), ("ar1", (1 - PHI) / (1 + PHI))])
def test_ess_law(law_chains, kind, truth):
    x = law_chains[0 if kind == "iid" else 1]
    ref = np.median(brute_readouts(x, 8)["ess"]) / LAW_N
    got = np.median(D.batch_means_host(x, 8).ess()) / LAW_N
    print("%s: median ess / n  brute force %.5f  BatchMeans %.5f  truth %.5f" % (kind, ref, got, truth))
    assert 0.8 * truth <= ref <= 1.25 * truth, "the seed no longer serves: the brute-force reference misses the law"
    assert 0.8 * truth <= got <= 1.25 * truth
    assert abs(got - ref) <= 1e-9 * ref


def test_rhat(law_chains):
    iid, ar = law_chains
    for x in (iid, ar):
        chains = [D.batch_means_host(x[i * 1024:(i + 1) * 1024], 3) for i in range(4)]
        r = D.rhat(chains)
        assert r.shape == (LANES,) and np.median(r) < 1.05
        # against the formula on the stacked chains
        c = np.stack([x[i * 1024:(i + 1) * 1024] for i in range(4)]).astype(np.longdouble)
        Wv, Bv = c.var(axis=1, ddof=1).mean(axis=0), 1024 * c.mean(axis=1).var(axis=0, ddof=1)
        np.testing.assert_allclose(r, np.sqrt((1023.0 / 1024 * Wv + Bv / 1024) / Wv).astype(float), rtol=1e-12)
    assert np.max(D.rhat([D.batch_means_host(iid[i * 1024:(i + 1) * 1024], 3) for i in range(4)])) < 1.05
    shifted = [D.batch_means_host(iid[i * 1024:(i + 1) * 1024] + (2.0 if i == 3 else 0.0), 3) for i in range(4)]
    assert np.min(D.rhat(shifted)) > 1.2
    const = [D.batch_means_host(np.ones((8, 2)), 2) for _ in range(2)]
    assert np.all(np.isnan(D.rhat(const)))
    with pytest.raises(ValueError, match="two chains"):
        D.rhat(shifted[:1])
    with pytest.raises(ValueError, match="different lengths"):
        D.rhat([shifted[0], D.batch_means_host(iid[:8], 3)])


# ------------------------------------------------------------------------------------------------ the conditional edge probabilities
def conditional_case(N, nloc=None, seed=0):
    """(logodds, perm, a) with a NaN row, NaN entries, +-inf and one out-of-range perm entry (where N allows)"""
    rng = np.random.default_rng(seed)
    nloc = N if nloc is None else nloc
    lo = rng.standard_normal((nloc, N)) * 3
    perm = np.stack([rng.permutation(N) for _ in range(nloc)]).astype(np.int32)
    a = (rng.random((nloc, N)) < 0.5).astype(np.int32)
    lo[rng.random((nloc, N)) < 0.2] = np.nan
    lo[0, 0] = np.inf if N == 1 else lo[0, 0]
    if N >= 3:
        lo[1, :] = np.nan                                  # a row the sweep did not run
        lo[0, 0], lo[0, 1], lo[2, 0] = np.inf, -np.inf, 0.5
        perm[2, 0] = N                                     # out of range: skipped (the row's other steps still land)
        lo[2, 1], perm[2, 1] = 0.25, -1
    return lo, perm, a


@pytest.mark.parametrize("N", [1, 3, 65])
def test_edge_conditional_host(N):
    lo, perm, a = conditional_case(N)
    p = D.edge_conditional_host(lo, perm, a)
    assert p.shape == a.shape and p.dtype == np.float64
    want = a.astype(np.float64)
    touched = np.zeros(a.shape, dtype=bool)
    for n in range(a.shape[0]):
        ok = ~np.isnan(lo[n]) & (perm[n] >= 0) & (perm[n] < N)
        with np.errstate(over="ignore"):
            want[n, perm[n][ok]] = 1.0 / (1.0 + np.exp(-lo[n][ok]))
        touched[n, perm[n][ok]] = True
    assert np.array_equal(p, want)
    assert np.all(np.isin(p[~touched], (0.0, 1.0))) and np.array_equal(p[~touched], a[~touched].astype(float))
    assert np.all((p >= 0) & (p <= 1))
    if N >= 3:
        assert np.array_equal(p[1], a[1].astype(float))                       # the NaN row: its current values
        assert p[0, perm[0, 0]] == 1.0 and p[0, perm[0, 1]] == 0.0           # +-inf


# ------------------------------------------------------------------------------------------------ the model-level class on the oracle engine
def oracle_model(N=5, B=2, T=300):
    np.random.seed(0)
    model = M.SparseBernoulliGLM(N, B=B, regression_kwargs=dict(S_w=3.0, mu_b=-1.0), engine_factory=OracleEngine, seed=1)
    model.add_data((np.random.default_rng(3).random((T, N)) < 0.2).astype(float))
    return model


def check_chain_diagnostics(diag, stacks, levels, sections):
    """every read-out of a ChainDiagnostics against brute force over the stacked samples {read-out: (n, ...)}"""
    n = diag.count
    for what in sections:
        x = stacks[what]
        bm = diag._bm(what, range(levels))
        check_accumulators(bm.pending, bm.mean_, bm.M2, x, levels)
        check_readouts(bm, x, levels)
        ref = brute_readouts(x, levels)
        tol_m, tol_M2 = bounds(n, x)
        l = diag.level()
        assert np.max(np.abs(diag.mean(what) - ref["mean"]), initial=0.0) <= tol_m
        assert np.max(np.abs(diag.mcse(what) ** 2 - ref["mcse"] ** 2), initial=0.0) <= tol_M2 / (((n >> l) - 1) * (n >> l))
        assert np.array_equal(diag.ess(what), bm.ess(), equal_nan=True) and np.array_equal(diag.mcse(what, 0), bm.mcse(0))


def test_chain_diagnostics_on_the_oracle_engine():
    model = oracle_model()
    with pytest.raises(ValueError, match=r"diagnose\(rb=False\) works"):
        model.diagnose(rb=True)
    diag = model.diagnose(levels=3, rb=False)
    assert diag.sections == ("edge", "weight", "bias") and diag.count == 0
    acc = model.summarize(rates=False)
    stacks = dict(edge=[], weight=[], bias=[], ll=[])
    for it in range(11):
        model.resample_model()
        ll = acc.collect()
        assert diag.collect(ll=ll) == ll
        A, W = model.adjacency, model.weights
        stacks["edge"].append(A.astype(float)), stacks["weight"].append(np.where(A[:, :, None], W, 0.0)), stacks["bias"].append(model.biases)
        stacks["ll"].append(ll)
    stacks = {k: np.array(v) for k, v in stacks.items()}
    assert diag.count == 11 and diag.level() == 1 and diag.level(64) == 2 and diag.level(4) == 1
    check_chain_diagnostics(diag, stacks, 3, ("edge", "weight", "bias", "ll"))
    freq = stacks["edge"].mean(0)
    assert np.sum((freq > 0) & (freq < 1)) >= 5, "the fixture no longer exercises the edges"
    assert np.array_equal(diag.edge_prob, acc.edge_prob)                      # exactly: a count over n
    assert isinstance(diag.mean("ll"), float) and diag.mean("ll") == pytest.approx(stacks["ll"].mean(), rel=1e-12)
    worst = diag.min_ess()
    assert set(worst) == {"edge", "weight", "bias", "ll"}                     # (no neuron has a xi)
    for what, (value, index) in worst.items():
        e = np.asarray(diag.ess(what))
        assert value == np.nanmin(e) and e[index] == value
    with pytest.raises(ValueError, match="no read-out"):
        diag.mean("edge_rb")
    with pytest.raises(ValueError, match="level 3"):
        diag.mcse("edge", level=3)
    # without a log-likelihood of the caller's the model's own joins the trace
    before = diag._ll.n
    assert diag.collect() == model.log_likelihood() and diag._ll.n == before + 1
    # reset, and two chains from different seeds under R-hat
    diag.reset()
    assert diag.count == 0
    with pytest.raises(RuntimeError, match="no sample"):
        diag.mean("edge")
    other = oracle_model()
    other.seed = 2
    d2 = other.diagnose(levels=3, weights=False, rb=False)
    assert d2.sections == ("edge", "bias")
    for it in range(4):
        model.resample_model(), other.resample_model()
        diag.collect(), d2.collect()
    r = D.rhat([diag, d2], "bias")
    assert r.shape == (5,) and np.all(r > 0)
    assert np.array_equal(r, D.rhat([diag._bm("bias", (0,)), d2._bm("bias", (0,))]))
    assert D.rhat([diag, d2], "edge").shape == (5, 5) and D.rhat([diag, d2], "ll").shape == ()


# ------------------------------------------------------------------------------------------------ several ranks
def _run_ranks(world, rank, port, out_path):
    """the chain of oracle_model with diagnostics on `world` gloo ranks (shards of 3 and 2 neurons: the gather pads); rank 0 saves the read-outs"""
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    model = oracle_model()
    diag = model.diagnose(levels=3, rb=False)
    for it in range(9):
        model.resample_model()
        diag.collect()
    out = {}
    for what in ("edge", "weight", "bias", "ll"):
        out.update({what + "_mean": diag.mean(what), what + "_mcse": diag.mcse(what), what + "_ess": diag.ess(what),
                    what + "_mcse0": diag.mcse(what, 0)})
    out["edge_prob"] = diag.edge_prob
    out["worst"] = np.array([v[0] for v in diag.min_ess().values()])
    if rank == 0:
        np.savez(out_path, **out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_equal_one(tmp_path):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    one, two = str(tmp_path / "one.npz"), str(tmp_path / "two.npz")
    _run_ranks(1, 0, 0, one)
    mp.spawn(_run_ranks_worker, args=(2, port, two), nprocs=2, join=True)
    a, b = np.load(one), np.load(two)
    assert a["edge_mcse"].shape == (5, 5) and a["weight_ess"].shape == (5, 5, 2) and a["bias_mean"].shape == (5,) and a["ll_mcse"].shape == ()
    for k in a.files:
        # the rows are gathered, not recomputed: a rank's entries are the one-rank chain's wherever the states are (the exchange keeps them
        # within 1e-12, tests/test_distributed_gloo.py)
        np.testing.assert_allclose(a[k], b[k], rtol=1e-9, atol=1e-12, err_msg=k)
    assert np.array_equal(a["edge_prob"], b["edge_prob"])


def _run_ranks_worker(rank, world, port, out_path):
    _run_ranks(world, rank, port, out_path)


# ------------------------------------------------------------------------------------------------ the third header
def test_third_header_binds():
    from pyglm_amd import _lib
    assert sorted(_lib.DIAGNOSTICS_FUNCTIONS) == ["pgl_diag_bytes", "pgl_diag_edge_conditional", "pgl_diag_entries", "pgl_diag_fold"]
    assert _lib.DIAGNOSTICS_CONSTANTS == dict(PGL_DIAG_MAX_LEVELS=16, PGL_DIAG_EDGE=1, PGL_DIAG_EDGE_RB=2, PGL_DIAG_WEIGHT=4, PGL_DIAG_BIAS=8,
                                              PGL_DIAG_ALL=15)
    assert _lib.PGL_DIAG_MAX_LEVELS == D.MAX_LEVELS
    # (the device accumulators take their sections from D.SECTIONS itself: _DeviceDiag.mask / section_layout)
    assert D._DeviceDiag.mask(D.SECTIONS) == _lib.PGL_DIAG_ALL and [1 << i for i in range(4)] == [_lib.DIAGNOSTICS_CONSTANTS["PGL_DIAG_" + s.upper()]
                                                                                                   for s in D.SECTIONS]
    # the tables of the other two headers describe those headers alone; pyglm_hip.h still declares its 65
    assert len(_lib.FUNCTIONS) == 65
    for other in (_lib.FUNCTIONS, _lib.DISPERSION_FUNCTIONS):
        assert not set(_lib.DIAGNOSTICS_FUNCTIONS) & set(other)
    assert not set(_lib.DIAGNOSTICS_CONSTANTS) & (set(_lib.CONSTANTS) | set(_lib.DISPERSION_CONSTANTS))
    restype, params = _lib.DIAGNOSTICS_FUNCTIONS["pgl_diag_fold"]
    assert restype is ctypes.c_int and [p for p, _ in params] == ["a", "W", "b", "p", "pending", "mean", "M2", "N", "B", "nloc", "levels", "k",
                                                                   "what", "hip_stream"]
    assert dict(params)["k"] is ctypes.c_longlong and dict(params)["what"] is ctypes.c_uint and dict(params)["M2"] is ctypes.c_void_p
    assert _lib.DIAGNOSTICS_FUNCTIONS["pgl_diag_entries"] == (ctypes.c_long, [("N", ctypes.c_int), ("B", ctypes.c_int), ("nloc", ctypes.c_int),
                                                                              ("what", ctypes.c_uint)])
    assert _lib.DIAGNOSTICS_FUNCTIONS["pgl_diag_bytes"] == (ctypes.c_size_t, [("entries", ctypes.c_long), ("levels", ctypes.c_int)])
    assert [p for p, _ in _lib.DIAGNOSTICS_FUNCTIONS["pgl_diag_edge_conditional"][1]] == ["logodds", "perm", "a", "p", "nloc", "N", "hip_stream"]
    assert _lib._params("pgl_diag_fold") == _lib.DIAGNOSTICS_PARAMS["pgl_diag_fold"] and _lib._params("pgl_sweep") == _lib.PARAMS["pgl_sweep"]
    # every declared symbol is exported by the built library; the two size functions need no GPU
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, (restype, params) in _lib.DIAGNOSTICS_FUNCTIONS.items():
        fn = getattr(raw, name)
        fn.restype, fn.argtypes = restype, [t for _, t in params]
    assert raw.pgl_diag_entries(1024, 5, 1024, 15) == 1024 * (2 * 1024 + 5 * 1024 + 1)
    assert raw.pgl_diag_entries(3, 5, 2, 1) == 6 and raw.pgl_diag_entries(3, 5, 2, 4) == 30 and raw.pgl_diag_entries(3, 5, 2, 8) == 2
    assert raw.pgl_diag_entries(3, 5, 2, 16) == -1 and raw.pgl_diag_entries(-1, 5, 2, 1) == -1 and raw.pgl_diag_entries(0, 5, 2, 3) == 0
    assert raw.pgl_diag_bytes(1024 * (2 * 1024 + 5 * 1024 + 1), 8) == 3 * 8 * 8 * 1024 * (2 * 1024 + 5 * 1024 + 1)
    assert raw.pgl_diag_bytes(10, 0) == 0 and raw.pgl_diag_bytes(10, 17) == 0 and raw.pgl_diag_bytes(-1, 3) == 0
