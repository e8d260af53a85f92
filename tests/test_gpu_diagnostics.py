"""The chain diagnostics on the GPU (pgl_diag_fold, pgl_diag_edge_conditional: pyglm_amd/csrc/pgl_diag.hip) against their definitions in
pyglm_amd/diagnostics.py: the fold on synthetic device arrays whose entry counts fall below one workgroup, straddle its edge and leave a
remainder, over carries that reach level 4 and pass the cap of three levels; the conditional edge probabilities with NaN rows, infinities and
an out-of-range proposal; the model-level class over 17 sweeps of the general flip path, the small-model launch and a Gaussian model; shards;
guards; and that a chain does not notice its diagnostics.

What is compared how (tests/test_diagnostics_host.py states the bounds and the brute force): `pending` is a pairwise sum, the earlier half
first -- bit-equal; (mean, M2) within 8 n eps max|x| and 8 n eps max|x|^2 of the brute force in longdouble (the device contracts the Welford
step's multiply-add, NumPy does not: both are inside the bound); a conditional probability within 8 eps of NumPy's (one exp, one division),
and exactly 0.0 or 1.0 where no proposal landed.  A section `what` does not name has no entries in the accumulators (pgl_diag_entries), so
"untouched" is shown on what lies around them: a canary-filled guard behind every plane's buffer, NULL for the inputs of the sections not
named (they cannot have been read), and the levels a sample does not reach keeping their bits."""
import ctypes

import numpy as np
import pytest

from tests import test_diagnostics_host as host_tests

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
CANARY = -7.25e77
GUARD = 67
BITS = dict(edge=1, edge_rb=2, weight=4, bias=8)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda")


def _planes(levels, entries):
    """three zeroed [levels][entries] buffers, each with a canary-filled guard behind it"""
    import torch
    out = []
    for _ in range(3):
        t = torch.full((levels * entries + GUARD,), CANARY, dtype=torch.float64, device="cuda")
        t[:levels * entries] = 0.0
        out.append(t)
    return out


def _section_values(a, W, b, p, N, B):
    """the entries' values, by section, as the definition states them"""
    on = a != 0
    return dict(edge=np.where(on, 1.0, 0.0), edge_rb=p, weight=np.where(np.repeat(on, B, axis=1), W, 0.0), bias=b)


# ------------------------------------------------------------------------------------------------ pgl_diag_fold on synthetic arrays
@pytest.mark.parametrize("levels", [1, 3, 8])
@pytest.mark.parametrize("N, B, nloc", [(1, 1, 1), (3, 5, 3), (65, 1, 65), (17, 3, 5)])
def test_fold_against_the_definition(N, B, nloc, levels):
    import torch
    from pyglm_amd import _lib
    from pyglm_amd import diagnostics as D
    from pyglm_amd._lib import call, ptr
    lib = _lib.load()
    rng = np.random.default_rng(1000 * N + 10 * B + levels)
    K = 17
    # per sample: a with values other than 0 / 1 among them, W and b of mean 1e4 and spread 1 (the cancellation case), p in [0, 1]
    As = rng.integers(-1, 3, size=(K, nloc, N)).astype(np.int32)
    Ws = 1e4 + rng.standard_normal((K, nloc, N * B))
    bs = 1e4 + rng.standard_normal((K, nloc))
    ps = rng.random((K, nloc, N))
    values = [_section_values(As[k], Ws[k], bs[k], ps[k], N, B) for k in range(K)]
    order = ("edge", "edge_rb", "weight", "bias")
    for mask in (1, 2, 4, 8, 15):
        names = [s for s in order if BITS[s] & mask]
        E = lib.pgl_diag_entries(N, B, nloc, mask)
        assert E == sum(values[0][s].size for s in names)
        assert lib.pgl_diag_bytes(E, levels) == 3 * levels * E * 8
        pending, mean, M2 = _planes(levels, E)
        stack = np.stack([np.concatenate([values[k][s].reshape(-1) for s in names]) for k in range(K)])
        for k in range(1, K + 1):
            before = [t.clone() for t in (pending, mean, M2)]
            # the inputs of the sections not named are NULL: they cannot be read
            a_d = _dev(As[k - 1]) if mask & 5 else None
            W_d = _dev(Ws[k - 1]) if mask & 4 else None
            b_d = _dev(bs[k - 1]) if mask & 8 else None
            p_d = _dev(ps[k - 1]) if mask & 2 else None
            call("pgl_diag_fold", a=ptr(a_d), W=ptr(W_d), b=ptr(b_d), p=ptr(p_d), pending=ptr(pending), mean=ptr(mean), M2=ptr(M2), N=N, B=B,
                 nloc=nloc, levels=levels, k=k, what=mask, hip_stream=None)
            torch.cuda.synchronize()
            got = [t[:levels * E].cpu().numpy().reshape(levels, E) for t in (pending, mean, M2)]
            host_tests.check_accumulators(*got, stack[:k], levels)
            tz = (k & -k).bit_length() - 1
            top = min(tz, levels - 1)
            for t, t0 in zip((pending, mean, M2), before):
                assert torch.all(t[levels * E:] == CANARY)                                       # the guard
                assert torch.equal(t[(top + 1) * E:levels * E], t0[(top + 1) * E:levels * E])      # the levels this sample does not reach
            if tz > levels - 1:
                # past the cap: the last level took a batch mean (check_accumulators above: its count is k >> top, twice what a level above
                # would count) and kept its pending first half
                assert torch.equal(pending[top * E:(top + 1) * E], before[0][top * E:(top + 1) * E])
        ref = D.batch_means_host(stack, levels)
        assert np.array_equal(got[0], ref.pending)
        tol_m, tol_M2 = host_tests.bounds(K, stack)
        assert np.max(np.abs(got[1] - ref.mean_)) <= tol_m and np.max(np.abs(got[2] - ref.M2)) <= tol_M2


def test_fold_refuses_bad_arguments_and_writes_nothing():
    import torch
    from pyglm_amd import _lib
    from pyglm_amd._lib import ptr
    lib = _lib.load()
    N, B, nloc, levels = 3, 2, 3, 3
    E = lib.pgl_diag_entries(N, B, nloc, 15)
    bufs = [torch.full((levels * E,), CANARY, dtype=torch.float64, device="cuda") for _ in range(3)]
    a, W, b, p = _dev(np.ones((nloc, N), np.int32)), _dev(np.ones((nloc, N * B))), _dev(np.ones(nloc)), _dev(np.ones((nloc, N)))
    good = dict(a=ptr(a), W=ptr(W), b=ptr(b), p=ptr(p), pending=ptr(bufs[0]), mean=ptr(bufs[1]), M2=ptr(bufs[2]), N=N, B=B, nloc=nloc,
                levels=levels, k=1, what=15, hip_stream=None)
    names = _lib.DIAGNOSTICS_PARAMS["pgl_diag_fold"]
    bad_cases = [dict(levels=0), dict(levels=17), dict(levels=-1), dict(k=0), dict(k=-4), dict(N=-1), dict(B=-1), dict(nloc=-1), dict(what=0),
                 dict(what=16), dict(what=31), dict(a=None), dict(W=None), dict(b=None), dict(p=None), dict(a=None, what=1), dict(a=None, what=4),
                 dict(p=None, what=2), dict(W=None, what=4), dict(b=None, what=8), dict(pending=None), dict(mean=None), dict(M2=None),
                 dict(B=0, what=4)]
    for bad in bad_cases:
        kw = dict(good, **bad)
        assert lib.pgl_diag_fold(*[kw[n] for n in names]) == 1, bad
        assert b"argument check failed" in lib.pgl_last_error()
    cond = _lib.DIAGNOSTICS_PARAMS["pgl_diag_edge_conditional"]
    lo, perm, pc = _dev(np.zeros((nloc, N))), _dev(np.zeros((nloc, N), np.int32)), torch.full((nloc * N,), CANARY, dtype=torch.float64, device="cuda")
    goodc = dict(logodds=ptr(lo), perm=ptr(perm), a=ptr(a), p=ptr(pc), nloc=nloc, N=N, hip_stream=None)
    for bad in [dict(logodds=None), dict(perm=None), dict(a=None), dict(p=None), dict(nloc=-1), dict(N=-1)]:
        kw = dict(goodc, **bad)
        assert lib.pgl_diag_edge_conditional(*[kw[n] for n in cond]) == 1, bad
    torch.cuda.synchronize()
    assert all(torch.all(t == CANARY) for t in bufs + [pc])
    # what the mask does not name may be NULL; an empty shard launches nothing
    for t in bufs:
        t[:nloc] = 0.0                                    # (level 0 of the bias section alone: the entries sample 1 touches)
    assert lib.pgl_diag_fold(*[dict(good, a=None, W=None, p=None, what=8)[n] for n in names]) == 0
    assert lib.pgl_diag_fold(*[dict(good, nloc=0)[n] for n in names]) == 0
    assert lib.pgl_diag_edge_conditional(*[dict(goodc, nloc=0)[n] for n in cond]) == 0
    torch.cuda.synchronize()
    assert all(torch.all(t[nloc:] == CANARY) for t in bufs) and torch.all(pc == CANARY)
    assert torch.all(bufs[0][:nloc] == 1.0) and torch.all(bufs[1][:nloc] == 1.0) and torch.all(bufs[2][:nloc] == 0.0)


# ------------------------------------------------------------------------------------------------ pgl_diag_edge_conditional
@pytest.mark.parametrize("N", [1, 3, 65])
def test_edge_conditional_against_the_definition(N):
    import torch
    from pyglm_amd import diagnostics as D
    from pyglm_amd._lib import call, ptr
    lo, perm, a = host_tests.conditional_case(N, seed=N)
    nloc = a.shape[0]
    p = torch.full((nloc * N + GUARD,), CANARY, dtype=torch.float64, device="cuda")
    lo_d, perm_d, a_d = _dev(lo), _dev(perm), _dev(a)
    call("pgl_diag_edge_conditional", logodds=ptr(lo_d), perm=ptr(perm_d), a=ptr(a_d), p=ptr(p), nloc=nloc, N=N, hip_stream=None)
    torch.cuda.synchronize()
    assert torch.all(p[nloc * N:] == CANARY)                                   # the guard behind p: the out-of-range proposals stored nothing
    got, want = p[:nloc * N].cpu().numpy().reshape(nloc, N), D.edge_conditional_host(lo, perm, a)
    assert np.max(np.abs(got - want)) <= 8 * EPS
    touched = np.zeros(a.shape, dtype=bool)
    for n in range(nloc):
        ok = ~np.isnan(lo[n]) & (perm[n] >= 0) & (perm[n] < N)
        touched[n, perm[n][ok]] = True
    assert np.array_equal(got[~touched], (a[~touched] != 0).astype(float))      # exactly 0.0 or 1.0
    if N >= 3:
        assert got[0, perm[0, 0]] == 1.0 and got[0, perm[0, 1]] == 0.0         # +-inf
        assert np.array_equal(got[1], (a[1] != 0).astype(float))               # the NaN row


# ------------------------------------------------------------------------------------------------ the model-level class
def _model(kind, N=4, B=2, T=500, seed=1, **engine_kwargs):
    from pyglm_amd import models as M
    np.random.seed(0)
    rng = np.random.default_rng(3)
    if kind == "gaussian":
        model = M.SparseGaussianGLM(N, B=B, seed=seed, engine_kwargs=engine_kwargs)
        Y = rng.standard_normal((T, N))
    else:
        model = M.SparseBernoulliGLM(N, B=B, regression_kwargs=dict(S_w=1.0, mu_b=-1.0), seed=seed, engine_kwargs=engine_kwargs)
        Y = (rng.random((T, N)) < 0.2).astype(float)
    model.add_data(Y)
    return model


def _sweep_perm(eng):
    """the proposal order of the engine's last sweep, read back from where the sweep put it"""
    import torch
    raw = eng._din[eng._perm_off:eng._perm_off + 4 * eng.nloc * eng.N]
    return raw.view(torch.int32).view(eng.nloc, eng.N).cpu().numpy()


@pytest.mark.parametrize("kind, B, engine_kwargs", [("bernoulli", 2, dict(visit_order=False)),      # the general flip path (pgl_flips.hip)
                                                     ("bernoulli", 2, {}), ("bernoulli", 1, {}),     # the small-model launch (pgl_small.hip)
                                                     ("gaussian", 2, {})])
def test_model_readouts_against_the_definition(kind, B, engine_kwargs):
    from pyglm_amd import diagnostics as D
    N, levels, sweeps = 4, 3, 17
    model = _model(kind, N=N, B=B, **engine_kwargs)
    eng = model.engine
    assert not eng.keep_logodds
    diag = model.diagnose(levels=levels)
    assert eng.keep_logodds and diag.sections == ("edge", "edge_rb", "weight", "bias")
    acc = model.summarize(rates=False)
    stacks = dict(edge=[], edge_rb=[], weight=[], bias=[], ll=[])
    for it in range(sweeps):
        model.resample_model()
        ll = acc.collect()
        assert diag.collect(ll=ll) == ll
        lo, perm = eng.logodds.cpu().numpy(), _sweep_perm(eng)
        A, W = model.adjacency, model.weights
        assert sorted(perm[0].tolist()) == list(range(N))
        # the conditionals the device formed, against the definition from the read-back log-odds, proposal order and state
        p_dev = diag._acc.p.cpu().numpy()
        p_host = D.edge_conditional_host(lo, perm, A)
        assert np.max(np.abs(p_dev - p_host)) <= 8 * EPS
        stacks["edge"].append(A.astype(float)), stacks["edge_rb"].append(p_dev), stacks["weight"].append(np.where(A[:, :, None], W, 0.0))
        stacks["bias"].append(model.biases), stacks["ll"].append(ll)
    stacks = {k: np.array(v) for k, v in stacks.items()}
    assert diag.count == sweeps and diag.level() == 2
    assert np.isfinite(stacks["edge_rb"]).all() and np.any((stacks["edge_rb"] > 0) & (stacks["edge_rb"] < 1))
    host_tests.check_chain_diagnostics(diag, stacks, levels, ("edge", "edge_rb", "weight", "bias", "ll"))
    # the host definition recomputed from the stacks, read-out by read-out
    for what in ("edge", "edge_rb", "weight", "bias"):
        ref = D.batch_means_host(stacks[what], levels)
        tol_m, tol_M2 = host_tests.bounds(sweeps, stacks[what])
        bm = diag._bm(what, range(levels))
        assert np.array_equal(bm.pending, ref.pending)
        assert np.max(np.abs(bm.mean_ - ref.mean_)) <= tol_m and np.max(np.abs(bm.M2 - ref.M2)) <= tol_M2
        for l in (None, 0, 1, 2):
            m = sweeps >> diag.level() if l is None else sweeps >> l
            assert np.max(np.abs(diag.mcse(what, l) ** 2 - ref.mcse(l) ** 2)) <= tol_M2 / ((m - 1) * m)
            assert np.array_equal(np.isnan(diag.ess(what, l)), np.isnan(ref.ess(l)))
    assert np.array_equal(diag.edge_prob, acc.edge_prob)                       # exactly
    assert np.max(np.abs(diag.edge_prob_rb - stacks["edge_rb"].mean(0))) <= host_tests.bounds(sweeps, stacks["edge_rb"])[0]
    gain = diag.rb_gain
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(gain, (diag.mcse("edge") / diag.mcse("edge_rb")) ** 2, equal_nan=True) and gain.shape == (N, N)
    worst = diag.min_ess()
    assert set(worst) == {"edge", "edge_rb", "weight", "bias", "ll"}
    for what, (value, index) in worst.items():
        assert value == np.nanmin(diag.ess(what)) and np.asarray(diag.ess(what))[index] == value
    # a second chain from another seed under R-hat
    other = _model(kind, N=N, B=B, seed=2, **engine_kwargs)
    d2 = other.diagnose(levels=levels)
    for it in range(sweeps):
        other.resample_model()
        d2.collect()
    for what in ("edge", "edge_rb", "weight", "bias", "ll"):
        r = D.rhat([diag, d2], what)
        assert np.array_equal(r, D.rhat([diag._bm(what, (0,)), d2._bm(what, (0,))]), equal_nan=True)
    assert np.all(D.rhat([diag, d2], "bias") > 0)


def test_the_device_accumulators_are_the_host_accumulators():
    """rb=False: the same chain folded by the device and by the NumPy accumulator an engine_factory engine takes"""
    from pyglm_amd.diagnostics import _HostDiag
    model = _model("bernoulli")
    diag = model.diagnose(levels=3, rb=False)
    assert not model.engine.keep_logodds and diag.sections == ("edge", "weight", "bias")
    hostacc = _HostDiag(model, 3, diag.sections)
    stacks = dict(edge=[], weight=[], bias=[])
    for it in range(9):
        model.resample_model()
        diag.collect(ll=0.0)
        hostacc.fold(*model._local_state(), it + 1)
        A = model.adjacency
        stacks["edge"].append(A.astype(float)), stacks["weight"].append(np.where(A[:, :, None], model.weights, 0.0))
        stacks["bias"].append(model.biases)
    for what in diag.sections:
        dev, ref = diag._acc.read(9, what, range(3)), hostacc.read(9, what, range(3))
        assert np.array_equal(dev["pending"], ref["pending"])
        tol_m, tol_M2 = host_tests.bounds(9, np.array(stacks[what]))
        assert np.max(np.abs(dev["mean"] - ref["mean"])) <= tol_m and np.max(np.abs(dev["M2"] - ref["M2"])) <= tol_M2


# ------------------------------------------------------------------------------------------------ shards
def test_shards_give_the_rows_of_the_whole_bit_for_bit():
    import torch
    from oracle import pyglm_oracle as orc
    from pyglm_amd.diagnostics import _DeviceDiag
    from pyglm_amd.engine import GibbsEngine, make_draws, prior_terms
    rng = np.random.default_rng(5)
    N, B, T, levels = 4, 2, 400, 3
    basis = orc.cosine_basis(B, L=20) / 20
    Y = (rng.random((T, N)) < 0.2).astype(float)
    hyp = prior_terms(np.tile(np.eye(B) * 4.0, (N, N, 1, 1)), np.zeros((N, N, B)), np.full(N, 2.0), np.full(N, -1.5))
    rho = np.full((N, N), 0.5)
    rho[1, 2], rho[3, 0] = 0.0, 1.0                      # never proposed: NaN log-odds, the edge's current value
    out = {}
    for n0, n1 in ((0, 4), (0, 2), (2, 4)):
        eng = GibbsEngine(N, B, n0, n1, device="cuda:0")
        eng.add_data(Y, basis=basis)
        eng.keep_logodds = True
        s = _DeviceDiag(eng, levels, ("edge", "edge_rb", "weight", "bias"))
        srng = np.random.default_rng(6)
        a = srng.random((N, N)) < 0.5
        W = srng.standard_normal((N, N, B)) * a[:, :, None]
        b = srng.standard_normal(N) - 1.5
        a, W, b = a[n0:n1], W[n0:n1], b[n0:n1]
        sl = slice(n0, n1)
        for k in range(1, 6):
            perm, u, z = make_draws(1, k, range(n0, n1), N, N * B)
            a, W, b, _ = eng.sweep(a, W, b, rho[sl], hyp[0][sl], hyp[1][sl], hyp[2][sl], hyp[3][sl], hyp[4][sl], perm, u, z, seed=1, sweep=k)
            s.fold(a, W, b, k)
        torch.cuda.synchronize()
        out[(n0, n1)] = ({what: s.read(5, what) for what in s.layout}, s.p.cpu().numpy())
    whole, p_whole = out[(0, 4)]
    assert np.isnan(p_whole).sum() == 0 and set(np.unique(p_whole[1, 2:3])) <= {0.0, 1.0}
    for (n0, n1) in ((0, 2), (2, 4)):
        part, p_part = out[(n0, n1)]
        assert np.array_equal(p_part, p_whole[n0:n1])
        for what in ("edge", "edge_rb", "weight", "bias"):
            for key in ("pending", "mean", "M2"):
                assert np.array_equal(part[what][key], whole[what][key][:, n0:n1]), (what, key)
    assert np.any(whole["edge_rb"]["M2"][0] > 0) and np.any(whole["weight"]["M2"][1] > 0)


# ------------------------------------------------------------------------------------------------ guards
def test_one_fold_per_sweep_with_the_conditionals():
    model = _model("bernoulli")
    diag = model.diagnose(levels=3)
    with pytest.raises(RuntimeError, match="log-odds"):
        diag.collect(ll=0.0)                              # no sweep yet
    assert diag.count == 0
    model.resample_model()
    diag.collect(ll=0.0)
    with pytest.raises(RuntimeError, match="one fold per sweep"):
        diag.collect(ll=0.0)
    assert diag.count == 1
    model.resample_model()
    diag.collect(ll=0.0)
    assert diag.count == 2
    # without the conditionals nothing ties a fold to a sweep
    plain = model.diagnose(levels=3, rb=False)
    plain.collect(ll=0.0), plain.collect(ll=0.0)
    assert plain.count == 2
    # a second diagnostics object allocated after a sweep does not take that sweep's conditionals for its own chain
    late = model.diagnose(levels=3)
    with pytest.raises(RuntimeError, match="one fold per sweep"):
        late.collect(ll=0.0)


def test_memory_is_checked_before_anything_is_allocated():
    import torch
    from pyglm_amd.diagnostics import _DeviceDiag
    from pyglm_amd.engine import GibbsEngine
    probe = GibbsEngine(4, 2, device="cuda:0")
    need = _DeviceDiag.bytes(probe, 3, 15)
    assert need == 3 * 3 * 8 * 4 * (2 * 4 + 2 * 4 + 1) + 4 * 16 + 8 * (16 + 32 + 4)
    tight = GibbsEngine(4, 2, device="cuda:0", mem_budget_bytes=need - 1)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(MemoryError, match=r"chain diagnostics: the accumulators need %d bytes, %d are free" % (need, need - 1)):
        _DeviceDiag(tight, 3, 15)
    assert torch.cuda.memory_allocated() == before
    assert _DeviceDiag(GibbsEngine(4, 2, device="cuda:0", mem_budget_bytes=need), 3, 15).entries == 4 * 17
    from pyglm_amd import models as M
    model = M.SparseBernoulliGLM(4, B=2, seed=1, engine_kwargs=dict(mem_budget_bytes=1000))
    with pytest.raises(MemoryError, match="chain diagnostics"):
        model.diagnose(levels=3)
    with pytest.raises(ValueError, match="levels"):
        _DeviceDiag(probe, 17, 15)
    with pytest.raises(ValueError, match="no such sections"):
        _DeviceDiag(probe, 3, 16)


# ------------------------------------------------------------------------------------------------ non-interference
def test_a_chain_does_not_notice_its_diagnostics():
    plain, watched = _model("bernoulli"), _model("bernoulli")
    diag = watched.diagnose(levels=3)
    for it in range(3):
        plain.resample_model(), watched.resample_model()
        diag.collect()
        assert np.array_equal(plain.adjacency, watched.adjacency) and np.array_equal(plain.weights, watched.weights)
        assert np.array_equal(plain.biases, watched.biases) and np.array_equal(plain.last_loglik_local, watched.last_loglik_local)
    assert plain.engine.logodds is None and watched.engine.logodds is not None
    assert plain.log_likelihood() == watched.log_likelihood()
