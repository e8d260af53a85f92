"""The inter-spike-interval fold on the GPU (pgl_isi_fold, pyglm_amd/csrc/pgl_isi.hip) against its definition, simulate.isi_host, and the
definition of the carry `since`, integer for integer: events on, before and after every wave and workgroup boundary of the split of time
(the shapes are taken from pgl_isi_segment_rows()), chunks that compose, the layouts the ABI allows, refused arguments, the two chunk shapes
of production; then model.simulate(isi=D), model.isi_histogram and PredictiveCheck(isi=D) against the NumPy path.

Every call through _fold also checks that nothing was written behind work, hist, moments or since."""
import functools

import numpy as np
import pytest

from pyglm_amd import simulate
from tests.test_gpu_xcorr import _model

pytestmark = pytest.mark.gpu

GUARD = 1024                      # elements behind every output, bytes behind `work`: they must survive every call
GARBAGE = 12345                   # what the outputs hold before the first call


@functools.lru_cache(maxsize=None)
def _bt():
    from pyglm_amd._lib import load
    return load().pgl_isi_segment_rows()


def _since(Y):
    """the definition of the carry for a series Y (T, N)"""
    T = Y.shape[0]
    ev = [np.flatnonzero(Y[:, n] > 0) for n in range(Y.shape[1])]
    return np.array([T - 1 - e[-1] if e.size else -1 for e in ev])


def _reference(Y, D, done):
    """(hist (R, N, D), moments (R, N, 3), since (R, N)) of the first `done` rows of Y (R, T, N), by the definition"""
    parts = [simulate.isi_host(Y[r, :done], D) for r in range(Y.shape[0])]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([_since(Y[r, :done]) for r in range(Y.shape[0])])


def _fold(Y, D, cuts=None, ldy=None, behind=0, first_accumulate=0):
    """pgl_isi_fold on Y (R, T, N), as one call or cut into the chunks `cuts` (accumulate = 1 after the first) -> the list of (hist, moments,
    since) after every call, as NumPy arrays.  The outputs hold GARBAGE before the first call.  ldy > N: rows of ldy doubles; behind: every
    replicate block is that many rows longer than T; the cells that are no part of Y hold 1e6 (an event, if read)."""
    import torch
    from pyglm_amd._lib import call, load, ptr
    R, T, N = Y.shape
    ldy = N if ldy is None else ldy
    wide = np.full((R, T + behind, ldy), 1e6)
    wide[:, :T, :N] = Y
    Y_d = torch.from_numpy(wide).cuda()
    strideY = (T + behind) * ldy
    hist = torch.full((R * N * D + GUARD,), GARBAGE, dtype=torch.int32, device="cuda")
    moments = torch.full((R * N * 3 + GUARD,), GARBAGE, dtype=torch.int64, device="cuda")
    since = torch.full((R * N + GUARD,), GARBAGE, dtype=torch.int32, device="cuda")
    done, works, states = 0, [], []
    for k, rows in enumerate(cuts if cuts is not None else [T]):
        nbytes = load().pgl_isi_work_bytes(N, R, rows)
        assert nbytes >= 20 * -(-rows // _bt()) * R * N
        work = torch.empty(nbytes + GUARD, dtype=torch.uint8, device="cuda")
        work[nbytes:] = 0xA5
        works.append(work[nbytes:])
        call("pgl_isi_fold", ptr(Y_d[0, done:]) if done < T + behind else ptr(Y_d), ldy, strideY, rows, N, R, D, ptr(hist), ptr(moments), ptr(since),
             1 if k else first_accumulate, ptr(work), None)
        done += rows
        torch.cuda.synchronize()
        states.append((hist[:R * N * D].cpu().numpy().reshape(R, N, D).astype(np.int64), moments[:R * N * 3].cpu().numpy().reshape(R, N, 3),
                       since[:R * N].cpu().numpy().reshape(R, N).astype(np.int64)))
    assert all(bool((tail == 0xA5).all()) for tail in works), "bytes behind `work` were written"
    for name, out, n in (("hist", hist, R * N * D), ("moments", moments, R * N * 3), ("since", since, R * N)):
        assert bool((out[n:] == GARBAGE).all()), "elements behind `%s` were written" % name
    return states


def _assert_state(state, ref):
    for got, want, name in zip(state, ref, ("hist", "moments", "since")):
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])


@functools.lru_cache(maxsize=None)
def _boundary_series():
    """(1, T, 70), T = 3 Bt + 17: silent; one event; events at rows 0 and T - 1 only (an interval across two empty segments); every bin; values
    of {0, 1, 2, 5, -1, NaN}; periodic columns that place an event on, before and after every wave and workgroup boundary, at phase 0 and at
    phase p - 1; Bernoulli(0.05) and Bernoulli(0.5) columns"""
    Bt = _bt()
    T, N = 3 * Bt + 17, 70
    rng = np.random.default_rng(Bt)
    Y = np.zeros((T, N))
    Y[T // 3, 1] = 1.0
    Y[0, 2] = Y[T - 1, 2] = 1.0
    Y[:, 3] = 1.0
    Y[:, 4] = rng.choice([0.0, 1.0, 2.0, 5.0, -1.0, np.nan], size=T)
    c = 5
    for p in (2, 3, 7, 63, 64, 65, Bt - 1, Bt, Bt + 1, 2 * Bt + 3):
        for phase in (0, p - 1):
            Y[phase::p, c] = 1.0
            c += 1
    assert c == 25
    Y[:, 25:48] = rng.random((T, 23)) < 0.05
    Y[:, 48:] = rng.random((T, N - 48)) < 0.5
    Y = Y[None]
    Y.setflags(write=False)
    return Y


def test_across_segments_is_the_definition():
    Y = _boundary_series()
    T, D = Y.shape[1], 8
    ref = _reference(Y, D, T)
    assert ref[0][0, 2, D - 1] == 1 and list(ref[1][0, 2]) == [1, T - 1, (T - 1) ** 2] and ref[0][0, 3, 0] == T - 1
    state, = _fold(Y, D)
    _assert_state(state, ref)


def test_chunks_compose_and_the_carry_is_the_definition():
    Y = _boundary_series()
    Bt, T, D = _bt(), Y.shape[1], 8
    cuts = [1, Bt - 1, 2 * Bt + 1]
    cuts.append(T - sum(cuts))
    assert all(r > 0 for r in cuts)
    done = 0
    for rows, state in zip(cuts, _fold(Y, D, cuts=cuts)):
        done += rows
        _assert_state(state, _reference(Y, D, done))
    assert done == T


def test_chunks_of_one_row_and_a_chunk_without_an_event():
    Yc = _boundary_series()
    Bt, D = _bt(), 8
    Y = Yc[:, :70 + Bt + 40].copy()
    Y[:, 70:70 + Bt + 5] = 0.0                                  # the chunk after the 70 single rows has no event in any column
    cuts = [1] * 70 + [Bt + 5, 35]
    states = _fold(Y, D, cuts=cuts)
    done = 0
    for rows, state in zip(cuts, states):
        done += rows
        _assert_state(state, _reference(Y, D, done))
    assert done == Y.shape[1] and states[-1][1][0, :, 0].sum() > states[69][1][0, :, 0].sum()


@pytest.mark.parametrize("N", [1, 64, 65, 129])
@pytest.mark.parametrize("D", [2, 3, 255, 256])
def test_layouts(N, D):
    # R = 3, rows of N + 7 doubles, replicate blocks 5 rows longer than T, 1e6 in every unused cell: read, it would be an event
    Bt = _bt()
    R, T = 3, Bt + Bt // 2 + 3
    rng = np.random.default_rng(N + D)
    Y = (rng.random((R, T, N)) < rng.choice([0.003, 0.05, 0.6], size=(R, 1, N))).astype(np.float64)
    ref = _reference(Y, D, T)
    state, = _fold(Y, D, ldy=N + 7, behind=5)                   # accumulate = 0 over GARBAGE
    _assert_state(state, ref)
    cuts = [Bt // 2, 1, T - Bt // 2 - 1]
    _assert_state(_fold(Y, D, cuts=cuts, ldy=N + 7, behind=5)[-1], ref)


def test_no_rows():
    Bt = _bt()
    Y = (np.random.default_rng(7).random((2, Bt + 9, 5)) < 0.2).astype(np.float64)
    zero, = _fold(Y, 8, cuts=[0])                               # accumulate = 0: only zeroes
    assert not zero[0].any() and not zero[1].any() and np.all(zero[2] == -1)
    states = _fold(Y, 8, cuts=[0, Bt + 9, 0])                   # accumulate = 1: changes nothing
    _assert_state(states[1], _reference(Y, 8, Bt + 9))
    _assert_state(states[2], states[1])


def test_refused_arguments_leave_the_outputs_untouched():
    import torch
    from pyglm_amd._lib import load, ptr
    lib = load()
    N, R, T, D = 5, 2, 40, 8
    Y = torch.ones((R, T, N), dtype=torch.float64, device="cuda")
    work = torch.zeros(lib.pgl_isi_work_bytes(N, R, T), dtype=torch.uint8, device="cuda")
    hist = torch.full((R, N, 256), GARBAGE, dtype=torch.int32, device="cuda")
    moments = torch.full((R, N, 3), GARBAGE, dtype=torch.int64, device="cuda")
    since = torch.full((R, N), GARBAGE, dtype=torch.int32, device="cuda")
    good = dict(ldy=N, rows=T, N=N, R=R, D=D)
    for bad in (dict(D=1), dict(D=257), dict(D=0), dict(ldy=N - 1), dict(N=0), dict(R=0), dict(rows=-1)):
        a = dict(good, **bad)
        for accumulate in (0, 1):
            rc = lib.pgl_isi_fold(ptr(Y), a["ldy"], T * N, a["rows"], a["N"], a["R"], a["D"], ptr(hist), ptr(moments), ptr(since), accumulate, ptr(work),
                                  None)
            assert rc == 1, bad                                 # PGL_ERR_ARG
    torch.cuda.synchronize()
    assert bool((hist == GARBAGE).all()) and bool((moments == GARBAGE).all()) and bool((since == GARBAGE).all())
    assert lib.pgl_isi_work_bytes(0, 1, 10) == 0 and lib.pgl_isi_work_bytes(1, 1, -1) == 0


@pytest.mark.parametrize("R,N,rows", [(8, 1024, 204), (1, 1024, 1638)])
def test_the_production_chunk_shapes(R, N, rows):
    Y = (np.random.default_rng(rows).random((R, rows, N)) < 0.08).astype(np.float64)
    state, = _fold(Y, 64)
    _assert_state(state, _reference(Y, 64, rows))


# ---- the model
MODELS = [(20, 3, 30, ("bernoulli",), 3, 700), (12, 3, 30, ("bernoulli", "binomial", "negbin"), 3, 700)]      # (N, B, L, kinds, R, T)


@functools.lru_cache(maxsize=None)
def _model_case(case):
    """the model of MODELS[case] and its simulation on the NumPy path, interval statistics and lagged products included"""
    N, B, L, kinds, R, T = MODELS[case]
    model = _model(N, B, L, kinds, seed=N + R)
    host = model.simulate(T, replicates=R, seed=600 + N, gpu=False, isi=16, lags=5)
    for a in (host.Y, host.isi, host.isi_moments, host.lagged):
        a.setflags(write=False)
    return model, host


@pytest.mark.parametrize("chunk", [None, 37])
@pytest.mark.parametrize("case", range(len(MODELS)))
def test_simulate_on_the_device_folds_the_intervals_of_its_paths(case, chunk, monkeypatch):
    N, B, L, kinds, R, T = MODELS[case]
    model, host = _model_case(case)
    for r in range(R):
        h, m = simulate.isi_host(host.Y[r], 16)
        assert np.array_equal(host.isi[r], h) and np.array_equal(host.isi_moments[r], m)
    assert host.isi_moments[..., 0].min() > 0
    if chunk:
        assert T % chunk != 0
        monkeypatch.setattr(simulate, "chunk_bins", lambda N, B, R=1: chunk)
    for keep in (True, False):
        for lags in (0, 5):
            sim = model.simulate(T, replicates=R, seed=600 + N, gpu=True, isi=16, lags=lags, keep_paths=keep)
            assert sim.isi.dtype == sim.isi_moments.dtype == np.int64 and sim.isi.shape == (R, N, 16)
            assert np.array_equal(sim.isi, host.isi) and np.array_equal(sim.isi_moments, host.isi_moments)
            assert np.array_equal(sim.sum, host.sum) and (sim.Y is None or np.array_equal(sim.Y, host.Y))
            if lags:
                assert np.array_equal(sim.lagged, host.lagged)
    assert model.simulate(T, replicates=R, seed=600 + N, gpu=True).isi is None


@pytest.mark.parametrize("case", range(len(MODELS)))
def test_isi_histogram_of_a_data_set(case):
    model, host = _model_case(case)
    model.data_list.append((None, np.array(host.Y[0])))
    try:
        d, h = model.isi_histogram(data=-1, bins=16, gpu=True), model.isi_histogram(data=-1, bins=16, gpu=False)
    finally:
        model.data_list.pop()
    assert d[0].dtype == d[1].dtype == np.int64
    assert np.array_equal(d[0], h[0]) and np.array_equal(d[1], h[1]) and np.array_equal(d[0], host.isi[0]) and d[0].sum() > 0


@pytest.mark.parametrize("kinds", [("bernoulli",), ("bernoulli", "binomial", "negbin")])
def test_predictive_check_of_the_intervals_matches_the_host_path(kinds):
    N, R, D = 12, 4, 16
    model = _model(N, 3, 30, kinds, seed=71)
    model.add_data(model.simulate(600, seed=72, gpu=False).Y[0])
    out = []
    for gpu in (True, False):
        ppc = model.predictive_check(replicates=R, seed=73, gpu=gpu, isi=D)
        for _ in range(3):
            ppc.collect()
        out.append(ppc)
    d, h = out
    for stat in ("isi", "cv"):
        assert np.array_equal(d.observed[stat], h.observed[stat], equal_nan=True)
    for got, want in zip(d._isi_state()[:3], h._isi_state()[:3]):
        assert np.array_equal(got, want)
    p = d.pvalue("isi")
    assert p.shape == (N, D) and np.array_equal(p, h.pvalue("isi"), equal_nan=True) and np.nanmin(p) >= 2.0 / 13.0
    np.testing.assert_allclose(d.isi_mean, h.isi_mean, rtol=0, atol=1e-12)
    np.testing.assert_allclose(d.isi_std, h.isi_std, rtol=0, atol=1e-12)
    assert np.array_equal(d.cvs, h.cvs, equal_nan=True)
    for stat in ("cv", "rate", "fano"):
        assert np.array_equal(d.pvalue(stat), h.pvalue(stat), equal_nan=True)
