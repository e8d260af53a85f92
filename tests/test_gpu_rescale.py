"""The time-rescaling fold on the GPU (pgl_rescale_fold / pgl_rescale_ks, pyglm_amd/csrc/pgl_rescale.hip) against its definition,
rescale.rescale_host and rescale.ks_binned: events on, before and after every wave and segment boundary of the split of time (the shapes
are taken from pgl_rescale_segment_rows()), the parameters and layouts the ABI allows, data sets that add up, a shard with offset pointers,
refused arguments; then model.rescaled_intervals, TimeRescaling.collect() and the statistical pair of tests/test_rescale_host.py through the
device path.

What is compared how:
  hist    exactly -- under a precondition asserted first, on the host's values: no z lies within 1e-9 of an interior edge d / D.  The error
          of a z is at most e^-xi xi (len + 16) 2^-52 (a sequential sum of len positive terms; exp, log1p, expm1 at a few ulp), below 1e-12
          for the lengths here; the margin is 1e3 times that.
  zsum    within M (L_max + 16) 2^-50, L_max the longest interval of the column in bins, M the number of its intervals.
  ks      bit for bit (64-bit integers up to one division); the Welford moments too (the kernel's step is not contracted).

Every call through _fold also checks that nothing was written behind hist, zsum or work."""
import ctypes
import functools

import numpy as np
import pytest

from pyglm_amd import rescale
from pyglm_amd.summary import _welford
from tests import test_rescale_host as host_tests

pytestmark = pytest.mark.gpu

GUARD = 1024                      # elements behind every output, bytes behind `work`: they must survive every call
GARBAGE = 12345                   # what the outputs hold before the first call
SEED, DRAW = 2 ** 40 + 77, 5      # of the uniforms: with SEED the precondition on the margin holds for every case below
MARGIN = 1e-9


@functools.lru_cache(maxsize=None)
def _S():
    from pyglm_amd._lib import load
    return load().pgl_rescale_segment_rows()


@functools.lru_cache(maxsize=None)
def _boundary_series():
    """(psi, bias, Y), T = 3 S + 17, N = 70 -- two column groups, 6 live lanes in the second.  psi + bias is uniform on [-6, 2].  Columns:
    silent; one event; events at rows 0 and T - 1 only (an interval across every segment); every bin; values of {0, 1, 2, 5, -1, NaN};
    periodic columns that place an event on, before and after every wave and segment boundary, at phase 0 and at phase p - 1; Bernoulli(0.05)
    and Bernoulli(0.5) columns; psi = -40 (z rounds to 0) and psi = +40 (z rounds to 1: the top bin)"""
    S = _S()
    T, N = 3 * S + 17, 70
    rng = np.random.default_rng(S)
    bias = rng.uniform(-1.0, 1.0, size=N)
    psi = rng.uniform(-6.0, 2.0, size=(T, N)) - bias
    Y = np.zeros((T, N))
    Y[T // 3, 1] = 1.0
    Y[0, 2] = Y[T - 1, 2] = 1.0
    Y[:, 3] = 1.0
    Y[:, 4] = rng.choice([0.0, 1.0, 2.0, 5.0, -1.0, np.nan], size=T)
    c = 5
    for p in (2, 3, 7, 63, 64, 65, S - 1, S, S + 1, 2 * S + 3):
        for phase in (0, p - 1):
            Y[phase::p, c] = 1.0
            c += 1
    assert c == 25
    Y[:, 25:47] = rng.random((T, 22)) < 0.05
    Y[:, 47:68] = rng.random((T, 21)) < 0.5
    Y[:, 68:] = rng.random((T, 2)) < 0.05
    psi[:, 68], psi[:, 69] = -40.0 - bias[68], 40.0 - bias[69]
    for a in (psi, bias, Y):
        a.setflags(write=False)
    return psi, bias, Y


def _second_set():
    """a second, shorter data set of the same 70 columns: S + 5 rows"""
    S = _S()
    rng = np.random.default_rng(S + 1)
    T, N = S + 5, 70
    return rng.uniform(-6.0, 2.0, size=(T, N)), rng.uniform(-1.0, 1.0, size=N), (rng.random((T, N)) < rng.choice([0.02, 0.2, 0.7], size=N)).astype(float)


def _par_array(N):
    return np.array([1.0, 2.5, 10.0])[np.arange(N) % 3]


def _fold(sets, D, par=1.0, ldn=None, seed=SEED, draw=DRAW, cols=None, first_accumulate=0, start=None):
    """pgl_rescale_fold on the data sets `sets` = [(psi (T, N), bias (N,) or None, Y (T, N), elem0), ...] of one sample, accumulate = 1 after the
    first -> (hist (nloc, D) int64, zsum (nloc, 2)).  The outputs hold GARBAGE before the first call (or `start` = (hist, zsum)).  ldn > N:
    rows of ldn doubles, the cells that are no part of psi and Y hold 1e6 (read, Y would be an event).  cols = (lo, hi): the shard of those
    columns, through pointers offset by lo and neuron0 = lo.  par: qpar0 (a scalar, qpar NULL) or the per-column array."""
    import torch
    from pyglm_amd._lib import call, load, ptr
    N = sets[0][0].shape[1]
    ldn = N if ldn is None else ldn
    lo, hi = cols or (0, N)
    nloc = hi - lo
    hist = torch.full((nloc * D + GUARD,), GARBAGE, dtype=torch.int32, device="cuda")
    zsum = torch.full((nloc * 2 + GUARD,), float(GARBAGE), dtype=torch.float64, device="cuda")
    if start is not None:
        hist[:nloc * D] = torch.from_numpy(start[0].astype(np.int32).ravel()).cuda()
        zsum[:nloc * 2] = torch.from_numpy(np.ascontiguousarray(start[1]).ravel()).cuda()
    qpar, qpar0 = None, 1.0
    if np.ndim(par):
        qpar = torch.from_numpy(np.ascontiguousarray(np.asarray(par, dtype=np.float64)[lo:hi])).cuda()
    else:
        qpar0 = float(par)
    tails = []
    for i, (psi, bias, Y, elem0) in enumerate(sets):
        T = psi.shape[0]
        wp, wy = np.full((T, ldn), 1e6), np.full((T, ldn), 1e6)
        wp[:, :N], wy[:, :N] = psi, Y
        P, Yd = torch.from_numpy(wp).cuda(), torch.from_numpy(wy).cuda()
        bd = None if bias is None else torch.from_numpy(np.array(bias[lo:hi])).cuda()
        nbytes = load().pgl_rescale_work_bytes(nloc, T)
        assert nbytes >= 40 * -(-T // _S()) * nloc and nbytes % 16 == 0
        work = torch.empty(nbytes + GUARD, dtype=torch.uint8, device="cuda")
        work[nbytes:] = 0xA5
        tails.append(work[nbytes:])
        off = lambda t: ctypes.c_void_p(t.data_ptr() + 8 * lo) if T else None
        call("pgl_rescale_fold", off(P), ldn, ptr(bd), off(Yd), T, nloc, ptr(qpar), qpar0, D, seed, draw, lo, elem0, ptr(hist), ptr(zsum),
             1 if i else first_accumulate, ptr(work), None)
        torch.cuda.synchronize()
    assert all(bool((t == 0xA5).all()) for t in tails), "bytes behind `work` were written"
    assert bool((hist[nloc * D:] == GARBAGE).all()), "elements behind `hist` were written"
    assert bool((zsum[nloc * 2:] == float(GARBAGE)).all()), "elements behind `zsum` were written"
    return hist[:nloc * D].cpu().numpy().reshape(nloc, D).astype(np.int64), zsum[:nloc * 2].cpu().numpy().reshape(nloc, 2)


def _host(sets, D, par=1.0, seed=SEED, draw=DRAW):
    """the definition of the same sample -> (hist, zsum, tol (N,) of zsum), after asserting the margin of every z to the interior edges"""
    N = sets[0][0].shape[1]
    hist, zsum, M, Lmax = np.zeros((N, D), dtype=np.int64), np.zeros((N, 2)), np.zeros(N), np.zeros(N)
    for psi, bias, Y, elem0 in sets:
        h, zs, z = rescale.rescale_host(psi + (0.0 if bias is None else bias[None, :]), Y, par, D, seed, draw, 0, elem0)
        hist += h
        zsum += zs
        for j in range(N):
            ev = np.flatnonzero(Y[:, j] > 0)
            if ev.size > 1:
                M[j] += ev.size - 1
                Lmax[j] = max(Lmax[j], np.diff(ev).max())
            f = z[j] * D
            edge = np.rint(f)
            inner = (edge >= 1) & (edge <= D - 1)
            assert not inner.any() or np.abs(f - edge)[inner].min() / D > MARGIN, "a z within the margin of an edge: choose another SEED"
    assert np.array_equal(hist.sum(axis=1), M)
    return hist, zsum, M * (Lmax + 16.0) * 2.0 ** -50


def _assert_same(got, want):
    hist, zsum, tol = want
    assert np.array_equal(got[0], hist), np.argwhere(got[0] != hist)[:5]
    err = np.abs(got[1] - zsum).max(axis=1)
    print("zsum: largest error / tolerance over the columns with intervals: %.3g" % np.max(err[tol > 0] / tol[tol > 0]))
    assert np.all(err <= tol), (np.flatnonzero(err > tol), err[err > tol], tol[err > tol])


def test_across_waves_and_segments_is_the_definition():
    psi, bias, Y = _boundary_series()
    T, D = Y.shape[0], 64
    sets = [(psi, bias, Y, 1000)]
    want = _host(sets, D)
    hist = want[0]
    assert not hist[0].any() and not hist[1].any() and hist[2].sum() == 1 and hist[3].sum() == T - 1
    assert hist[68].sum() > 5 and hist[68, 0] == hist[68].sum()                 # psi = -40: every z rounds to 0
    assert hist[69].sum() > 5 and hist[69, D - 1] >= hist[69].sum() - 8          # psi = +40: z rounds to 1 unless the events are neighbours
    _assert_same(_fold(sets, D), want)


@pytest.mark.parametrize("per_column", [False, True])
@pytest.mark.parametrize("D", [2, 64, 255, 256])
def test_parameters_and_layouts(D, per_column):
    psi, bias, Y = _boundary_series()
    par = _par_array(70) if per_column else 1.0
    sets = [(psi, bias, Y, 0)]
    _assert_same(_fold(sets, D, par=par, ldn=70 + 7), _host(sets, D, par=par))


def test_no_bias_and_a_scalar_parameter():
    psi, bias, Y = _boundary_series()
    sets = [(psi[:300], None, Y[:300], 2 ** 32 - 100)]                           # (the element wraps at 2^32, as the counter word does)
    _assert_same(_fold(sets, 16, par=2.5), _host(sets, 16, par=2.5))


def test_data_sets_add_up_shards_and_repeats_give_the_same_bits():
    psi, bias, Y = _boundary_series()
    T, D, par = Y.shape[0], 64, _par_array(70)
    one, two = (psi, bias, Y, 0), _second_set() + (T,)
    both = _fold([one, two], D, par=par)
    _assert_same(both, _host([one, two], D, par=par))
    a, b = _fold([one], D, par=par), _fold([two], D, par=par)
    assert np.array_equal(both[0], a[0] + b[0]) and np.array_equal(both[1], a[1] + b[1])
    assert not np.array_equal(_fold([two[:3] + (0,)], D, par=par)[0], b[0])     # elem0 is part of the stream
    # accumulate = 1 from the start continues what the outputs hold
    again = _fold([two], D, par=par, first_accumulate=1, start=a)
    assert np.array_equal(again[0], both[0]) and np.array_equal(again[1], both[1])
    # the shard of columns 64 .. 69: offset pointers, neuron0 = 64, nloc = 6
    shard = _fold([one, two], D, par=par, cols=(64, 70))
    assert np.array_equal(shard[0], both[0][64:]) and np.array_equal(shard[1], both[1][64:])
    wide = _fold([one, two], D, par=par, cols=(64, 70), ldn=70 + 9)
    assert np.array_equal(wide[0], shard[0]) and np.array_equal(wide[1], shard[1])
    # the same call again
    repeat = _fold([one, two], D, par=par)
    assert np.array_equal(repeat[0], both[0]) and np.array_equal(repeat[1], both[1])


def test_refused_arguments_leave_the_outputs_untouched_and_no_rows_are_accepted():
    import torch
    from pyglm_amd._lib import load, ptr
    lib = load()
    N, T, D = 5, 40, 8
    Psi = torch.zeros((T, N), dtype=torch.float64, device="cuda")
    Y = torch.ones((T, N), dtype=torch.float64, device="cuda")
    work = torch.zeros(lib.pgl_rescale_work_bytes(N, T) + 16, dtype=torch.uint8, device="cuda")
    hist = torch.full((N, 256), GARBAGE, dtype=torch.int32, device="cuda")
    zsum = torch.full((N, 2), float(GARBAGE), dtype=torch.float64, device="cuda")

    def fold(ldn=N, T=T, nloc=N, D=D, hist=hist, zsum=zsum, accumulate=0, work=ptr(work), Psi=Psi, Y=Y):
        return lib.pgl_rescale_fold(ptr(Psi), ldn, None, ptr(Y), T, nloc, None, 1.0, D, 1, 0, 0, 0, ptr(hist), ptr(zsum), accumulate, work, None)

    odd = ctypes.c_void_p(work.data_ptr() + 4)
    for bad in (dict(D=1), dict(D=257), dict(D=0), dict(ldn=N - 1), dict(nloc=0), dict(T=-1), dict(hist=None), dict(zsum=None), dict(accumulate=2),
                dict(accumulate=-1), dict(work=odd), dict(work=None), dict(Psi=None), dict(Y=None)):
        assert fold(**bad) == 1, bad                              # PGL_ERR_ARG
    torch.cuda.synchronize()
    assert bool((hist == GARBAGE).all()) and bool((zsum == float(GARBAGE)).all())
    assert lib.pgl_rescale_work_bytes(0, 10) == 0 and lib.pgl_rescale_work_bytes(1, -1) == 0 and lib.pgl_rescale_work_bytes(3, 0) == 16
    ks = torch.zeros(N, dtype=torch.float64, device="cuda")
    ex = torch.zeros(N, dtype=torch.int32, device="cuda")
    hs = torch.zeros((N, D), dtype=torch.int64, device="cuda")
    for bad in (dict(D=1), dict(D=257), dict(nloc=0), dict(k=0)):
        a = dict(dict(nloc=N, D=D, k=1), **bad)
        assert lib.pgl_rescale_ks(ptr(hist), a["nloc"], a["D"], 1.36, ptr(ks), ptr(ks), ptr(ks), ptr(ex), ptr(hs), a["k"], None) == 1, bad
    # T = 0: accumulate = 1 changes nothing, accumulate = 0 leaves zeros -- with null Psi, Y and work
    assert fold(T=0, accumulate=1, Psi=None, Y=None, work=None) == 0
    torch.cuda.synchronize()
    assert bool((hist == GARBAGE).all()) and bool((zsum == float(GARBAGE)).all())
    assert fold(T=0, Psi=None, Y=None, work=None) == 0
    torch.cuda.synchronize()
    assert not bool(hist.reshape(-1)[:N * D].any()) and bool((hist.reshape(-1)[N * D:] == GARBAGE).all()) and not bool(zsum.any())
    assert fold() == 0                                            # every bin an event: T - 1 intervals per column
    torch.cuda.synchronize()
    assert bool((hist.reshape(-1)[:N * D].reshape(N, D).sum(dim=1) == T - 1).all())


def test_ks_and_its_moments_bit_for_bit():
    import torch
    from pyglm_amd._lib import call, ptr
    rng = np.random.default_rng(5)
    for N, D in ((70, 64), (3, 2), (300, 256)):
        hists = rng.poisson(rng.choice([0.2, 3.0, 40.0], size=(3, N, 1)), size=(3, N, D)).astype(np.int64)
        hists[:, 1] = 0                                           # M = 0: NaN, and NaN moments from then on
        hists[1, 2] = 0                                           # M = 0 in one sample only
        hists[:, 0] = (hists[:, 0] > 0) * (2 ** 31 - 1) if D == 256 else hists[:, 0]   # counts at the top of int32: the numerator needs 64 bits
        coef = 1.0
        ks = torch.full((N + GUARD,), float(GARBAGE), dtype=torch.float64, device="cuda")
        mean, M2 = torch.zeros(N, dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.float64, device="cuda")
        ex = torch.zeros(N, dtype=torch.int32, device="cuda")
        hs = torch.zeros((N, D), dtype=torch.int64, device="cuda")
        rmean, rM2, rex = np.zeros(N), np.zeros(N), np.zeros(N, dtype=np.int64)
        for k in range(1, 4):
            h = hists[k - 1]
            call("pgl_rescale_ks", ptr(torch.from_numpy(h.astype(np.int32)).cuda()), N, D, coef, ptr(ks), ptr(mean), ptr(M2), ptr(ex), ptr(hs), k, None)
            torch.cuda.synchronize()
            want = rescale.ks_binned(h)
            with np.errstate(invalid="ignore"):
                _welford(rmean, rM2, want, float(k))
                rex += want > rescale.band(coef, h.sum(axis=1))
            assert np.isnan(want[1]) and np.array_equal(ks[:N].cpu().numpy(), want, equal_nan=True)
            assert np.array_equal(mean.cpu().numpy(), rmean, equal_nan=True) and np.array_equal(M2.cpu().numpy(), rM2, equal_nan=True)
            assert np.array_equal(ex.cpu().numpy(), rex) and np.array_equal(hs.cpu().numpy(), hists[:k].sum(axis=0))
        assert bool((ks[N:] == float(GARBAGE)).all()) and np.isnan(rmean[2])
        if N == 70:
            assert 0 < rex.sum() < 3 * N and np.isfinite(rmean[3:]).all()


# ---- the model
@functools.lru_cache(maxsize=None)
def _model_case(obs):
    """N = 8, B = 2, data sets of 2 000 and 300 bins: Bernoulli (0), negative binomial (1) or mixed (4), as tests/test_gpu_summary.py builds them"""
    from tests.test_gpu_summary import _model
    return _model(obs, 8, B=2, Ts=(2000, 300))


def _assert_readouts(dev, host, zsum_tol):
    assert dev.count == host.count
    assert np.array_equal(dev.hist_last, host.hist_last) and np.array_equal(dev.hist, host.hist) and np.array_equal(dev.intervals, host.intervals)
    for name in ("ks_last", "ks_mean", "ks_std", "exceed_fraction", "band"):              # bit for bit, given equal histograms
        assert np.array_equal(getattr(dev, name), getattr(host, name), equal_nan=True), name
    assert np.array_equal(dev.failing(), host.failing())
    assert np.all(np.abs(dev.zsum_last - host.zsum_last).max(axis=1) <= zsum_tol)


def _zsum_tol(Ys):
    """M (L_max + 16) 2^-50 per neuron over the data sets Ys"""
    ev = [[np.flatnonzero(Y[:, n] > 0) for Y in Ys] for n in range(Ys[0].shape[1])]
    M = np.array([sum(max(e.size - 1, 0) for e in col) for col in ev], dtype=float)
    L = np.array([max([np.diff(e).max() for e in col if e.size > 1] or [0]) for col in ev], dtype=float)
    return M * (L + 16.0) * 2.0 ** -50


@pytest.mark.parametrize("obs", [0, 1, 4])
def test_the_model_on_the_device_equals_the_host_class(obs):
    model, Ys = _model_case(obs)
    dev = model.time_rescaling(bins=32, seed=3, coef=1.0)
    host = rescale.TimeRescaling(model, bins=32, seed=3, coef=1.0, host=True)
    assert type(dev._acc).__name__ == "_DeviceFold" and type(host._acc).__name__ == "_HostFold"
    tol = _zsum_tol(Ys)
    for _ in range(3):
        model.resample_model()
        dev.collect()
        host.collect()
        _assert_readouts(dev, host, tol)
    assert dev.count == 3 and dev.intervals.min() > 100 and np.all(dev.hist.sum(axis=1) == 3 * dev.intervals)
    # the one-off read-out of a data set at the current state: both paths, and sample 1 of a test on that data set alone
    for data in (0, 1):
        d, h = model.rescaled_intervals(data=data, bins=32, seed=3, gpu=True), model.rescaled_intervals(data=data, bins=32, seed=3, gpu=False)
        assert d[0].dtype == np.int64 and np.array_equal(d[0], h[0]) and np.all(np.abs(d[1] - h[1]).max(axis=1) <= _zsum_tol([Ys[data]]))
    dev.reset()
    dev.collect()
    both = model.rescaled_intervals(0, 32, 3)[0] + model.rescaled_intervals(1, 32, 3)[0]
    assert dev.count == 1 and np.array_equal(dev.hist, both) and np.array_equal(dev.ks_mean, rescale.ks_binned(both))


def test_heldout_recordings():
    model, Ys = _model_case(0)
    held = [Ys[1][:250], Ys[0][:700]]
    dev = model.time_rescaling(bins=16, seed=4, datas=held)
    host = rescale.TimeRescaling(model, bins=16, seed=4, datas=held, host=True)
    assert dev._eng is not model.engine and type(dev._acc).__name__ == "_DeviceFold"
    for _ in range(2):
        model.resample_model()
        dev.collect()
        host.collect()
    _assert_readouts(dev, host, _zsum_tol(held))
    assert np.array_equal(dev.intervals, [(held[0][:, n] > 0).sum() + (held[1][:, n] > 0).sum() - 2 for n in range(8)])


def test_memory_is_checked_before_anything_is_allocated(monkeypatch):
    model, _ = _model_case(0)
    monkeypatch.setattr(type(model.engine), "_free_bytes", lambda self: 1000)
    with pytest.raises(MemoryError, match="time rescaling"):
        model.time_rescaling()


def test_the_statistical_pair_on_the_device():
    model = host_tests.statistical_model(engine_factory=None)
    model.add_data(np.array(host_tests.statistical_data(gpu=True)))            # the recording of the host test, simulated on the device
    dev =host_tests.statistical_verdicts(model)
    ref = host_tests.statistical_verdicts(model, host=True)
    print("sqrt(M) ks at the generating state", np.sqrt(dev[0][1]) * dev[0][0])
    print("sqrt(M) ks with the biases shifted", np.sqrt(dev[1][1]) * dev[1][0])
    host_tests.check_verdicts(dev)
    for (ks, M, ex), (ks_h, M_h, ex_h) in zip(dev, ref):
        assert np.array_equal(M, M_h) and np.array_equal(ex, ex_h) and np.array_equal(ks > 1.63 / np.sqrt(M), ks_h > 1.63 / np.sqrt(M_h))
