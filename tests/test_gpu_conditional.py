"""model.conditional_simulate() / model.conditional_check() on the GPU (pgl_conditional_simulate) against the NumPy path of the same law
(pyglm_amd/simulate.py, conditional_host) given the SAME base: the same bits for the spike and count models at every shape of the kernel
(every split of the lanes, ring / basis / Wff in LDS or not), replicate independence, chunking, windows, the reduction to simulate(), the cap
and the argument checks.  Every case stays below 1e7 draws, as in test_gpu_simulate.py: bit-equality is then the honest condition; Gaussian
paths and everything formed from psi are held to that file's rtol = 1e-10, atol = 1e-12."""
import ctypes

import numpy as np
import pytest

from pyglm_amd import _lib, simulate
from pyglm_amd._lib import PglError
from tests.test_gpu_simulate import _model

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-10, atol=1e-12)


def _recorded(N, B, L, kinds, T, seed, w_scale=None, gpu=False):
    """a model as test_gpu_simulate builds them, with a seeded path of its own simulate() as data set 0"""
    model = _model(N, B, L, kinds, seed=seed, w_scale=w_scale)
    Y = model.simulate(T, seed=seed + 1, gpu=gpu).Y[0]
    model.add_data(Y)
    return model, Y


def _law_inputs(model, Y, free, start):
    """Wff, kind, par and the history of the law, read from the model's state here, in NumPy"""
    A, W, _ = model._adopt_state()
    N, B, L = model.N, model.B, model.basis.shape[0]
    Wm = (W * A[:, :, None]).reshape(N, N * B)
    cols = (np.asarray(free)[:, None] * B + np.arange(B)).ravel()
    kind, par = simulate.observation_kinds([model.regressions[n] for n in free])
    hist = np.zeros((L, len(free)))
    h = Y[max(0, start - L):start][:, free]
    hist[L - len(h):] = h
    return Wm[free][:, cols], kind, par, hist


def _host(model, Y, d, R, seed, rep0=0, bins=None, **kw):
    """the NumPy law on the device result's own base (its first `bins` rows)"""
    Wff, kind, par, hist = _law_inputs(model, Y, d.free, d.t0)
    base = d.base if bins is None else d.base[:bins]
    return simulate.conditional_simulate(Wff, base, np.asarray(model.basis, dtype=np.float64), kind, par, d.free, R, seed, rep0, hist, d.t0, True,
                                         False, None, **kw)


def _assert_same(d, h, exact=True, bins=None):
    cut = (lambda v: v) if bins is None else (lambda v: v[:, :bins])
    names = ("Y", "sum", "sumsq", "history") if bins is None else ("Y",)
    for name in names:
        a, b = cut(getattr(d, name)) if name == "Y" else getattr(d, name), getattr(h, name)
        if exact:
            assert np.array_equal(a, b), name
        else:
            np.testing.assert_allclose(a, b, err_msg=name, **TOL)


def _pick(N, F, seed):
    return np.sort(np.random.default_rng(seed).choice(N, F, replace=False))


CASES = [
    # N, B, L, kinds, free, R, T
    (3, 1, 1, ("bernoulli",), [0, 1], 2, 500),                                      # smallest basis and ring
    (4, 1, 100, ("bernoulli",), [2], 1, 3000),                                      # F = 1: self-coupling only, 64 lanes on one row
    (12, 3, 30, ("bernoulli", "negbin", "binomial"), [0, 5, 11], 5, 2000),          # mixed models, gaps in `free`
    (80, 5, 100, ("bernoulli", "negbin"), 64, 3, 1000),                             # the last F with four lanes per neuron; Wff streamed
    (80, 5, 100, ("bernoulli", "negbin"), 65, 2, 1000),                             # one neuron more: two lanes per neuron
    (40, 5, 400, ("bernoulli", "negbin"), 33, 8, 300),                              # ring beyond its LDS cap, in global memory
    (48, 5, 100, ("bernoulli", "negbin"), 40, 2, 500),                              # ring, basis and Wff all in LDS: a request of 102 KB, beyond 64 KiB
    (300, 2, 10, ("bernoulli", "binomial"), 256, 2, 300),                           # F at its maximum: a lane per neuron, Wff (1 MB) streamed
    (100, 2, 100, ("bernoulli", "negbin"), 100, 2, 300),                            # ring in global memory AND Wff streamed
    (6, 5, 500, ("bernoulli", "negbin"), [0, 2, 3, 5], 2, 700),                     # a basis beyond its LDS cap, read from global memory
]


@pytest.mark.parametrize("N,B,L,kinds,free,R,T", CASES)
def test_device_is_the_host_law_on_the_same_base(N, B, L, kinds, free, R, T):
    free = _pick(N, free, seed=N) if isinstance(free, int) else np.asarray(free)
    assert R * T * len(free) <= 10 ** 7
    model, Y = _recorded(N, B, L, kinds, T, seed=N + R)
    d = model.conditional_simulate(free, replicates=R, seed=2000 + N, gpu=True)
    h = _host(model, Y, d, R, 2000 + N)
    _assert_same(d, h)
    assert d.Y.shape == (R, T, len(free)) and d.Y.dtype == np.float64 and (d.t0, d.t1) == (0, T)
    assert 0 < d.Y.sum() and np.all(d.Y >= 0) and np.all(d.Y == np.floor(d.Y))
    assert len(np.unique(d.sum, axis=0)) == R                  # the replicates differ
    assert np.array_equal(d.sum, d.Y.sum(axis=1)) and np.array_equal(d.sumsq, (d.Y ** 2).sum(axis=1))
    np.testing.assert_array_equal(d.rate(), h.rate())
    np.testing.assert_array_equal(d.fano(), h.fano())


def test_gaussian_parity():
    N, B, L, R, T = 96, 3, 40, 4, 1000
    model, Y = _recorded(N, B, L, ("gaussian",), T, seed=31, w_scale=0.5 / np.sqrt(N * B))
    free = _pick(N, 20, seed=3)
    d = model.conditional_simulate(free, replicates=R, seed=32, gpu=True)
    _assert_same(d, _host(model, Y, d, R, 32), exact=False)
    assert np.std(d.Y) > 0.1


@pytest.fixture(scope="module")
def mixed():
    """N = 64 of three count models with a recording of 600 bins; the tests below leave its state as they found it"""
    model, Y = _recorded(64, 5, 100, ("bernoulli", "negbin", "binomial"), 600, seed=5)
    return model, Y, _pick(64, 11, seed=1)


def test_one_call_of_five_replicates_is_five_calls_of_one(mixed):
    model, Y, free = mixed
    d = model.conditional_simulate(free, replicates=5, seed=9, first_replicate=10, gpu=True)
    for r in range(5):
        one = model.conditional_simulate(free, replicates=1, seed=9, first_replicate=10 + r, gpu=True)
        assert np.array_equal(one.Y[0], d.Y[r]) and np.array_equal(one.sum[0], d.sum[r]) and np.array_equal(one.history[0], d.history[r])
    other = model.conditional_simulate(free, replicates=1, seed=10, first_replicate=10, gpu=True)
    assert not np.array_equal(other.Y[0], d.Y[0])


def test_chunks_that_do_not_divide_T_and_windows(mixed):
    model, Y, free = mixed
    L = model.basis.shape[0]
    whole = model.conditional_simulate(free, replicates=3, seed=8, start=150, stop=391, gpu=True)
    assert (whole.t0, whole.t1) == (150, 391) and whole.Y.shape == (3, 241, 11)
    Wff, kind, par, hist = _law_inputs(model, Y, free, 150)
    assert np.array_equal(hist, Y[150 - L:150][:, free])
    args = (Wff, whole.base, np.asarray(model.basis, dtype=np.float64), kind, par, free, 3, 8, 0, hist, 150, True)
    cut = simulate.conditional_simulate(*args, True, None, chunk=7)           # 34 launches of 7 bins and one of 3
    _assert_same(cut, whole)
    _assert_same(cut, simulate.conditional_simulate(*args, False, None))
    # the window's base is rows start:stop of the whole recording's, and nothing else enters
    full = model.conditional_simulate(free, replicates=1, seed=8, gpu=True, keep_paths=False)
    assert np.array_equal(whole.base, full.base[150:391])
    # the activations the device hands out are the host's, chunked or not
    p_cut = simulate.conditional_simulate(*args, True, None, chunk=50, want_psi=True).psi
    p_host = simulate.conditional_simulate(*args, False, None, want_psi=True).psi
    np.testing.assert_allclose(p_cut, p_host, **TOL)


def test_paths_carry_the_recording_and_sums_need_no_paths(mixed):
    model, Y, free = mixed
    kept = model.conditional_simulate(free, replicates=3, seed=12, start=40, gpu=True)
    bare = model.conditional_simulate(free, replicates=3, seed=12, start=40, gpu=True, keep_paths=False)
    assert bare.Y is None and bare.sum.shape == bare.sumsq.shape == (3, 11)
    assert np.array_equal(bare.sum, kept.sum) and np.array_equal(bare.sumsq, kept.sumsq) and np.array_equal(bare.history, kept.history)
    assert np.array_equal(kept.history, kept.Y[:, -model.basis.shape[0]:])
    clamped = np.setdiff1d(np.arange(64), free)
    for r in range(3):
        p = kept.paths(r)
        assert p.shape == (560, 64) and np.array_equal(p[:, clamped], Y[40:][:, clamped]) and np.array_equal(p[:, free], kept.Y[r])


def test_base_is_the_bias_and_the_clamped_columns(mixed):
    model, Y, free = mixed
    A, W, b = model._adopt_state()
    X = np.asarray(model.data_list[0][0])
    clamped = np.setdiff1d(np.arange(64), free)
    Wm = A[:, :, None] * W
    want = b[free, 0] + np.einsum("tmb,jmb->tj", X[:, clamped], Wm[free][:, clamped])
    d = model.conditional_simulate(free, gpu=True, keep_paths=False)
    np.testing.assert_allclose(d.base, want, **TOL)
    assert np.array_equal(d.free, free)


@pytest.mark.parametrize("gpu", [True, False])
def test_every_neuron_free_is_simulate(gpu):
    N, T, R = 12, 800, 3
    model, _ = _recorded(N, 3, 30, ("bernoulli", "negbin", "binomial"), T, seed=17)
    c = model.conditional_simulate(np.arange(N), replicates=R, seed=21, first_replicate=4, gpu=gpu)
    s = model.simulate(T, replicates=R, seed=21, first_replicate=4, gpu=False)
    for name in ("Y", "sum", "sumsq", "history"):
        assert np.array_equal(getattr(c, name), getattr(s, name)), name


def test_conditional_check_on_the_device_is_the_host_fold(mixed):
    model, Y, free = mixed
    A, W, b = model._adopt_state()
    keep = W.copy(), b.copy()
    dev = model.conditional_check(free, replicates=3, seed=4, start=25, stop=500, gpu=True)
    host = model.conditional_check(free, replicates=3, seed=4, start=25, stop=500, gpu=False)
    rng = np.random.default_rng(0)
    try:
        for _ in range(3):
            dev.collect()
            host.collect()
            W *= 1.0 + 0.05 * rng.standard_normal(W.shape)        # another state for the next sample
            b += 0.05 * rng.standard_normal(b.shape)
    finally:
        W[...], b[...] = keep
    assert dev.count == host.count == 9 and dev.calls == 3
    assert not isinstance(dev._acc[0], np.ndarray) and isinstance(host._acc[0], np.ndarray)      # each folded where it ran
    np.testing.assert_allclose(dev.rate_mean, host.rate_mean, **TOL)
    np.testing.assert_allclose(dev.rate_std, host.rate_std, **TOL)
    sd, sh = dev.log_score(), host.log_score()
    assert sd["per_bin"].shape == (475, 11) and sd["per_neuron"].shape == (11,)
    for key in ("total", "per_neuron", "per_bin"):
        np.testing.assert_allclose(sd[key], sh[key], err_msg=key, **TOL)
    assert dev.rate_std.max() > 0


def test_an_exploding_free_neuron_names_the_global_index():
    model, Y = _recorded(6, 1, 4, ("negbin",), 40, seed=2)
    _, _, b = model._adopt_state()
    keep = b[4, 0]
    b[4, 0] = 40.0
    with pytest.raises(PglError, match=r"neuron 4 in replicate 6 at bin 3 "):
        model.conditional_simulate([1, 4], replicates=1, first_replicate=6, seed=1, start=3, gpu=True)
    b[4, 0] = keep
    d = model.conditional_simulate([1, 4], replicates=2, first_replicate=6, seed=1, start=3, gpu=True)
    _assert_same(d, _host(model, Y, d, 2, 1, rep0=6))


def test_argument_errors():
    model, _ = _recorded(300, 1, 4, ("bernoulli",), 20, seed=1)
    with pytest.raises(ValueError, match="257 free neurons"):
        model.conditional_simulate(np.arange(257), gpu=True)
    with pytest.raises(ValueError, match="neuron 5 is listed more than once"):
        model.conditional_simulate([3, 5, 5], gpu=True)
    with pytest.raises(ValueError, match="index 300 is outside"):
        model.conditional_simulate([0, 300], gpu=True)
    with pytest.raises(ValueError, match="empty"):
        model.conditional_simulate([], gpu=True)
    with pytest.raises(ValueError, match=r"window \[5, 21\)"):
        model.conditional_simulate([0], start=5, stop=21, gpu=True)
    with pytest.raises(ValueError, match="holds at most 8192"):
        simulate.conditional_simulate(np.zeros((256, 256 * 33)), np.zeros((4, 256)), np.ones((2, 33)), np.zeros(256), np.zeros(256), np.arange(256),
                                      1, 0, 0, np.zeros((2, 256)), 0, True, True, None)
    # the C entry refuses F = 0, Tc = 0, F beyond the maximum and null pointers, and writes nothing
    import torch
    lib = _lib.load()
    assert lib.pgl_conditional_max_free() == simulate.PGL_COND_MAX_FREE == 256
    f64 = dict(dtype=torch.float64, device="cuda")
    F, B, L, Tc = 2, 1, 3, 4
    t = dict(Wff=torch.zeros(F, F * B, **f64), base=torch.zeros(Tc, F, **f64), basis=torch.ones(L, B, **f64), kind=torch.zeros(F, dtype=torch.int32, device="cuda"),
             par=torch.zeros(F, **f64), neuron=torch.arange(F, dtype=torch.int32, device="cuda"), ring=torch.zeros(1, L, F, **f64),
             sum=torch.full((1, F), 7.0, **f64), sumsq=torch.full((1, F), 7.0, **f64), status=torch.zeros(4, dtype=torch.int32, device="cuda"))

    def entry(F=F, Tc=Tc, **null):
        p = {k: (None if k in null else _lib.ptr(v)) for k, v in t.items()}
        return lib.pgl_conditional_simulate(p["Wff"], p["base"], 2, p["basis"], F, B, L, p["kind"], p["par"], p["neuron"], 1, 0, 0, p["ring"], None, 0,
                                            None, 0, p["sum"], p["sumsq"], 0, Tc, p["status"], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert entry(F=0) == 1 and entry(Tc=0) == 1 and entry(F=257) == 1
    for name in t:
        assert entry(**{name: True}) == 1, name
    torch.cuda.synchronize()
    assert float(t["sum"].min()) == 7.0 and int(t["status"].abs().sum()) == 0
    assert entry() == 0
    torch.cuda.synchronize()
    assert 7.0 <= float(t["sum"].min()) and float(t["sum"].max()) <= 7.0 + Tc


def test_sixteen_free_neurons_of_1024():
    N, B, L, F, R, T = 1024, 5, 100, 16, 8, 2000
    # (the recording comes from the device path of simulate(): the same law to the last bit, test_gpu_simulate.py, in a fraction of the time)
    model, Y = _recorded(N, B, L, ("bernoulli", "negbin"), T, seed=21, gpu=True)
    free = _pick(N, F, seed=2)
    d = model.conditional_simulate(free, replicates=R, seed=22, gpu=True)
    assert d.Y.shape == (R, T, F) and d.base.shape == (T, F) and 0 < d.Y.sum()
    h = _host(model, Y, d, R, 22, bins=300)
    _assert_same(d, h, bins=300)
