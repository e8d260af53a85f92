"""Free-running simulation under covariates and latent factors on the GPU (pgl_simulate_offset in pgl_generate.hip, pgl_simulate_offset_build and
pgl_latent_prior_paths in pgl_simulate_offset.hip) against the law in pyglm_amd/simulate.py: the kernel with `Off` given at every launch plan of
simulate_kernel, Off = NULL, chunking, the offset builder and the prior paths bit for bit, the paths' stream within its bound, the model's side.

What is compared how:
  simulate   Y, sum, sumsq, history bit for bit (tests/test_gpu_simulate.py: _assert_same), the Gaussian case at its rtol 1e-10: the offset is
             one more rounded sum on both sides.  Every case stays far below 1e7 draws, as there.
  build      bit for bit against covariates.offset_host([S | X_r], beta): rounded products and sums in one order on both sides.
  paths      with z_override bit for bit against latent_recurrence_host (two rounded products, one rounded sum per step); on the stream within
             2^-43 / (1 - max phi) of latent_prior_host: 2^-44 per normal -- the figure tests/test_gpu_latents.py holds the stream to -- and an
             error e_t = phi e_{t-1} + s d_t with |d_t| <= 2^-44 stays below 2^-44 s / (1 - phi) <= 2^-44 / (1 - phi); the factor 2 covers the
             recurrence's own three roundings per step (|x| <= 9: 3 * 9 * 2^-53 / (1 - phi), a thousandth of the bound)."""
import ctypes
import types

import numpy as np
import pytest

from pyglm_amd import covariates as cov
from pyglm_amd import models, simulate
from pyglm_amd._lib import PglError
from pyglm_amd.utils.basis import cosine_basis
from tests import test_gpu_simulate as base

pytestmark = pytest.mark.gpu

GARBAGE = 12345.0


def _cuda(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).cuda()


def _bits(t):
    import torch
    return t.view(torch.int64).clone()


def _arrays(N, B, L, kinds, seed):
    """(Wm, bias, basis, kind, par) of a model of tests/test_gpu_simulate.py, or of its wide case"""
    if N >= 2000:
        rng = np.random.default_rng(41)
        Wm = rng.standard_normal((N, N * B)) * (0.5 / np.sqrt(N)) * (rng.random((N, N * B)) < 0.5)
        kind = (np.arange(N) % 3 + (np.arange(N) % 3 > 0)).astype(np.int32)
        par = np.where(kind == simulate.KIND_NEGBIN, 2.5, 10.0)
        Wm /= np.repeat(np.where(kind == simulate.KIND_BERNOULLI, 1.0, 5.0), B)[None, :]
        bias = np.where(kind == simulate.KIND_BERNOULLI, -2.0, -0.7) + 0.3 * rng.standard_normal(N)
        return Wm, bias, cosine_basis(B, L=L) / L, kind, par
    m = base._model(N, B, L, kinds, seed=seed, w_scale=0.5 / np.sqrt(N * B) if kinds == ("gaussian",) else None)
    A, W, b = m._adopt_state()
    kind, par = simulate.observation_kinds(m.regressions)
    return (W * A[:, :, None]).reshape(N, N * B), b.ravel().copy(), np.asarray(m.basis, dtype=np.float64), kind, par


def _launch(arr, T, R, seed, Off=None, ldo_t=0, ldo_r=0, entry="pgl_simulate_offset", t0=0, rep0=0):
    """one launch of `entry` over T bins from silence -> what _assert_same compares"""
    import torch
    from pyglm_amd import _lib
    from pyglm_amd._lib import call, ptr
    Wm, bias, basis, kind, par = arr
    N, (L, B) = Wm.shape[0], basis.shape
    Wm_d, bias_d, basis_d, par_d = _cuda(Wm), _cuda(bias), _cuda(basis), _cuda(par)
    kind_d = _cuda(np.asarray(kind, dtype=np.int32))
    f64 = dict(dtype=torch.float64, device="cuda")
    ring, Y = torch.zeros((R, L, N), **f64), torch.empty((R, T, N), **f64)
    s, ss = torch.zeros((R, N), **f64), torch.zeros((R, N), **f64)
    work = torch.zeros(_lib.load().pgl_simulate_work_bytes(N, B, R), dtype=torch.uint8, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    kw = dict(Off=ptr(Off), ldo_t=ldo_t, ldo_r=ldo_r) if entry == "pgl_simulate_offset" else {}
    call(entry, Wm=ptr(Wm_d), bias=ptr(bias_d), basis=ptr(basis_d), N=N, B=B, L=L, kind=ptr(kind_d), par=ptr(par_d), R=R, rep0=rep0, seed=seed,
         ring=ptr(ring), Y=ptr(Y), ldr=T * N, sum=ptr(s), sumsq=ptr(ss), t0=t0, Tc=T, work=ptr(work), status=ptr(status), hip_stream=None, **kw)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, 0, 0]
    rows = (t0 + T - L + np.arange(L)) % L
    return types.SimpleNamespace(Y=Y.cpu().numpy(), sum=s.cpu().numpy(), sumsq=ss.cpu().numpy(), history=ring.cpu().numpy()[:, rows], t0=t0, t1=t0 + T)


def _host(arr, T, R, seed, off, t0=0, rep0=0):
    Wm, bias, basis, kind, par = arr
    return simulate.simulate_host(Wm, bias, basis, kind, par, T, R, seed, rep0, np.zeros((R, basis.shape[0], Wm.shape[0])), t0, True, offset=off)


# one shape per launch plan of simulate_kernel, and a Gaussian one
SHAPES = [(4, 1, 100, ("bernoulli",), 1, 600, True),                              # one workgroup
          (12, 3, 30, ("bernoulli", "negbin", "binomial"), 3, 500, True),        # one workgroup, lanes in groups per neuron, kinds mixed
          (64, 5, 100, ("bernoulli", "negbin"), 8, 400, True),                   # rows in registers, rings in LDS
          (64, 5, 100, ("bernoulli", "negbin"), 24, 120, True),                  # rings in global memory, several replicate groups
          (2100, 4, 10, None, 3, 30, True),                                      # x from the exchange buffer
          (5, 2, 30, ("gaussian",), 3, 500, False)]


@pytest.mark.parametrize("N,B,L,kinds,R,T,exact", SHAPES)
def test_kernel_is_the_host_law_under_an_offset(N, B, L, kinds, R, T, exact):
    arr = _arrays(N, B, L, kinds, seed=N + R)
    rng = np.random.default_rng(N + T)
    off = rng.uniform(-1.0, 1.0, (R, T, N))
    per = _cuda(off)
    shared = _cuda(off[0])
    ld = N + 5
    padded = np.full((R, T, ld), np.nan)                              # whoever reads the padding as data shows
    padded[:, :, :N] = off
    padded = _cuda(padded)
    before = [_bits(t) for t in (per, shared, padded)]
    want = _host(arr, T, R, 1000 + N, off)
    if exact:                                                         # offsets of size 1 leave the spike trains neither silent nor saturated
        assert 0.0 < want.Y[:, :, arr[3] == simulate.KIND_BERNOULLI].mean() < 1.0
    base._assert_same(_launch(arr, T, R, 1000 + N, per, N, T * N), want, exact=exact)
    base._assert_same(_launch(arr, T, R, 1000 + N, padded, ld, T * ld), want, exact=exact)
    base._assert_same(_launch(arr, T, R, 1000 + N, shared, N, 0), _host(arr, T, R, 1000 + N, off[:1]), exact=exact)
    for was, t in zip(before, (per, shared, padded)):
        assert bool((was == _bits(t)).all()), "Off was written"
    if exact:
        assert not np.array_equal(want.Y, _host(arr, T, R, 1000 + N, None).Y)       # (the offset decides draws)


def test_a_null_offset_is_pgl_simulate():
    arr = _arrays(64, 5, 100, ("bernoulli", "negbin"), seed=72)
    a = _launch(arr, 300, 8, 5, None, 0, 0)
    b = _launch(arr, 300, 8, 5, entry="pgl_simulate")
    base._assert_same(a, b)
    base._assert_same(a, _host(arr, 300, 8, 5, None))


def test_offset_arguments_are_checked():
    arr = _arrays(4, 1, 100, ("bernoulli",), seed=5)
    Off = _cuda(np.zeros((2, 10, 4)))
    for ldo_t, ldo_r in ((3, 40), (4, 39), (4, -1)):
        with pytest.raises(PglError):
            _launch(arr, 10, 2, 1, Off, ldo_t, ldo_r)


def _drive(N, K_obs, Q, T, seed, latents="prior", phi=None):
    rng = np.random.default_rng(seed)
    return simulate.Drive(rng.standard_normal((N, K_obs + Q)) * 0.5, S_obs=rng.standard_normal((T, K_obs)) if K_obs else None,
                          latents=latents if Q else None, phi=phi)


def test_chunks_that_do_not_divide_T(monkeypatch):
    N, B, L, T, R = 16, 2, 10, 100, 3
    Wm, bias, basis, kind, par = _arrays(N, B, L, ("bernoulli", "negbin"), seed=7)
    drive = _drive(N, 2, 3, T, 1, phi=np.array([0.9, 0.0, 0.5]))
    run = lambda dev, **kw: simulate.simulate(Wm, bias, basis, kind, par, T, replicates=R, seed=8, on_device=dev, drive=drive, **kw)
    whole = run(True)
    monkeypatch.setattr(simulate, "chunk_bins", lambda N, B, R=1: 7)         # 14 launches of 7 bins and one of 2
    cut = run(True)
    base._assert_same(cut, whole)
    assert np.array_equal(cut.latents, whole.latents) and np.array_equal(cut.latent_last, whole.latent_last)
    # the host path on the device's latents: the same law (its own prior paths differ from the device's in the last bits of a normal)
    fed = simulate.Drive(drive.beta, S_obs=drive.S_obs, latents=cut.latents)
    host = simulate.simulate(Wm, bias, basis, kind, par, T, replicates=R, seed=8, on_device=False, drive=fed)
    base._assert_same(cut, host)
    # row k of the covariates belongs to bin t0 + k: a forecast from an array at t0 = 250, cut likewise
    cov_only = _drive(N, 2, 0, T, 2)
    hist = (np.random.default_rng(3).random((L, N)) < 0.3).astype(float)
    d = simulate.simulate(Wm, bias, basis, kind, par, T, replicates=R, seed=8, on_device=True, drive=cov_only, history=hist, t0=250)
    off = cov.offset_host(cov_only.S_obs, cov_only.beta)[None]
    h = simulate.simulate_host(Wm, bias, basis, kind, par, T, R, 8, 0, np.broadcast_to(hist, (R, L, N)).copy(), 250, True, offset=off)
    assert (d.t0, d.t1) == (250, 350)
    base._assert_same(d, h)


# ------------------------------------------------------------------------------------------------------------------ the offset builder
@pytest.mark.parametrize("Tc,N,K_obs,Q,R", [(1, 1, 1, 0, 1), (63, 65, 2, 1, 3), (64, 64, 0, 8, 2), (65, 130, 24, 8, 4)])
def test_offset_build_is_offset_host(Tc, N, K_obs, Q, R):
    import torch
    from pyglm_amd._lib import call, ptr
    rng = np.random.default_rng(Tc + N + Q)
    K = K_obs + Q
    S, X, beta = rng.standard_normal((Tc, K_obs)), rng.standard_normal((R, Tc, Q)), rng.standard_normal((N, K))
    lds, ldn, ldo = K_obs + 2, N + 5, N + 3
    Sp = np.full((Tc, lds), np.nan)
    Sp[:, :K_obs] = S
    Bp = np.full((K, ldn), np.nan)
    Bp[:, :N] = beta.T
    S_d, X_d, B_d = _cuda(Sp), _cuda(X), _cuda(Bp)
    Off = torch.full((R, Tc, ldo), GARBAGE, dtype=torch.float64, device="cuda")
    call("pgl_simulate_offset_build", S=ptr(S_d) if K_obs else None, lds=lds, X=ptr(X_d) if Q else None, ldx_r=Tc * Q if R > 1 else 0, Beta=ptr(B_d),
         ldn=ldn, Off=ptr(Off), ldo_t=ldo, ldo_r=Tc * ldo, Tc=Tc, N=N, K_obs=K_obs, Q=Q, R=R, hip_stream=None)
    got = Off.cpu().numpy()
    assert np.all(got[:, :, N:] == GARBAGE), "guard columns were written"
    want = simulate.simulate_offset_host(S if K_obs else None, X if Q else None, beta)
    assert want.shape == (R, Tc, N) and np.array_equal(got[:, :, :N], want)
    if Q == 0:
        ref = torch.full((Tc, ldo), GARBAGE, dtype=torch.float64, device="cuda")
        call("pgl_covariate_offset", S=ptr(S_d), lds=lds, Beta=ptr(B_d), Off=ptr(ref), ldn=ldn, T=Tc, nloc=N, K=K_obs, hip_stream=None)
        assert np.array_equal(ref.cpu().numpy()[:, :N].view(np.int64), want[0].view(np.int64))


def test_offset_build_takes_shared_latents_and_checks_its_arguments():
    import torch
    from pyglm_amd._lib import call, ptr
    rng = np.random.default_rng(0)
    Tc, N, K_obs, Q = 70, 9, 1, 2
    S, X, beta = rng.standard_normal((Tc, K_obs)), rng.standard_normal((1, Tc, Q)), rng.standard_normal((N, K_obs + Q))
    S_d, X_d, B_d = _cuda(S), _cuda(X), _cuda(beta.T)
    Off = torch.full((Tc, N), GARBAGE, dtype=torch.float64, device="cuda")
    kw = dict(S=ptr(S_d), lds=K_obs, X=ptr(X_d), ldx_r=0, Beta=ptr(B_d), ldn=N, Off=ptr(Off), ldo_t=N, ldo_r=0, Tc=Tc, N=N, K_obs=K_obs, Q=Q, R=1,
              hip_stream=None)
    call("pgl_simulate_offset_build", **kw)
    assert np.array_equal(Off.cpu().numpy(), simulate.simulate_offset_host(S, X, beta)[0])
    Off.fill_(GARBAGE)
    for bad in (dict(Q=9), dict(K_obs=0, Q=0), dict(R=2), dict(ldo_t=N - 1), dict(ldn=N - 1), dict(lds=0), dict(Tc=0), dict(X=None), dict(Beta=None),
                dict(K_obs=31, lds=31)):
        with pytest.raises(PglError):
            call("pgl_simulate_offset_build", **dict(kw, **bad))
    torch.cuda.synchronize()
    assert bool((Off == GARBAGE).all())


# ------------------------------------------------------------------------------------------------------------------ the prior paths
def _paths(R, Tc, Q, phi, t0=0, rep0=0, seed=1, carry=None, z=None, ldx_r=None):
    """one pgl_latent_prior_paths call -> (X (R, Tc, Q), carry (R, Q))"""
    import torch
    from pyglm_amd._lib import call, ptr
    ldx_r = Tc * Q if ldx_r is None else ldx_r
    X = torch.full((R * ldx_r + 64,), GARBAGE, dtype=torch.float64, device="cuda")
    c = _cuda(np.zeros((R, Q)) if carry is None else carry)
    z_d = None if z is None else _cuda(z)
    phi = np.asarray(phi, dtype=np.float64)
    s = np.sqrt(1.0 - phi * phi)
    call("pgl_latent_prior_paths", X=ptr(X), ldx_r=ldx_r, R=R, rep0=rep0, t0=t0, Tc=Tc, Q=Q, phi=ctypes.cast((ctypes.c_double * Q)(*phi), ctypes.c_void_p),
         s=ctypes.cast((ctypes.c_double * Q)(*s), ctypes.c_void_p), carry=ptr(c), has_carry=0 if carry is None else 1, z_override=ptr(z_d),
         seed=seed, hip_stream=None)
    out = X.cpu().numpy()
    assert np.all(out[R * ldx_r:] == GARBAGE), "elements behind X were written"
    return out[:R * ldx_r].reshape(R, ldx_r)[:, :Tc * Q].reshape(R, Tc, Q), c.cpu().numpy()


@pytest.mark.parametrize("Q,R,Tc", [(1, 1, 1), (3, 5, 63), (8, 64, 64), (3, 1, 65), (8, 5, 1638), (1, 64, 65), (8, 1, 513)])
@pytest.mark.parametrize("has_carry", [0, 1])
def test_paths_recurrence_is_the_host_loop(Q, R, Tc, has_carry):
    rng = np.random.default_rng(Q + R + Tc)
    phi = np.array([0.9, 0.0, 0.5, 0.99, 0.3, 0.0, 0.7, 0.95])[:Q] if Q > 1 else np.array([0.9])
    z1, z2 = rng.standard_normal((R, Tc, Q)), rng.standard_normal((R, Tc, Q))
    carry = rng.standard_normal((R, Q)) if has_carry else None
    X1, c1 = _paths(R, Tc, Q, phi, carry=carry, z=z1)
    want1 = simulate.latent_recurrence_host(z1, phi, carry)
    assert np.array_equal(X1, want1) and np.array_equal(c1, want1[:, -1])
    X2, c2 = _paths(R, Tc, Q, phi, carry=c1, z=z2)                    # the next chunk, from the carry the first one left
    whole = simulate.latent_recurrence_host(np.concatenate([z1, z2], axis=1), phi, carry)
    assert np.array_equal(np.concatenate([X1, X2], axis=1), whole) and np.array_equal(c2, whole[:, -1])
    if Q > 1 and not has_carry:
        assert np.array_equal(X1[:, :, 1], z1[:, :, 1])               # phi = 0: z itself


@pytest.mark.parametrize("t0,Tc,rep0", [(0, 700, 0), (2 ** 32 - 5, 10, 3), (123456, 65, 2 ** 31 - 70)])
def test_paths_on_the_stream(t0, Tc, rep0):
    R, Q, seed = 5, 3, 0xFEDCBA9876543210
    phi = np.array([0.9, 0.0, 0.5])
    X, c = _paths(R, Tc, Q, phi, t0=t0, rep0=rep0, seed=seed)
    want = simulate.latent_prior_host(seed, rep0 + np.arange(R), t0, Tc, phi)
    dev = float(np.max(np.abs(X - want)))
    print("paths t0=%d Tc=%d: max |X - host| = %.3g = 2^%.1f (bound 2^-43 / (1 - max phi) = %.3g)" % (t0, Tc, dev, np.log2(max(dev, 1e-300)), 2.0 ** -43 / 0.1))
    assert dev <= 2.0 ** -43 / (1.0 - phi.max())
    assert np.array_equal(c, X[:, -1]) and np.unique(X).size == X.size
    # replicate rep0 + 2 alone, and the chunk cut in two with the carry: the same bits
    one, _ = _paths(1, Tc, Q, phi, t0=t0, rep0=rep0 + 2, seed=seed)
    assert np.array_equal(one[0], X[2])
    a, ca = _paths(R, 4, Q, phi, t0=t0, rep0=rep0, seed=seed)
    b, _ = _paths(R, Tc - 4, Q, phi, t0=t0 + 4, rep0=rep0, seed=seed, carry=ca)
    assert np.array_equal(np.concatenate([a, b], axis=1), X)
    wide, _ = _paths(R, Tc, Q, phi, t0=t0, rep0=rep0, seed=seed, ldx_r=Tc * Q + 7)      # a replicate stride beyond the chunk
    assert np.array_equal(wide, X)


def test_paths_arguments_are_checked():
    import torch
    from pyglm_amd._lib import call, ptr
    R, Tc, Q = 2, 5, 2
    X = torch.full((R * Tc * Q,), GARBAGE, dtype=torch.float64, device="cuda")
    c = torch.zeros((R, Q), dtype=torch.float64, device="cuda")
    vec = lambda *v: ctypes.cast((ctypes.c_double * len(v))(*v), ctypes.c_void_p)
    kw = dict(X=ptr(X), ldx_r=Tc * Q, R=R, rep0=0, t0=0, Tc=Tc, Q=Q, phi=vec(0.5, 0.0), s=vec(np.sqrt(0.75), 1.0), carry=ptr(c), has_carry=0,
              z_override=None, seed=1, hip_stream=None)
    for bad in (dict(Q=0), dict(Q=9), dict(R=0), dict(Tc=0), dict(rep0=-1), dict(has_carry=2), dict(X=None), dict(carry=None), dict(phi=None), dict(s=None),
                dict(ldx_r=Tc * Q - 1), dict(phi=vec(1.0, 0.0)), dict(phi=vec(-0.1, 0.0)), dict(s=vec(0.0, 1.0)), dict(phi=vec(float("nan"), 0.0))):
        with pytest.raises(PglError) as e:
            call("pgl_latent_prior_paths", **dict(kw, **bad))
        assert "argument check failed" in str(e.value)
    torch.cuda.synchronize()
    assert bool((X == GARBAGE).all()) and bool((c == 0).all())
    call("pgl_latent_prior_paths", **kw)
    assert bool((X != GARBAGE).all())


# ------------------------------------------------------------------------------------------------------------------ the model's side
@pytest.fixture(scope="module")
def fitted():
    N, B, T = 6, 2, 300
    rng = np.random.default_rng(12)
    S = np.where((np.arange(T) // 25) % 2 == 0, 1.0, -1.0)[:, None]
    g = np.cumsum(rng.standard_normal(T)) * 0.15
    psi = -1.2 + S * np.array([1.0, -1.0, 1.0, -1.0, 0.5, 0.0]) + g[:, None] * np.array([1.0, 1.0, -1.0, -1.0, 0.5, 0.5])
    Y = (rng.random((T, N)) < 1.0 / (1.0 + np.exp(-psi))).astype(float)
    np.random.seed(4)
    m = models.SparseBernoulliGLM(N, B=B, seed=7, n_covariates=1, n_latents=2, latent_ar=[0.9, 0.0])
    m.add_data(Y, covariates=S)
    for _ in range(3):
        m.resample_model()
    return m, Y, S


def test_model_simulates_under_prior_and_fitted_latents(fitted):
    m, Y, S = fitted
    T = Y.shape[0]
    d = m.simulate(T, replicates=3, seed=5, gpu=True, covariates=S, latents="prior", first_replicate=2)
    assert d.latents.shape == (3, T, 2) and np.array_equal(d.latent_last, d.latents[:, -1])
    want = simulate.latent_prior_host(5, 2 + np.arange(3), 0, T, m.latent_ar)
    assert np.max(np.abs(d.latents - want)) <= 2.0 ** -43 / (1.0 - 0.9)
    h = m.simulate(T, replicates=3, seed=5, gpu=False, covariates=S, latents=d.latents, first_replicate=2)
    base._assert_same(d, h)
    assert 0.0 < d.Y.mean() < 1.0 and len(np.unique(d.sum, axis=0)) == 3
    bare = m.simulate(T, replicates=3, seed=5, gpu=True, covariates=S, latents="prior", first_replicate=2, keep_paths=False)
    assert bare.Y is None and bare.latents is None and np.array_equal(bare.sum, d.sum) and np.array_equal(bare.latent_last, d.latent_last)
    df, hf = (m.simulate(T, replicates=3, seed=6, gpu=gpu, covariates="data", latents="fitted") for gpu in (True, False))
    base._assert_same(df, hf)
    assert df.latents.shape == (1, T, 2) and np.array_equal(df.latents[0], m.latents[0]) and np.array_equal(df.latent_last, hf.latent_last)
    assert not np.array_equal(df.Y, d.Y)


def test_model_continuation_is_one_call(fitted):
    m, Y, S = fitted
    whole = m.simulate(300, replicates=3, seed=9, gpu=True, covariates=S, latents="prior")
    first = m.simulate(130, replicates=3, seed=9, gpu=True, covariates=S[:130], latents="prior")
    second = m.simulate(170, replicates=3, seed=9, gpu=True, covariates=S[130:], latents="prior", history=first)
    assert (second.t0, second.t1) == (130, 300)
    assert np.array_equal(np.concatenate([first.Y, second.Y], axis=1), whole.Y)
    assert np.array_equal(np.concatenate([first.latents, second.latents], axis=1), whole.latents)
    assert np.array_equal(second.latent_last, whole.latent_last) and np.array_equal(first.sum + second.sum, whole.sum)


def test_predictive_check_matches_the_host_path(fitted):
    m, Y, S = fitted
    out = []
    for gpu in (True, False):
        ppc = m.predictive_check(replicates=4, seed=3, gpu=gpu, covariates="data", latents="prior", lags=3, isi=8)
        ppc.collect()
        ppc.collect()
        out.append(ppc)
    d, h = out
    assert d.rates.shape == (8, m.N)
    assert np.array_equal(d.rates, h.rates) and np.array_equal(d.fanos, h.fanos, equal_nan=True)
    for stat in ("rate", "fano", "isi", "cv"):                        # from integer sums, on the host on both sides
        assert np.array_equal(d.pvalue(stat), h.pvalue(stat), equal_nan=True), stat
    # the correlogram's p-values count c_rep >= c_obs and c_rep <= c_obs cell by cell, with c computed by torch on the device and by NumPy on
    # the host.  Where a replicate's integer sums equal the data's, c_rep = c_obs in exact arithmetic -- always in a cell (lag 0, i, i), where
    # c = (m - m^2) / (m - m^2) = 1, and now and then in a cell (lag, i, i) of 300 bins -- and the last bit of two libraries' division
    # decides the tie.  A cell without a tie on either side (ge + le = n) must agree; the moments below are held everywhere
    sd, sh = d._xcorr_state(), h._xcorr_state()
    differ = d.pvalue("xcorr") != h.pvalue("xcorr")
    tie = (sd[1] + sd[2] > sd[3]) | (sh[1] + sh[2] > sh[3])
    print("xcorr p-value cells that differ: %d of %d; cells with a tie: %d" % (int(differ.sum()), differ.size, int(tie.sum())))
    assert not (differ & ~tie).any() and not tie.all()
    np.testing.assert_allclose(d.xcorr_mean, h.xcorr_mean, rtol=0, atol=1e-12)
    np.testing.assert_allclose(d.xcorr_std, h.xcorr_std, rtol=0, atol=1e-12)
    np.testing.assert_allclose(d.isi_mean, h.isi_mean, rtol=0, atol=1e-12)
    np.testing.assert_allclose(d.isi_std, h.isi_std, rtol=0, atol=1e-12)
    assert np.all(np.isfinite(d.pvalue("rate"))) and d.pvalue("xcorr").shape == (3, m.N, m.N)


def test_a_model_without_either_term_simulates_as_before(fitted):
    np.random.seed(2)
    m = models.SparseBernoulliGLM(6, B=2, seed=7, n_covariates=0, n_latents=0)
    m.add_data(fitted[1])
    m.resample_model()
    d, h = (m.simulate(200, replicates=3, seed=4, gpu=gpu) for gpu in (True, False))
    base._assert_same(d, h)
    A, W, b = m._adopt_state()
    kind, par = simulate.observation_kinds(m.regressions)
    arr = ((W * A[:, :, None]).reshape(6, -1), b.ravel().copy(), np.asarray(m.basis, dtype=np.float64), kind, par)
    base._assert_same(d, _launch(arr, 200, 3, 4, entry="pgl_simulate"))          # the entry it always went through, called directly
    assert d.latents is None and d.latent_last is None
    with pytest.raises(ValueError, match="n_latents=0"):
        m.simulate(10, gpu=True, latents="prior")
