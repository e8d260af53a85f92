"""The latents' temporal prior on the GPU (pyglm_amd/csrc/pgl_latent_dynamics.hip) against its law, pyglm_amd/latents.py.

pgl_latent_ar_draw maps normals z to x = m + M z.  Whatever elimination order it uses, the law is pinned by two facts, both measured against
J = ar_precision_dense in units of U = 2^-53 with kappa = kappa_2(J) from eigvalsh:
  mean        z = 0: ||x - J^-1 h||_2 <= 8 Q U kappa ||J^-1 h||_2, the reference a float64 solve refined with long-double residuals -- the
              form of the per-bin draw's bound (tests/test_gpu_latents.py) for the one T Q x T Q system.
  covariance  M from T Q calls with unit z: max |M M' J - I| <= 8 Q U kappa.
  stream      z_override = NULL against z_override = latent_normals_host: a normal is off by at most 2^-44 (tests/test_gpu_latents.py), so x
              by at most sqrt(T Q) 2^-44 ||M||_2.
The shapes: T below, at and one past a multiple of seg, empty and short last runs, one to eight levels, a phi with a zero entry, Q = 8, and
the default seg at one and at several levels.  Lambda_t = sum_n omega C C' over N = 6 neurons, omega ~ Gamma(1, 1/4)."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import pyglm_oracle as orc
from pyglm_amd import covariates as cov
from pyglm_amd import latents as lat

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
GUARD, GARBAGE = 512, 12345.0
# (T, Q, seg, phi)
CASES = [(1, 1, 2, .9), (2, 2, 2, (0, .9)), (3, 1, 2, .9), (37, 2, 2, (0, .9)), (37, 3, 3, .99), (64, 1, 4, .999), (65, 2, 4, .5), (40, 8, 5, .9),
         (300, 1, 2, .95), (96, 2, 32, .9), (33, 2, 0, .9), (2000, 2, 0, .99)]
COV_CASES = [c for c in CASES if c[0] * c[1] <= 320]


def _cuda(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).cuda()


def _inputs(T, Q, seed=None):
    rng = np.random.default_rng(1000 * T + Q if seed is None else seed)
    C, om = rng.standard_normal((6, Q)), rng.gamma(1.0, 0.25, size=(T, 6))
    return np.einsum("tn,nj,nk->tjk", om, C, C), rng.standard_normal((T, Q))


def _refined_solve(J, h):
    """J^-1 h: a float64 solve refined with long-double residuals"""
    Jl, hl = J.astype(LD), h.astype(LD)
    x = np.linalg.solve(J, h).astype(LD)
    for _ in range(4):
        x = x + np.linalg.solve(J, (hl - Jl.dot(x)).astype(np.float64))
    return x


@functools.lru_cache(maxsize=None)
def _reference(T, Q, phi):
    """(Lambda (T, Q, Q), r (T, Q), J, kappa, J^-1 h in long double) of a case, computed once"""
    Lam, r = _inputs(T, Q)
    J = lat.ar_precision_dense(Lam, phi)
    w = np.linalg.eigvalsh(J)
    out = (Lam, r, J, float(w[-1] / w[0]), _refined_solve(J, r.reshape(-1)))
    for v in (Lam, r, J, out[4]):
        v.setflags(write=False)
    return out


class _Draw(object):
    """pgl_latent_ar_draw on fixed (Lambda, r, phi, seg): the inputs go to the device once; every call starts from S0 (T, lds) behind guard
    cells and from scratch filled with NaN (whoever reads a cell nobody wrote shows) -> (the latent columns (T, Q), status)"""

    def __init__(self, Lam, r, phi, seg, col0=0, lds=None, seed=3):
        import torch
        from pyglm_amd import _lib
        self.T, self.Q = r.shape
        self.col0, self.lds, self.seg = col0, (col0 + self.Q if lds is None else lds), seg
        self.phi = (ctypes.c_double * self.Q)(*lat.check_ar(phi, self.Q))
        self.S0 = np.random.default_rng(seed).standard_normal((self.T, self.lds))
        self.S0d = _cuda(self.S0).reshape(-1)
        self.S = torch.full((self.T * self.lds + GUARD,), GARBAGE, dtype=torch.float64, device="cuda")
        self.Ld, self.rd = _cuda(cov.tri_pack(Lam)), _cuda(r)
        self.bytes = int(_lib.load().pgl_latent_ar_scratch(self.T, self.Q, seg))
        assert self.bytes % 8 == 0 and self.bytes >= 8 * self.T * self.Q
        self.scratch = torch.empty(self.bytes // 8 + GUARD, dtype=torch.float64, device="cuda")
        self.status = torch.full((1 + 8,), 77, dtype=torch.int32, device="cuda")

    def __call__(self, z, seed=0, sweep=0, elem0=0, status0=0, whole=False):
        import torch
        from pyglm_amd._lib import call, ptr
        T, Q, lds = self.T, self.Q, self.lds
        self.S[:T * lds] = self.S0d
        self.scratch[:self.bytes // 8] = float("nan")
        self.scratch[self.bytes // 8:] = GARBAGE
        self.status[0] = status0
        zd = None if z is None else _cuda(z)
        call("pgl_latent_ar_draw", Lambda=ptr(self.Ld), r=ptr(self.rd), phi=ctypes.cast(self.phi, ctypes.c_void_p), z_override=ptr(zd), seed=seed,
             sweep=sweep, elem0=elem0, S=ptr(self.S), lds=lds, col0=self.col0, status=ptr(self.status), T=T, Q=Q, seg=self.seg,
             scratch=ptr(self.scratch), scratch_bytes=self.bytes, hip_stream=None)
        torch.cuda.synchronize()
        assert bool((self.S[T * lds:] == GARBAGE).all()) and bool((self.status[1:] == 77).all()), "cells behind S or status were written"
        assert bool((self.scratch[self.bytes // 8:] == GARBAGE).all()), "cells behind the scratch were written"
        S1 = self.S[:T * lds].cpu().numpy().reshape(T, lds)
        keep = np.ones(lds, dtype=bool)
        keep[self.col0:self.col0 + Q] = False
        assert S1[:, keep].tobytes() == self.S0[:, keep].tobytes(), "a cell of S outside the latent columns changed"
        return (S1 if whole else S1[:, self.col0:self.col0 + Q].copy()), int(self.status[0].item())


@functools.lru_cache(maxsize=None)
def _device_map(T, Q, seg, phi):
    """(m, M) of the device: x at z = 0 and the T Q columns x(e_i) - m"""
    Lam, r = _reference(T, Q, phi)[:2]
    d = _Draw(Lam, r, phi, seg)
    m, status = d(np.zeros((T, Q)))
    assert status == 0
    M = np.empty((T * Q, T * Q))
    for i in range(T * Q):
        z = np.zeros(T * Q)
        z[i] = 1.0
        x, status = d(z.reshape(T, Q))
        assert status == 0
        M[:, i] = (x - m).reshape(-1)
    return m, M


# ------------------------------------------------------------------------------------------------------------------ the law
@pytest.mark.parametrize("T, Q, seg, phi", CASES)
def test_mean_against_refined_dense_solve(T, Q, seg, phi):
    Lam, r, J, kappa, ref = _reference(T, Q, phi)
    x, status = _Draw(Lam, r, phi, seg, col0=1, lds=Q + 3)(np.zeros((T, Q)))
    assert status == 0 and np.all(np.isfinite(x))
    err, tol = float(np.linalg.norm(x.reshape(-1) - ref)), 8 * Q * U * kappa * float(np.linalg.norm(ref))
    print("mean T=%d Q=%d seg=%d: kappa %.3g, err / bound %.4f" % (T, Q, seg, kappa, err / tol))
    assert err <= tol


@pytest.mark.parametrize("T, Q, seg, phi", COV_CASES)
def test_covariance_is_the_inverse_precision(T, Q, seg, phi):
    J, kappa = _reference(T, Q, phi)[2:4]
    _, M = _device_map(T, Q, seg, phi)
    err, tol = float(np.abs(M.dot(M.T).dot(J) - np.eye(T * Q)).max()), 8 * Q * U * kappa
    print("covariance T=%d Q=%d seg=%d: kappa %.3g, max |M M' J - I| / bound %.4f" % (T, Q, seg, kappa, err / tol))
    assert err <= tol


@pytest.mark.parametrize("elem0", [0, 2 ** 32 - 5])
def test_stream_is_the_host_normals(elem0):
    """every bin -- interiors of level 0, separators drawn at the levels above, the base chain -- is drawn on its own element of the stream"""
    T, Q, seg, phi = 37, 2, 2, (0, .9)
    Lam, r = _reference(T, Q, phi)[:2]
    _, M = _device_map(T, Q, seg, phi)
    seed, sweep = (9 << 40) + 123, (2 << 32) + 17
    d = _Draw(Lam, r, phi, seg)
    x_dev, s0 = d(None, seed=seed, sweep=sweep, elem0=elem0)
    z = lat.latent_normals_host(seed, sweep, elem0, T, Q)
    x_host, s1 = d(z)
    err, tol = float(np.linalg.norm(x_dev - x_host)), np.sqrt(T * Q) * 2.0 ** -44 * float(np.linalg.norm(M, 2))
    print("stream elem0=%d: |x - x(host z)| = %.3e, bound %.3e" % (elem0, err, tol))
    assert s0 == 0 and s1 == 0 and err <= tol
    assert np.unique(np.linalg.solve(M, (x_dev - d(np.zeros((T, Q)))[0]).reshape(-1)).round(9)).size == T * Q      # T Q distinct normals


# ------------------------------------------------------------------------------------------------------------------ geometry
def _engine_with_two_sets(T2, Q, phi):
    """an engine (N = 3, B = 1) with a short first data set and a second one of T2 bins, after one sweep"""
    from pyglm_amd.engine import GibbsEngine, make_draws, prior_terms
    N, B = 3, 1
    rng = np.random.default_rng(23)
    eng = GibbsEngine(N, B, n_latents=Q, latent_ar=phi)
    for T in (501, T2):
        eng.add_data((rng.random((T, N)) < 0.2).astype(float), basis=np.eye(B))
        eng.set_latents(len(eng.datasets) - 1, rng.standard_normal((T, Q)) * 0.3)
    eng.set_covariate_weights(rng.standard_normal((N, Q)) * 0.7)
    a, W, b = rng.random((N, N)) < 0.5, rng.standard_normal((N, N, B)) * 0.3, np.full(N, -1.0)
    regs = [orc.Regression(N, B, **KW) for _ in range(N)]
    hyp = prior_terms(np.array([r.S_w for r in regs]), np.array([r.mu_w for r in regs]), np.full(N, KW["S_b"]), np.full(N, KW["mu_b"]))
    perm, u, z = make_draws(7, 2, range(N), N, N * B)
    a1, W1, b1, _ = eng.sweep(a, W * a[:, :, None], b, np.full((N, N), 0.4), *hyp, perm, u, z, seed=7, sweep=2)
    return eng, (a1, W1, b1)


@pytest.mark.parametrize("Q", [1, 8])
def test_bits_do_not_depend_on_the_launch(Q):
    """T = 20 011 at the default seg (several levels, none of them a whole number of segments): two calls give the same bits, and so does the engine's step
    on its SECOND data set from the same statistics, scratch and stream position apart; the draw agrees with the host's on the same z
    (latent_ar_draw_host eliminating in the same order, which fixes the map z -> x) entry by entry within rtol 1e-8"""
    from pyglm_amd import _lib
    T, phi, seed, sweep = 20011, 0.9, 7, 2
    eng, (a1, W1, b1) = _engine_with_two_sets(T, Q, phi)
    step = lat._DeviceStep(eng)
    step.latent_step(a1, W1, b1, seed, sweep, keep=True)
    LamP, r = step.last_latent_stats[1]
    x_eng = eng.latents(1)
    ds = eng.datasets[1]
    assert ds.elem0 > 0 and np.all(np.isfinite(x_eng))
    d = _Draw(cov.tri_unpack(LamP, Q), r, phi, 0)
    x1, s1 = d(None, seed=seed, sweep=sweep, elem0=ds.elem0)
    x2, s2 = d(None, seed=seed, sweep=sweep, elem0=ds.elem0)
    assert s1 == 0 and s2 == 0
    assert x1.tobytes() == x2.tobytes() and x1.tobytes() == x_eng.tobytes()
    z = lat.latent_normals_host(seed, sweep, ds.elem0, T, Q)
    x3, s3 = d(z)
    want = lat.latent_ar_draw_host(cov.tri_unpack(LamP, Q), r, z, phi, seg=_lib.load().pgl_latent_ar_seg())
    assert s3 == 0
    for name, x in (("z_override", x3), ("stream", x1)):
        rel = np.abs(x - want) / np.abs(want)
        print("geometry Q=%d, %s: max |x - host| / |host| = %.3e at |host| = %.3e (smallest |host| %.3e)"
              % (Q, name, rel.max(), np.abs(want).reshape(-1)[rel.argmax()], np.abs(want).min()))
        np.testing.assert_allclose(x, want, rtol=1e-8, atol=0)


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("where, t_bad", [("interior", 9), ("separator", 11), ("separator of two levels", 15), ("base chain", 63)])
def test_bad_pivot_leaves_S_alone(where, t_bad):
    """T = 70, Q = 3, seg = 4 (chains of 70, 17 and 4 blocks): a negative definite block in one bin sets the flag and NOTHING of S is written,
    wherever the bin is eliminated; the flag is sticky"""
    T, Q, seg = 70, 3, 4
    Lam, r = _inputs(T, Q, seed=5)
    z = np.random.default_rng(6).standard_normal((T, Q))
    good = _Draw(Lam, r, 0.9, seg, col0=1, lds=Q + 1)
    S1, status = good(z, whole=True)
    assert status == 0 and np.abs(S1[:, 1:] - good.S0[:, 1:]).min() > 0
    Lam = Lam.copy()
    Lam[t_bad] = -50.0 * np.eye(Q)
    d = _Draw(Lam, r, 0.9, seg, col0=1, lds=Q + 1)
    for status0, want in ((0, 1), (4, 5)):
        S1, status = d(z, status0=status0, whole=True)
        assert status == want
        assert S1.tobytes() == d.S0.tobytes(), "S was written although a pivot was bad (%s)" % where
    Lam[t_bad, 1, 1] = np.nan
    S1, status = _Draw(Lam, r, 0.9, seg, col0=1, lds=Q + 1)(z, whole=True)
    assert status == 1 and S1.tobytes() == d.S0.tobytes()


def test_argument_checks():
    import torch
    from pyglm_amd import _lib
    from pyglm_amd._lib import PglError, call, ptr
    T, Q = 10, 2
    lib = _lib.load()
    assert lib.pgl_latent_ar_seg() >= 2
    assert lib.pgl_latent_ar_scratch(T, Q, 0) == lib.pgl_latent_ar_scratch(T, Q, lib.pgl_latent_ar_seg())
    assert lib.pgl_latent_ar_scratch(T, Q, T) >= 8 * T * Q and lib.pgl_latent_ar_scratch(T, 9, 0) == 0 and lib.pgl_latent_ar_scratch(T, Q, 1) == 0
    nbytes = int(lib.pgl_latent_ar_scratch(T, Q, 2))
    buf = dict(Lam=torch.zeros(T, 3, dtype=torch.float64, device="cuda"), r=torch.zeros(T, Q, dtype=torch.float64, device="cuda"),
               S=torch.full((T, Q), 5.0, dtype=torch.float64, device="cuda"), status=torch.zeros(1, dtype=torch.int32, device="cuda"),
               scratch=torch.zeros(nbytes // 8, dtype=torch.float64, device="cuda"))

    def draw(phi=(0.5, 0.5), **kw):
        p = (ctypes.c_double * 8)(*(list(phi) + [0.0] * (8 - len(phi))))
        args = dict(Lambda=ptr(buf["Lam"]), r=ptr(buf["r"]), phi=ctypes.cast(p, ctypes.c_void_p), z_override=None, seed=0, sweep=0, elem0=0,
                    S=ptr(buf["S"]), lds=Q, col0=0, status=ptr(buf["status"]), T=T, Q=Q, seg=2, scratch=ptr(buf["scratch"]), scratch_bytes=nbytes,
                    hip_stream=None)
        args.update(kw)
        return call("pgl_latent_ar_draw", **args)

    for bad in (dict(Q=0), dict(Q=9), dict(seg=1), dict(seg=-2), dict(phi=(0.5, 1.0)), dict(phi=(-0.1, 0.5)), dict(phi=(0.5, float("nan"))),
                dict(scratch_bytes=nbytes - 8), dict(scratch=None), dict(lds=1), dict(status=None), dict(T=-1)):
        with pytest.raises(PglError, match="argument check failed"):
            draw(**bad)
    torch.cuda.synchronize()
    assert bool((buf["S"] == 5.0).all())
    draw(T=0, Lambda=None, r=None, S=None, scratch=None, scratch_bytes=0)         # T = 0 launches nothing
    draw()
    torch.cuda.synchronize()
    assert int(buf["status"].item()) == 0 and not bool((buf["S"] == 5.0).any())


# ------------------------------------------------------------------------------------------------------------------ engine
KW = dict(rho=0.4, S_w=3.0, mu_w=0.0, mu_b=-1.5, S_b=2.0)


def test_engine_step_follows_the_law():
    """N = 5, T = 41, Q = 2, K_obs = 1, phi = .9, after one sweep under non-trivial beta and latents: the new latents are m + M z of the
    engine's own kept statistics -- m the refined dense solve, M the device's map from T Q unit calls on those statistics, z the host's
    normals at the data set's stream position -- within the mean's bound plus sqrt(Q) 2^-44 ||M||_2 for the normals; Off keeps its bits"""
    import torch
    from pyglm_amd.engine import GibbsEngine, make_draws, prior_terms
    N, B, T, Q, K_obs, phi, seed, sweep = 5, 2, 41, 2, 1, 0.9, 31, 3
    K = K_obs + Q
    rng = np.random.default_rng(17)
    basis = orc.cosine_basis(B, L=20) / 20
    Y = (rng.random((T, N)) < 0.2).astype(float)
    X = orc.convolve_with_basis(Y, basis)
    S_obs = np.sin(np.arange(T) / 9.0)[:, None]
    a = rng.random((N, N)) < 0.5
    W = rng.standard_normal((N, N, B)) * 0.5 * a[:, :, None]
    b = rng.standard_normal(N) * 0.2 - 1.0
    beta0, X0 = rng.standard_normal((N, K)) * 0.7, rng.standard_normal((T, Q))
    eng = GibbsEngine(N, B, n_covariates=K_obs, n_latents=Q, latent_ar=phi)
    np.testing.assert_array_equal(eng.latent_ar, [phi, phi])
    eng.add_data(Y, X=X, covariates=S_obs)
    ds = eng.datasets[0]
    eng.set_covariate_weights(beta0)
    eng.set_latents(0, X0)
    regs = [orc.Regression(N, B, **KW) for _ in range(N)]
    hyp = prior_terms(np.array([r.S_w for r in regs]), np.array([r.mu_w for r in regs]), np.full(N, KW["S_b"]), np.full(N, KW["mu_b"]))
    perm, u, z = make_draws(seed, sweep, range(N), N, N * B)
    a1, W1, b1, _ = eng.sweep(a, W, b, np.full((N, N), KW["rho"]), *hyp, perm, u, z, seed=seed, sweep=sweep)
    off_before = ds.Off.clone()
    eng.profile = True
    step = lat._DeviceStep(eng)
    step.latent_step(a1, W1, b1, seed, sweep, keep=True)
    tm = eng.collect_timings()
    assert tm["latent_fold"]["calls"] == 1 and tm["latent_ar_draw"]["calls"] == 1 and "latent_draw" not in tm
    assert torch.equal(off_before.view(torch.int64), ds.Off.view(torch.int64)), "the latent step touched Off"
    S_new = ds.S.cpu().numpy()
    np.testing.assert_array_equal(S_new[:, :K_obs], S_obs)
    LamD, rD = step.last_latent_stats[0]
    Lam = cov.tri_unpack(LamD, Q)
    J = lat.ar_precision_dense(Lam, phi)
    w = np.linalg.eigvalsh(J)
    kappa = float(w[-1] / w[0])
    d = _Draw(Lam, rD, phi, 0)
    m0, status = d(np.zeros((T, Q)))
    assert status == 0
    M = np.stack([(d(np.eye(T * Q)[i].reshape(T, Q))[0] - m0).reshape(-1) for i in range(T * Q)], axis=1)
    zs = lat.latent_normals_host(seed, sweep, ds.elem0, T, Q)
    ref = _refined_solve(J, rD.reshape(-1)) + M.astype(LD).dot(zs.reshape(-1).astype(LD))
    err = float(np.linalg.norm(S_new[:, K_obs:].reshape(-1) - ref))
    tol = 8 * Q * U * kappa * float(np.linalg.norm(ref)) + np.sqrt(Q) * 2.0 ** -44 * float(np.linalg.norm(M, 2))
    print("engine step: kappa %.3g, err %.3e, bound %.3e" % (kappa, err, tol))
    assert err <= tol
    C = beta0[:, K_obs:]
    OK = ds.OK[:T].cpu().numpy()
    psi_net = ds.Psi[:, :N].cpu().numpy() + eng.bias.cpu().numpy()
    from pyglm_amd import _lib
    want = lat.latent_ar_step_host(C, X0, OK[:, :N], OK[:, eng.ldn:eng.ldn + N], psi_net, zs, phi, seg=_lib.load().pgl_latent_ar_seg())
    np.testing.assert_allclose(S_new[:, K_obs:], want, rtol=1e-9, atol=1e-10)
    bad = GibbsEngine(N, B, n_latents=Q, latent_ar=phi)
    with pytest.raises(ValueError, match="latent_ar"):
        GibbsEngine(N, B, n_latents=Q, latent_ar=1.0)
    assert bad.latent_ar.shape == (Q,)


# ------------------------------------------------------------------------------------------------------------------ model
def _model_data(N=5, T=600, K_obs=1):
    rng = np.random.default_rng(4)
    S = np.sin(np.arange(T) / 7.0)[:, None] * np.ones((1, K_obs))
    g = rng.standard_normal(T)
    load = np.array([1.5, -1.5, 1.0, -1.0, 0.5])[:N]
    Y = (rng.random((T, N)) < 1 / (1 + np.exp(1.0 - 0.8 * S[:, :1] - g[:, None] * load))).astype(float)
    return Y, S


def _state_bytes(m):
    st = m.get_state()
    parts = [st["latents"][0].tobytes(), m._beta.tobytes(), m.adjacency.tobytes(), m.weights.tobytes(), m.biases.tobytes(),
             np.array(m.log_likelihood()).tobytes()]
    return b"".join(parts)


def test_phi_zero_keeps_the_chain_bit_for_bit():
    """latent_ar=0.0 (and a vector of zeros) is the model without the argument: the engine queues pgl_latent_draw, and three sweeps leave
    the same bytes of state"""
    from pyglm_amd import models
    Y, S = _model_data()
    out = []
    for extra in (dict(), dict(latent_ar=None), dict(latent_ar=0.0), dict(latent_ar=[0.0, 0.0])):
        np.random.seed(2)
        m = models.SparseBernoulliGLM(5, B=2, seed=5, n_covariates=1, n_latents=2, **extra)
        m.add_data(Y, covariates=S)
        m.engine.profile = True
        for _ in range(3):
            m.resample_model()
        tm = m.engine.collect_timings()
        assert tm["latent_draw"]["calls"] == 3 and "latent_ar_draw" not in tm
        np.testing.assert_array_equal(m.latent_ar, [0.0, 0.0])
        out.append(_state_bytes(m))
    assert out[0] == out[1] == out[2] == out[3]


def test_model_chain_and_read_outs():
    """resample_model() for 3 sweeps under latent_ar = (.9, .5); log_likelihood() and means equal NumPy's at psi_net + offset_host([S_obs | X],
    beta) to 1e-12; the state round-trips, latents included, and phi is no part of it"""
    from pyglm_amd import models
    N, B, K_obs, Q = 5, 2, 1, 2
    Y, S = _model_data(N)
    T = Y.shape[0]
    np.random.seed(2)
    m = models.SparseBernoulliGLM(N, B=B, seed=5, n_covariates=K_obs, n_latents=Q, latent_ar=(.9, .5))
    m.add_data(Y, covariates=S)
    np.testing.assert_array_equal(m.latent_ar, [.9, .5]), np.testing.assert_array_equal(m.engine.latent_ar, [.9, .5])
    m.engine.profile = True
    for _ in range(3):
        m.resample_model()
    tm = m.engine.collect_timings()
    assert tm["latent_ar_draw"]["calls"] == 3 and "latent_draw" not in tm
    x, C, bo = m.latents[0], m.latent_loadings, m.covariate_weights
    assert x.shape == (T, Q) and C.shape == (N, Q) and np.abs(C).min() > 0 and np.all(np.isfinite(x)) and x.std() > 0.3
    np.testing.assert_array_equal(m.common_input(), cov.offset_host(x, C))
    Xd = m.engine.design_matrix(0).reshape(T, N * B)
    psi = Xd.dot((m.adjacency[:, :, None] * m.weights).reshape(N, N * B).T) + m.biases + cov.offset_host(np.column_stack([S, x]), np.column_stack([bo, C]))
    np.testing.assert_allclose(m.log_likelihood(), np.sum(Y * psi - np.log1p(np.exp(psi))), rtol=1e-12)
    np.testing.assert_allclose(m.means[0], 1.0 / (1.0 + np.exp(-psi)), rtol=1e-12)
    st = m.get_state()
    assert "latent_ar" not in st
    m.resample_model()
    after = (m.latents[0], m.latent_loadings, m.covariate_weights, m.weights, m.biases, m.adjacency)
    m.set_state(st)
    np.testing.assert_array_equal(m.latents[0], x)
    m.resample_model()
    for p, q in zip(after, (m.latents[0], m.latent_loadings, m.covariate_weights, m.weights, m.biases, m.adjacency)):
        np.testing.assert_array_equal(p, q)
    with pytest.raises(ValueError, match="held-out"):
        m.log_likelihood(datas=[Y], covariates=[S])


def test_slow_drive_is_followed_better_with_the_temporal_prior():
    """the two-population problem of tests/_latent_engine.py under an AR(1) drive, phi_true = .98 (tests/_latent_ar_engine.py), T = 800, 50
    sweeps: the posterior-mean common input correlates with the true drive MORE under latent_ar = .95 than under independent bins"""
    from tests import _latent_ar_engine as la
    from tests import _latent_engine as le
    Y, drive, load = la.ar_recovery_problem()
    corr = {}
    for ar in (None, la.AR_RECOVERY["phi"]):
        _, common = le.recovery_run(la.ar_recovery_model(ar), Y)
        corr[ar] = la.ar_recovery_corr(common, drive, load)
    print("correlation of the mean common input with the true drive: independent bins %.3f, latent_ar=%.2f %.3f"
          % (corr[None], la.AR_RECOVERY["phi"], corr[la.AR_RECOVERY["phi"]]))
    assert corr[la.AR_RECOVERY["phi"]] > corr[None]
