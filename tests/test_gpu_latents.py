"""Latent common input on the GPU (pyglm_amd/csrc/pgl_latents.hip) against its law, pyglm_amd/latents.py.

What is compared how, in units of U = 2^-53:
  fold     against latent_stats_host in long double from the same fp64 inputs.  An entry of Lambda is a sum over N columns of products
           w C_j C_k, two roundings each, and at most N - 1 roundings of partial sums in ANY order: (N + 8) U relative to sum_n |w C_j C_k|.
           An entry of r sums C_q c with c = Kappa + w (o - (Psi + bias)), o = sum_q x_q C_q: 2 Q roundings in o, four in c, one product,
           N - 1 sums: (N + 2 Q + 8) U relative to sum_n |C_q| (|Kappa| + |w| (sum_q |x_q C_q| + |psi_net|)).
  draw     ||x - x_ref||_2 <= 8 Q U kappa_2(A) ||x_ref||_2, x_ref by a long-double Cholesky: the form of tests/test_gpu_chol.py.
  stream   at Lambda = 0, A = I and x = r + z up to one rounding: z = x - r against latent_normals_host within 2^-44 absolute (the rounded
           argument 2 pi u1 is off by at most 2 pi 2^-53 and sqrt(-2 log u0) <= 8.6; a few ulp of the device's log / cos / sqrt on top).  A
           wrong counter or a swapped uniform is off by O(1).
The shapes are the kernels' edges: 64 lanes, the 256 columns of a wave's trip, 4 bins per workgroup (T around 256 = 64 workgroups' worth),
and PGL_LATENT_LDS_COLS = 1024 columns, the last size whose loadings are staged in LDS."""
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
# (T, nloc, Q, K_obs)
FOLD_CASES = [(1, 1, 1, 0), (255, 63, 3, 2), (256, 64, 8, 0), (257, 65, 8, 2), (257, 130, 3, 0), (257, 130, 1, 2), (5, 1030, 8, 2),
              (3, 1024, 8, 0), (3, 1025, 8, 0), (3, 1024, 1, 2), (3, 1025, 3, 2)]


def _cuda(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).cuda()           # (a copy: the cached inputs are read-only)


def _padded(x, ld, fill=np.nan):
    """(T, n) -> (T, ld) with `fill` (a NaN: whoever reads it as data shows) in the cells that are no part of x"""
    out = np.full((x.shape[0], ld), fill)
    out[:, :x.shape[1]] = x
    return out


# ------------------------------------------------------------------------------------------------------------------ fold
@functools.lru_cache(maxsize=None)
def _fold_inputs(T, N, Q, K_obs):
    rng = np.random.default_rng(7 * T + 3 * N + 11 * Q + K_obs)
    d = dict(S=rng.standard_normal((T, K_obs + Q)), beta=rng.standard_normal((N, K_obs + Q)), Psi=rng.standard_normal((T, N)) * 2,
             bias=rng.standard_normal(N), Omega=rng.uniform(0.02, 0.25, (T, N)), Kappa=rng.standard_normal((T, N)))
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _fold_reference(T, N, Q, K_obs):
    """long-double (Lambda (T, P), r (T, Q)) and the magnitudes their bounds are relative to"""
    d = _fold_inputs(T, N, Q, K_obs)
    C, x = d["beta"][:, K_obs:], d["S"][:, K_obs:]
    psi_net = d["Psi"].astype(LD) + d["bias"].astype(LD)
    Lam, r = lat.latent_stats_host(C, x, d["Omega"], d["Kappa"], psi_net, dtype=LD)
    aC = np.abs(C)
    mL = np.einsum("tn,nj,nk->tjk", d["Omega"], aC, aC)
    mr = (np.abs(d["Kappa"]) + d["Omega"] * (np.abs(x).dot(aC.T) + np.abs(psi_net.astype(np.float64)))).dot(aC)
    return cov.tri_pack(Lam), r, cov.tri_pack(mL), mr


def _fold(d, Q, K_obs, rows=None):
    """pgl_latent_fold of rows [lo, hi) (default: all) through offset pointers, from buffers with NaN padding (ldn > nloc, lds > K, ldb >
    nloc) -> (Lambda (rows, P), r (rows, Q)).  Checks that nothing outside Lambda and r is written: the guard cells behind them and every
    input buffer keep their bits."""
    import torch
    from pyglm_amd._lib import call, ptr
    T, N = d["Psi"].shape
    lo, hi = rows or (0, T)
    n, P, K = hi - lo, Q * (Q + 1) // 2, K_obs + Q
    ldn, lds, ldb = N + 3, K + 2, N + 5
    OK = np.full((T, 2 * ldn), np.nan)
    OK[:, :N], OK[:, ldn:ldn + N] = d["Omega"], d["Kappa"]
    ins = [_cuda(_padded(d["Psi"], ldn)), _cuda(OK), _cuda(_padded(d["S"], lds)), _cuda(_padded(d["beta"].T, ldb)), _cuda(d["bias"])]
    before = [t.clone() for t in ins]
    Psi, OKd, Sd, Bd, bias = ins
    Lam = torch.full((n * P + GUARD,), GARBAGE, dtype=torch.float64, device="cuda")
    r = torch.full((n * Q + GUARD,), GARBAGE, dtype=torch.float64, device="cuda")
    at = lambda t, ld, extra=0: ctypes.c_void_p(t.data_ptr() + 8 * (lo * ld + extra))
    call("pgl_latent_fold", Psi=at(Psi, ldn), ldn=ldn, bias=ptr(bias), Omega=at(OKd, 2 * ldn), ldo=2 * ldn, Kappa=at(OKd, 2 * ldn, ldn), ldk=2 * ldn,
         S=at(Sd, lds), lds=lds, col0=K_obs, Beta=ptr(Bd), ldb=ldb, T=n, nloc=N, Q=Q, Lambda=ptr(Lam), r=ptr(r), hip_stream=None)
    torch.cuda.synchronize()
    assert bool((Lam[n * P:] == GARBAGE).all()) and bool((r[n * Q:] == GARBAGE).all()), "elements behind Lambda or r were written"
    for was, now in zip(before, ins):
        assert torch.equal(was.view(torch.int64), now.view(torch.int64)), "an input buffer was written"
    return Lam[:n * P].cpu().numpy().reshape(n, P), r[:n * Q].cpu().numpy().reshape(n, Q)


def _check_fold(got, refs, N, Q, what):
    Lam, r = got
    Lr, rr, mL, mr = refs
    eL, er = np.abs(Lam.astype(LD) - Lr), np.abs(r.astype(LD) - rr)
    bL, br = (N + 8) * U * mL, (N + 2 * Q + 8) * U * mr
    print("%s: max err / bound: Lambda %.3f, r %.3f" % (what, float(np.max(eL / bL)), float(np.max(er / br))))
    assert np.all(eL <= bL) and np.all(er <= br)


@pytest.mark.parametrize("T, nloc, Q, K_obs", FOLD_CASES)
def test_fold_against_long_double(T, nloc, Q, K_obs):
    from pyglm_amd import _lib
    assert _lib.PGL_LATENT_LDS_COLS == 1024 and _lib.load().pgl_latent_max() == lat.LATENT_MAX
    _check_fold(_fold(_fold_inputs(T, nloc, Q, K_obs), Q, K_obs), _fold_reference(T, nloc, Q, K_obs), nloc, Q,
                "fold T=%d nloc=%d Q=%d K_obs=%d" % (T, nloc, Q, K_obs))


@pytest.mark.parametrize("T, nloc, Q, K_obs", [(257, 130, 8, 2), (5, 1030, 3, 0)])
def test_fold_bits_depend_on_the_row_alone(T, nloc, Q, K_obs):
    """two launches give the same bits; rows [a, b) folded alone -- another T, other workgroups, another grid -- equal those rows of the
    whole fold bit for bit"""
    d = _fold_inputs(T, nloc, Q, K_obs)
    whole, again = _fold(d, Q, K_obs), _fold(d, Q, K_obs)
    np.testing.assert_array_equal(whole[0], again[0]), np.testing.assert_array_equal(whole[1], again[1])
    lo, hi = (100, 203) if T > 200 else (1, 4)
    part = _fold(d, Q, K_obs, rows=(lo, hi))
    np.testing.assert_array_equal(part[0], whole[0][lo:hi]), np.testing.assert_array_equal(part[1], whole[1][lo:hi])
    one = _fold(d, Q, K_obs, rows=(T - 1, T))
    np.testing.assert_array_equal(one[0], whole[0][T - 1:]), np.testing.assert_array_equal(one[1], whole[1][T - 1:])


# ------------------------------------------------------------------------------------------------------------------ draw
def _ld_draw(A, rhs, z):
    """x = A^-1 rhs + L^-T z by a Cholesky in long double (numpy.linalg has none)"""
    K = A.shape[0]
    A, L = A.astype(LD), np.zeros((K, K), dtype=LD)
    for j in range(K):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j].dot(L[j, :j]))
        for i in range(j + 1, K):
            L[i, j] = (A[i, j] - L[i, :j].dot(L[j, :j])) / L[j, j]
    y = np.zeros(K, dtype=LD)
    for j in range(K):
        y[j] = (rhs[j] - L[j, :j].dot(y[:j])) / L[j, j]
    x, v = np.zeros(K, dtype=LD), y + z.astype(LD)
    for j in range(K - 1, -1, -1):
        x[j] = (v[j] - L[j + 1:, j].dot(x[j + 1:])) / L[j, j]
    return x


def _draw(LamP, r, z, S0, col0, seed=0, sweep=0, elem0=0, status0=0):
    """pgl_latent_draw on a copy of S0 (T, lds) behind guard cells -> (S (T, lds) afterwards, status)"""
    import torch
    from pyglm_amd._lib import call, ptr
    T, Q = r.shape
    lds = S0.shape[1]
    S = torch.full((T * lds + GUARD,), GARBAGE, dtype=torch.float64, device="cuda")
    S[:T * lds] = _cuda(S0).reshape(-1)
    status = torch.full((1 + 8,), 77, dtype=torch.int32, device="cuda")
    status[0] = status0
    Ld, rd, zd = _cuda(LamP), _cuda(r), (None if z is None else _cuda(z))
    call("pgl_latent_draw", Lambda=ptr(Ld), r=ptr(rd), z_override=ptr(zd), seed=seed, sweep=sweep, elem0=elem0, S=ptr(S), lds=lds, col0=col0,
         status=ptr(status), T=T, Q=Q, hip_stream=None)
    torch.cuda.synchronize()
    assert bool((S[T * lds:] == GARBAGE).all()) and bool((status[1:] == 77).all()), "cells behind S or status were written"
    return S[:T * lds].cpu().numpy().reshape(T, lds), int(status[0].item())


def _psd(rng, T, Q, scale):
    """(T, Q, Q) positive semi-definite, of rank Q - 1 where Q > 1, entries of order scale"""
    M = rng.standard_normal((T, Q, max(Q - 1, 1))) * np.sqrt(scale)
    return np.einsum("tik,tjk->tij", M, M)


@pytest.mark.parametrize("T, Q, col0", [(1, 1, 0), (255, 3, 2), (256, 8, 0), (257, 8, 2), (257, 1, 2)])
def test_draw_against_long_double(T, Q, col0):
    rng = np.random.default_rng(100 * T + 10 * Q + col0)
    Lam = _psd(rng, T, Q, 10.0 ** rng.integers(-2, 4))
    r, z = rng.standard_normal((T, Q)) * 3, rng.standard_normal((T, Q))
    if Q == 1:
        # the bound is relative to |x_ref|, and x = (y + z) / l is ONE scalar sum at Q = 1: where y and z cancel, the rounding of y alone
        # (U |y|) exceeds any multiple of U |x| -- in every fp64 algorithm.  That is the sum's conditioning, not the solve's, which the
        # bound is about: z takes r's sign there.  (From Q = 2 on the norm over the components carries the bound.)
        z = np.abs(z) * np.sign(r)
    lds = col0 + Q + 2
    S0 = rng.standard_normal((T, lds))
    S1, status = _draw(cov.tri_pack(Lam), r, z, S0, col0)
    assert status == 0
    keep = np.ones(lds, dtype=bool)
    keep[col0:col0 + Q] = False
    assert S1[:, keep].tobytes() == S0[:, keep].tobytes(), "a cell of S outside the latent columns changed"
    worst = 0.0
    for t in range(T):
        A = Lam[t] + np.eye(Q)
        ref = _ld_draw(A, r[t].astype(LD), z[t])
        err, tol = float(np.linalg.norm(S1[t, col0:col0 + Q] - ref)), 8 * Q * U * np.linalg.cond(A) * float(np.linalg.norm(ref))
        worst = max(worst, err / tol)
        assert err <= tol
    print("draw T=%d Q=%d: max err / bound %.3f" % (T, Q, worst))


def test_draw_flags_a_bad_pivot_and_leaves_the_row():
    rng = np.random.default_rng(5)
    T, Q = 70, 3
    Lam = _psd(rng, T, Q, 1.0)
    Lam[9] = -2.0 * np.eye(Q)                            # I + Lambda = -I
    Lam[66, 1, 1] = np.nan
    r, z = rng.standard_normal((T, Q)), rng.standard_normal((T, Q))
    S0 = rng.standard_normal((T, Q + 1))
    S1, status = _draw(cov.tri_pack(Lam), r, z, S0, 1, status0=4)
    assert status == 5                                   # the flag is set, what was there stays
    np.testing.assert_array_equal(S1[[9, 66]], S0[[9, 66]])
    good = np.ones(T, dtype=bool)
    good[[9, 66]] = False
    want = lat.latent_draw_host(Lam[good], r[good], z[good])
    np.testing.assert_allclose(S1[good, 1:], want, rtol=1e-11, atol=1e-12)
    assert _draw(cov.tri_pack(Lam[good]), r[good], z[good], S0[good], 1, status0=4)[1] == 4


@pytest.mark.parametrize("T, Q, elem0", [(257, 8, 1000), (3, 1, 0), (256, 3, 2 ** 32 - 100)])
def test_draw_stream_is_the_host_normals(T, Q, elem0):
    """z_override = NULL at Lambda = 0: z = x - r against latent_normals_host within 2^-44; row T - 1 and elem0 > 0 included, and an elem0
    whose elements wrap the 32-bit counter word as the host's do"""
    rng = np.random.default_rng(T + Q)
    seed, sweep = (9 << 40) + 123, (2 << 32) + 17
    r = rng.standard_normal((T, Q))
    S1, status = _draw(np.zeros((T, Q * (Q + 1) // 2)), r, None, np.zeros((T, Q)), 0, seed=seed, sweep=sweep, elem0=elem0)
    z = lat.latent_normals_host(seed, sweep, elem0, T, Q)
    err = np.abs((S1 - r) - z)
    print("stream T=%d Q=%d: max |z - host| = %.3e (2^-44 = %.3e)" % (T, Q, err.max(), 2.0 ** -44))
    assert status == 0 and np.all(err <= 2.0 ** -44)
    assert np.unique(S1 - r).size == T * Q


# ------------------------------------------------------------------------------------------------------------------ engine
EN = dict(N=5, B=2, T=300, Q=2, K_obs=1, seed=31, sweep=3)
KW = dict(rho=0.4, S_w=3.0, mu_w=0.0, mu_b=-1.5, S_b=2.0)


def test_engine_step_follows_the_host_law():
    """after one sweep under non-trivial beta and latents: latent_step(keep=True)'s statistics meet the fold's bounds against the long-double
    statistics of the Omega, Kappa, Psi, S and beta read back; x meets the draw's bound against the long-double draw from the device's own
    statistics and the host's normals, plus sqrt(Q) 2^-44 for the normals (|L^-T| <= 1 as A >= I); Off keeps its bits through the step, and
    after the covariate step equals offset_host([S_obs | X_new], beta_new) bit for bit"""
    import torch
    from pyglm_amd.engine import GibbsEngine, make_draws, prior_terms
    N, B, T, Q, K_obs = EN["N"], EN["B"], EN["T"], EN["Q"], EN["K_obs"]
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
    eng = GibbsEngine(N, B, n_covariates=K_obs, n_latents=Q)
    eng.add_data(Y, X=X, covariates=S_obs)
    lstep, cstep = lat._DeviceStep(eng), cov._DeviceStep(eng)
    ds = eng.datasets[0]
    assert eng.K == K and tuple(ds.S.shape) == (T, K) and not eng.latents(0).any()
    eng.set_covariate_weights(beta0)
    eng.set_latents(0, X0)
    np.testing.assert_array_equal(eng.latents(0), X0)
    S_old = np.column_stack([S_obs, X0])
    np.testing.assert_array_equal(ds.Off[:, :N].cpu().numpy(), cov.offset_host(S_old, beta0))
    regs = [orc.Regression(N, B, **KW) for _ in range(N)]
    hyp = prior_terms(np.array([r.S_w for r in regs]), np.array([r.mu_w for r in regs]), np.full(N, KW["S_b"]), np.full(N, KW["mu_b"]))
    perm, u, z = make_draws(EN["seed"], EN["sweep"], range(N), N, N * B)
    a1, W1, b1, _ = eng.sweep(a, W, b, np.full((N, N), KW["rho"]), *hyp, perm, u, z, seed=EN["seed"], sweep=EN["sweep"])
    off_before = ds.Off.clone()
    lstep.latent_step(a1, W1, b1, EN["seed"], EN["sweep"], keep=True)
    assert torch.equal(off_before.view(torch.int64), ds.Off.view(torch.int64)), "the latent step touched Off"
    OK = ds.OK[:T].cpu().numpy()
    Om, Kp = OK[:, :N], OK[:, eng.ldn:eng.ldn + N]
    Psi, bias = ds.Psi[:, :N].cpu().numpy(), eng.bias.cpu().numpy()
    np.testing.assert_array_equal(bias, b1)
    np.testing.assert_array_equal(eng.beta_dev[:, :N].cpu().numpy().T, beta0)
    S_new = ds.S.cpu().numpy()
    np.testing.assert_array_equal(S_new[:, :K_obs], S_obs)
    C = beta0[:, K_obs:]
    psi_net = Psi.astype(LD) + bias.astype(LD)
    Lr, rr = lat.latent_stats_host(C, X0, Om, Kp, psi_net, dtype=LD)
    aC = np.abs(C)
    mL = np.einsum("tn,nj,nk->tjk", Om, aC, aC)
    mr = (np.abs(Kp) + Om * (np.abs(X0).dot(aC.T) + np.abs(psi_net.astype(np.float64)))).dot(aC)
    LamD, rD = lstep.last_latent_stats[0]
    _check_fold((LamD, rD), (cov.tri_pack(Lr), rr, cov.tri_pack(mL), mr), N, Q, "engine fold")
    zs = lat.latent_normals_host(EN["seed"], EN["sweep"], ds.elem0, T, Q)
    LamF = cov.tri_unpack(LamD, Q)
    for t in range(T):
        A = LamF[t] + np.eye(Q)
        ref = _ld_draw(A, rD[t].astype(LD), zs[t])
        assert float(np.linalg.norm(S_new[t, K_obs:] - ref)) <= 8 * Q * U * np.linalg.cond(A) * float(np.linalg.norm(ref)) + np.sqrt(Q) * 2.0 ** -44
    np.testing.assert_allclose(S_new[:, K_obs:], lat.latent_step_host(C, X0, Om, Kp, Psi + bias, zs), rtol=1e-9, atol=1e-11)
    beta1 = cstep.covariate_step(a1, W1, b1, EN["seed"], EN["sweep"], psi_ready=True)
    assert beta1.shape == (N, K) and np.abs(beta1 - beta0).min() > 0
    np.testing.assert_array_equal(ds.Off[:, :N].cpu().numpy(), cov.offset_host(S_new, beta1))
    np.testing.assert_array_equal(ds.S.cpu().numpy(), S_new)                # the covariate step leaves S alone
    # the keyword only saves work: the same step with the upload and the activation done again draws the same beta from the same state
    eng.set_covariate_weights(beta0)
    eng.set_latents(0, X0)
    eng.sweep(a, W, b, np.full((N, N), KW["rho"]), *hyp, perm, u, z, seed=EN["seed"], sweep=EN["sweep"])
    lstep.latent_step(a1, W1, b1, EN["seed"], EN["sweep"])
    np.testing.assert_array_equal(ds.S.cpu().numpy(), S_new)
    np.testing.assert_array_equal(cstep.covariate_step(a1, W1, b1, EN["seed"], EN["sweep"]), beta1)
    eng.profile = True
    lstep.latent_step(a1, W1, b1, EN["seed"], EN["sweep"] + 1)
    tm = eng.collect_timings()
    assert tm["latent_fold"]["calls"] == 1 and tm["latent_draw"]["calls"] == 1 and tm["latent_fold"]["work"] == T * N


# ------------------------------------------------------------------------------------------------------------------ model
def _model_data(N=5, T=600, K_obs=1):
    rng = np.random.default_rng(4)
    S = np.sin(np.arange(T) / 7.0)[:, None] * np.ones((1, K_obs))
    g = rng.standard_normal(T)
    load = np.array([1.5, -1.5, 1.0, -1.0, 0.5])[:N]
    Y = (rng.random((T, N)) < 1 / (1 + np.exp(1.0 - 0.8 * S[:, :1] - g[:, None] * load))).astype(float)
    return Y, S


def test_model_chain_and_read_outs():
    """resample_model() for 3 sweeps; log_likelihood() and means equal NumPy's at psi_net + offset_host([S_obs | X], beta) to the existing
    model tests' 1e-12; the summary keeps the common drive's variance; the state round-trips, latents included"""
    from pyglm_amd import models
    N, B, K_obs, Q = 5, 2, 1, 2
    Y, S = _model_data(N)
    T = Y.shape[0]
    np.random.seed(2)
    m = models.SparseBernoulliGLM(N, B=B, seed=5, n_covariates=K_obs, n_latents=Q)
    m.add_data(Y, covariates=S)
    assert not m.latents[0].any()
    for _ in range(3):
        m.resample_model()
    x, C, bo = m.latents[0], m.latent_loadings, m.covariate_weights
    assert x.shape == (T, Q) and C.shape == (N, Q) and bo.shape == (N, K_obs) and np.abs(C).min() > 0 and x.std() > 0.5
    np.testing.assert_array_equal(m.common_input(), cov.offset_host(x, C))
    Xd = m.engine.design_matrix(0).reshape(T, N * B)
    psi = Xd.dot((m.adjacency[:, :, None] * m.weights).reshape(N, N * B).T) + m.biases + cov.offset_host(np.column_stack([S, x]), np.column_stack([bo, C]))
    np.testing.assert_allclose(m.log_likelihood(), np.sum(Y * psi - np.log1p(np.exp(psi))), rtol=1e-12)
    np.testing.assert_allclose(m.means[0], 1.0 / (1.0 + np.exp(-psi)), rtol=1e-12)
    acc = m.summarize()
    np.testing.assert_allclose(acc.collect(), m.log_likelihood(), rtol=1e-12)
    np.testing.assert_allclose(acc.rate_mean[0], m.means[0], rtol=1e-12)
    np.testing.assert_array_equal(acc.common_input_var_mean, np.sum(C ** 2, axis=1))
    st = m.get_state()
    m.resample_model()
    after = (m.latents[0], m.latent_loadings, m.covariate_weights, m.weights, m.biases, m.adjacency)
    m.set_state(st)
    np.testing.assert_array_equal(m.latents[0], x)
    m.resample_model()
    for p, q in zip(after, (m.latents[0], m.latent_loadings, m.covariate_weights, m.weights, m.biases, m.adjacency)):
        np.testing.assert_array_equal(p, q)
    with pytest.raises(ValueError, match="held-out"):
        m.log_likelihood(datas=[Y], covariates=[S])
    with pytest.raises(ValueError, match="n_latents=2"):
        m.simulate(10)


def test_without_latents_the_chain_keeps_its_bits():
    """n_latents=0 gives the same chain bit for bit as the model built without the argument, with covariates and without"""
    from pyglm_amd import models
    Y, S = _model_data()
    for kw, dkw in ((dict(), dict()), (dict(n_covariates=1), dict(covariates=S))):
        out = []
        for extra in (dict(), dict(n_latents=0)):
            np.random.seed(2)
            m = models.SparseBernoulliGLM(5, B=2, seed=5, **kw, **extra)
            m.add_data(Y, **dkw)
            for _ in range(3):
                m.resample_model()
            out.append((m.adjacency, m.weights, m.biases, m.covariate_weights, np.array(m.log_likelihood())))
        for p, q in zip(*out):
            assert p.tobytes() == q.tobytes()


def test_latents_take_the_common_input_off_the_network():
    """the recovery comparisons of tests/test_latents_host.py for the device chain: the same problem, seed and chain length"""
    from tests import _latent_engine as le
    Y, drive, load = le.recovery_problem()
    P0, _ = le.recovery_run(le.recovery_model(0), Y)
    P1, common = le.recovery_run(le.recovery_model(1), Y)
    ok, fig = le.recovery_verdict(P0, P1, common, Y, drive, load)
    print(fig)
    assert ok, fig
