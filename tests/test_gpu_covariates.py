"""External covariates on the GPU (pyglm_amd/csrc/pgl_covariates.hip, pgl_sweep_offset) against their law, pyglm_amd/covariates.py.

What is compared how:
  offset   bit for bit with offset_host (one rounded product and one rounded sum per term on both sides).
  fold     against covariate_stats_host in long double from the same fp64 inputs.  In units of 2^-53: an entry of Lambda is a sum of T
           products w S_j S_k, two roundings each, and at most T - 1 roundings of partial sums in ANY order: T + 1 <= T + 8, relative to
           sum_t |w S_j S_k|.  An entry of r sums S_k c with c = Kappa + w (o - (psi + bias)): four roundings inside c, each relative to a
           part of |Kappa| + |w| (|o| + |psi_net|), one for the product, T - 1 for the sums: T + 4 <= T + 8.
  draw     ||beta - beta_ref||_2 <= 8 K 2^-53 kappa_2(Lambda_n) ||beta_ref||_2, beta_ref by a long-double Cholesky: the form of
           tests/test_gpu_chol.py.
  sweep    flips equal, weights and bias to 1e-8 (the golden sweep tests' tolerance) against the oracle composed from its own pieces.
The shapes are the block edges of the kernels: 64 columns, 64 rows (offset), 256 rows (fold), 8 x 8 blocks of (j, k) pairs."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import pyglm_oracle as orc
from pyglm_amd import covariates as cov
from tests._covariate_engine import RECOVERY, recovery_problem, recovery_verdict
from tests._pg_agree import assert_pg_agree

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
GUARD, GARBAGE = 512, 12345.0
CASES = [(1, 1, 1), (255, 63, 2), (256, 64, 8), (257, 65, 9), (1000, 130, 32)]


def _cuda(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).cuda()           # (a copy: the cached inputs are read-only)


def _padded(x, ld, fill=1e6):
    """(T, n) -> (T, ld) with `fill` in the cells that are no part of x"""
    out = np.full((x.shape[0], ld), fill)
    out[:, :x.shape[1]] = x
    return out


# ------------------------------------------------------------------------------------------------------------------ offset
@pytest.mark.parametrize("T, nloc, K", CASES)
def test_offset_is_the_host_loop_bit_for_bit(T, nloc, K):
    import torch
    from pyglm_amd._lib import call, ptr
    rng = np.random.default_rng(T + nloc + K)
    S = rng.standard_normal((T, K)) * 10.0 ** rng.integers(-2, 3, size=(T, K))
    beta = rng.standard_normal((nloc, K))
    ldn, lds = nloc + 3, K + 2
    Bt = np.full((K, ldn), 1e6)
    Bt[:, :nloc] = beta.T
    Off = torch.full((T * ldn + GUARD,), GARBAGE, dtype=torch.float64, device="cuda")
    Sd, Bd = _cuda(_padded(S, lds)), _cuda(Bt)                          # (named: they live until the launch has run)
    call("pgl_covariate_offset", S=ptr(Sd), lds=lds, Beta=ptr(Bd), Off=ptr(Off), ldn=ldn, T=T, nloc=nloc, K=K, hip_stream=None)
    torch.cuda.synchronize()
    got = Off[:T * ldn].cpu().numpy().reshape(T, ldn)
    np.testing.assert_array_equal(got[:, :nloc], cov.offset_host(S, beta))
    assert np.all(got[:, nloc:] == GARBAGE) and bool((Off[T * ldn:] == GARBAGE).all()), "cells outside the T x nloc block were written"


# ------------------------------------------------------------------------------------------------------------------ fold
@functools.lru_cache(maxsize=None)
def _fold_inputs(T, N, K, salt=0):
    rng = np.random.default_rng(7 * T + 3 * N + K + 1000 * salt)
    d = dict(S=rng.standard_normal((T, K)), Psi=rng.standard_normal((T, N)) * 2, bias=rng.standard_normal(N), Omega=rng.uniform(0.02, 0.25, (T, N)),
             Kappa=rng.standard_normal((T, N)), Off=rng.standard_normal((T, N)))
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _fold_reference(T, N, K, salt=0):
    """long-double (Lambda (N, P), r (N, K)) and their bounds' magnitudes (sum |w S_j S_k|, sum |S_k| (|Kappa| + |w| (|o| + |psi_net|)))"""
    d = _fold_inputs(T, N, K, salt)
    psi_net = d["Psi"].astype(LD) + d["bias"].astype(LD)
    Lam, r = cov.covariate_stats_host(d["S"], d["Omega"], d["Kappa"], d["Off"], psi_net, dtype=LD)
    aS = np.abs(d["S"])
    mL = np.einsum("tn,tj,tk->njk", d["Omega"], aS, aS)
    mr = np.einsum("tn,tk->nk", np.abs(d["Kappa"]) + d["Omega"] * (np.abs(d["Off"]) + np.abs(psi_net.astype(np.float64))), aS)
    return cov.tri_pack(Lam), r, cov.tri_pack(mL), mr


def _fold(sets, K, cols=None):
    """pgl_covariate_fold over the data sets `sets` (dicts of _fold_inputs), accumulate = 1 behind the first; cols = (lo, hi): the shard of
    those columns through offset pointers -> (Lambda (nloc, P), r (nloc, K)).  Checks that nothing is written behind Lambda, r or work."""
    import torch
    from pyglm_amd._lib import call, load, ptr
    N = sets[0]["Psi"].shape[1]
    lo, hi = cols or (0, N)
    nloc, P = hi - lo, K * (K + 1) // 2
    ldn, lds = N + 2, K + 1
    Lam = torch.full((nloc * P + GUARD,), GARBAGE, dtype=torch.float64, device="cuda")
    r = torch.full((nloc * K + GUARD,), GARBAGE, dtype=torch.float64, device="cuda")
    tails = []
    for i, d in enumerate(sets):
        T = d["Psi"].shape[0]
        OK = np.full((T, 2 * ldn), 1e6)
        OK[:, :N], OK[:, ldn:ldn + N] = d["Omega"], d["Kappa"]
        Psi, Off, OKd, Sd = _cuda(_padded(d["Psi"], ldn)), _cuda(_padded(d["Off"], ldn)), _cuda(OK), _cuda(_padded(d["S"], lds))
        bias = _cuda(d["bias"][lo:hi])
        nbytes = load().pgl_covariate_work_bytes(nloc, T, K)
        assert nbytes == max(16, 8 * -(-T // 256) * (P + K) * nloc)
        work = torch.empty(nbytes + GUARD, dtype=torch.uint8, device="cuda")
        work[nbytes:] = 0xA5
        tails.append(work[nbytes:])
        at = lambda t, extra=0: ctypes.c_void_p(t.data_ptr() + 8 * (lo + extra))
        call("pgl_covariate_fold", Psi=at(Psi), ldn=ldn, bias=ptr(bias), Omega=at(OKd), ldo=2 * ldn, Kappa=at(OKd, ldn), ldk=2 * ldn,
             Off=at(Off), S=ptr(Sd), lds=lds, T=T, nloc=nloc, K=K, Lambda=ptr(Lam), r=ptr(r), accumulate=int(i > 0), work=ptr(work), hip_stream=None)
        torch.cuda.synchronize()
    assert all(bool((t == 0xA5).all()) for t in tails), "bytes behind `work` were written"
    assert bool((Lam[nloc * P:] == GARBAGE).all()) and bool((r[nloc * K:] == GARBAGE).all()), "elements behind Lambda or r were written"
    return Lam[:nloc * P].cpu().numpy().reshape(nloc, P), r[:nloc * K].cpu().numpy().reshape(nloc, K)


def _check_fold(got, refs, T, what):
    Lam, r = got
    Lr, rr, mL, mr = refs
    eL, er = np.abs(Lam.astype(LD) - Lr), np.abs(r.astype(LD) - rr)
    bL, br = (T + 8) * U * mL, (T + 8) * U * mr
    print("%s: max err / bound: Lambda %.3f, r %.3f" % (what, float(np.max(eL / bL)), float(np.max(er / br))))
    assert np.all(eL <= bL) and np.all(er <= br)


@pytest.mark.parametrize("T, nloc, K", CASES + [(513, 64, 9)])
def test_fold_against_long_double(T, nloc, K):
    _check_fold(_fold([_fold_inputs(T, nloc, K)], K), _fold_reference(T, nloc, K), T, "fold T=%d nloc=%d K=%d" % (T, nloc, K))


def test_fold_adds_data_sets():
    K, N = 9, 65
    a, b = _fold_inputs(257, N, K), _fold_inputs(300, N, K, salt=1)
    ra, rb = _fold_reference(257, N, K), _fold_reference(300, N, K, salt=1)
    _check_fold(_fold([a, b], K), tuple(x + y for x, y in zip(ra, rb)), 257 + 300, "two data sets")


def test_fold_shard_has_the_bits_of_the_whole():
    T, N, K = 1000, 130, 32
    whole = _fold([_fold_inputs(T, N, K)], K)
    shard = _fold([_fold_inputs(T, N, K)], K, cols=(17, 81))
    np.testing.assert_array_equal(shard[0], whole[0][17:81])
    np.testing.assert_array_equal(shard[1], whole[1][17:81])


# ------------------------------------------------------------------------------------------------------------------ draw
def _ld_draw(A, rhs, z):
    """beta = A^-1 rhs + L^-T z by a Cholesky in long double (numpy.linalg has none)"""
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


def _spd(rng, K, cond):
    Q, _ = np.linalg.qr(rng.standard_normal((K, K)))
    M = (Q * np.geomspace(1.0, cond, K)).dot(Q.T)
    return 0.5 * (M + M.T)


def _draw(Lam_full, r, Lambda0, h0, z, beta0=None, status0=None):
    import torch
    from pyglm_amd._lib import call, ptr
    n, K = r.shape
    beta = torch.full((n * K + GUARD,), GARBAGE, dtype=torch.float64, device="cuda")
    if beta0 is not None:
        beta[:n * K] = _cuda(beta0).reshape(-1)
    status = torch.zeros(n + GUARD, dtype=torch.int32, device="cuda")
    if status0 is not None:
        status[:n] = _cuda(np.asarray(status0, dtype=np.int32))
    ins = [_cuda(v) for v in (cov.tri_pack(Lam_full), r, Lambda0, h0, z)]      # (named: they live until the launch has run)
    call("pgl_covariate_draw", Lambda=ptr(ins[0]), r=ptr(ins[1]), Lambda0=ptr(ins[2]), h0=ptr(ins[3]), z=ptr(ins[4]),
         Beta_out=ptr(beta), status=ptr(status), nloc=n, K=K, hip_stream=None)
    torch.cuda.synchronize()
    assert bool((beta[n * K:] == GARBAGE).all()) and bool((status[n:] == 0).all())
    return beta[:n * K].cpu().numpy().reshape(n, K), status[:n].cpu().numpy()


@pytest.mark.parametrize("K", [1, 2, 9, 32])
def test_draw_against_long_double(K):
    """nloc = 65 (the last workgroup holds one neuron), well-conditioned systems and one with kappa_2 = 1e6 (neuron 5).  The bound is
    relative to ||beta||, so it is a statement about draws whose two parts do not cancel (rounding the sum of two rounded parts alone
    costs 2^-53 (||mean|| + ||noise||), whatever computes them): r is chosen so that the mean Lambda^-1 (r + h0) is a random vector six
    times as long as the noise L^-T z.  Checked for the draw and for the mean (the run with z = 0)."""
    rng = np.random.default_rng(K)
    n = 65
    Lambda0 = _spd(rng, K, 3.0)
    h0 = rng.standard_normal(K)
    Lam = np.array([_spd(rng, K, 1e6 if (i == 5 and K > 1) else 30.0) * rng.uniform(1, 50) - Lambda0 * (i == 5) for i in range(n)])
    z = rng.standard_normal((n, K))
    r = np.empty((n, K))
    for i in range(n):
        A = Lam[i] + Lambda0
        noise = np.linalg.solve(np.linalg.cholesky(A).T, z[i])
        m = rng.standard_normal(K)
        r[i] = A.dot(m * (6 * np.linalg.norm(noise) / np.linalg.norm(m))) - h0
    beta, status = _draw(Lam, r, Lambda0, h0, z)
    mean, status0 = _draw(Lam, r, Lambda0, h0, np.zeros((n, K)))
    assert not status.any() and not status0.any()
    worst = 0.0
    for i in range(n):
        A = Lam[i] + Lambda0
        kappa = np.linalg.cond(A)
        if i == 5 and K > 1:
            assert 0.9e6 < kappa < 1.1e6
        for got, zz in ((beta[i], z[i]), (mean[i], np.zeros(K))):
            ref = _ld_draw(A, (r[i] + h0).astype(LD), zz)
            err, bound = float(np.linalg.norm(got.astype(LD) - ref)), 8 * K * U * kappa * float(np.linalg.norm(ref))
            worst = max(worst, err / bound)
            assert err <= bound, (i, err, bound)
    print("draw K=%d: max err / bound %.3f" % (K, worst))


def test_draw_flags_a_system_that_is_not_positive_definite():
    """a Lambda0 that is not positive definite: the neurons whose likelihood part makes up for it are drawn as ever, the one whose does not
    is flagged, its beta left as it was; a flag already set stays"""
    rng = np.random.default_rng(0)
    n, K = 9, 3
    Lambda0 = np.diag([-1.0, 1.0, 1.0])
    h0 = np.zeros(K)
    Lam = np.array([_spd(rng, K, 5.0) * 10 for _ in range(n)])
    Lam[4] = np.eye(K) * 1e-3
    r, z = rng.standard_normal((n, K)), rng.standard_normal((n, K))
    before = rng.standard_normal((n, K))
    st0 = np.zeros(n, dtype=np.int32)
    st0[7] = 2
    beta, status = _draw(Lam, r, Lambda0, h0, z, beta0=before, status0=st0)
    assert status.tolist() == [0, 0, 0, 0, 1, 0, 0, 2, 0]
    np.testing.assert_array_equal(beta[4], before[4])
    for i in [k for k in range(n) if k != 4]:
        A = Lam[i] + Lambda0
        ref = _ld_draw(A, r[i].astype(LD), z[i])
        assert float(np.linalg.norm(beta[i] - ref)) <= 8 * K * U * np.linalg.cond(A) * float(np.linalg.norm(ref))


# ------------------------------------------------------------------------------------------------------------------ a sweep under an offset
SW = dict(N=4, B=2, T=300, K=2, seed=31, sweep=3)
KW = dict(rho=0.4, S_w=3.0, mu_w=0.0, mu_b=-1.5, S_b=2.0)


@functools.lru_cache(maxsize=None)
def _sweep_problem(obs):
    N, B, T, K = SW["N"], SW["B"], SW["T"], SW["K"]
    rng = np.random.default_rng(17)
    basis = orc.cosine_basis(B, L=20) / 20
    if obs == "bernoulli":
        Y = (rng.random((T, N)) < 0.2).astype(float)
    elif obs == "negbin":
        Y = rng.poisson(0.6, size=(T, N)).astype(float)
    else:
        Y = rng.standard_normal((T, N))
    X = orc.convolve_with_basis(Y, basis)
    S = np.column_stack([np.sin(np.arange(T) / 9.0), rng.standard_normal(T)])
    beta = rng.standard_normal((N, K)) * 0.7
    a = rng.random((N, N)) < 0.5
    W = rng.standard_normal((N, N, B)) * 0.5 * a[:, :, None]
    b = rng.standard_normal(N) * 0.2 - 1.0
    return X, Y, S, beta, a, W, b


def _engine(obs, K, xi=2.5, eta=None):
    from pyglm_amd.engine import GibbsEngine
    X, Y, S, beta, a, W, b = _sweep_problem(obs)
    eng = GibbsEngine(SW["N"], SW["B"], obs=obs, xi=xi, n_covariates=K)
    eng.add_data(Y, X=X, **(dict(covariates=S) if K else {}))
    if eta is not None:
        eng.set_noise(eta)
    return eng


def _hyp(N):
    from pyglm_amd.engine import make_draws, prior_terms
    regs = [orc.Regression(N, SW["B"], **KW) for _ in range(N)]
    hyp = prior_terms(np.array([r.S_w for r in regs]), np.array([r.mu_w for r in regs]), np.full(N, KW["S_b"]), np.full(N, KW["mu_b"]))
    return hyp, make_draws(SW["seed"], SW["sweep"], range(N), N, N * SW["B"])


def _numpy_ll(obs, regs, X, Y, o):
    out = np.zeros(len(regs))
    for n, r in enumerate(regs):
        y, psi = Y[:, n], r.activation(X) + o[:, n]
        if obs == "gaussian":
            out[n] = np.sum(-0.5 * np.log(2 * np.pi * r.eta) - 0.5 * (y - psi) ** 2 / r.eta)
        else:
            out[n] = np.sum(r.log_c_func(y) + r.a_func(y) * psi - r.b_func(y) * np.log1p(np.exp(psi)))
    return out


@pytest.mark.parametrize("obs", ["bernoulli", "negbin", "gaussian"])
def test_sweep_under_an_offset_against_the_composed_oracle(obs):
    """(i) with an injected omega (PG models): flips equal and weights to 1e-8 against prior_stats + lkhd_stats, h reduced by
    [X, 1]' (omega * o) here, + collapsed_resample_a + resample_W.  (ii) without: Omega agrees with oracle.pg_draw at psi + o (Gaussian:
    equals 1 / eta), Kappa equals kappa - Omega * o bit for bit from that Omega (kappa: what an engine without covariates leaves),
    ll equals NumPy's at psi + o to 1e-12, and the sweep's result equals the composed oracle's on the device's own Omega."""
    N, B, T, K = SW["N"], SW["B"], SW["T"], SW["K"]
    D = N * B
    X, Y, S, beta, a, W, b = _sweep_problem(obs)
    xi, eta = 2.5, np.linspace(0.5, 2.0, N)
    o = cov.offset_host(S, beta)
    hyp, (perm, u, z) = _hyp(N)
    rho = np.full((N, N), KW["rho"])

    def oracle(oms):
        out = []
        for n in range(N):
            r = orc.Regression(N, B, obs=obs, xi=xi, eta=eta[n], **KW)
            r.a, r.W, r.b = a[n].copy(), W[n].copy(), b[n:n + 1].copy()
            J0, h0 = r.prior_stats()
            Jl, hl = r.lkhd_stats([(X, Y[:, n])], [oms[:, n]])
            p = oms[:, n] * o[:, n]
            hl[:D] -= p.dot(X.reshape(T, D))
            hl[D] -= p.sum()
            r.collapsed_resample_a(J0, h0, J0 + Jl, h0 + hl, perm[n], u[n])
            r.resample_W(J0 + Jl, h0 + hl, z[n])
            out.append(r)
        return out

    def check(res, regs, what):
        a1, W1, b1, _ = res
        for n, r in enumerate(regs):
            np.testing.assert_array_equal(a1[n], r.a, err_msg="%s: flips of row %d" % (what, n))
            np.testing.assert_allclose(W1[n], r.W, rtol=1e-8, atol=1e-10)
            np.testing.assert_allclose(b1[n], r.b[0], rtol=1e-8, atol=1e-10)

    eng = _engine(obs, K, xi=xi, eta=eta if obs == "gaussian" else None)
    eng.set_covariate_weights(beta)
    start = [orc.Regression(N, B, obs=obs, xi=xi, eta=eta[n], **KW) for n in range(N)]
    for n, r in enumerate(start):
        r.a, r.W, r.b = a[n].copy(), W[n].copy(), b[n:n + 1].copy()
    if obs != "gaussian":
        om = np.column_stack([orc.pg_draw(r.b_func(Y[:, n]), r.activation(X) + o[:, n], 99, orc.stream_id(n, 0)) for n, r in enumerate(start)])
        res = eng.sweep(a, W, b, rho, *hyp, perm, u, z, seed=SW["seed"], sweep=SW["sweep"], omega_override=[om])
        OK = eng.datasets[0].OK[:T].cpu().numpy()
        np.testing.assert_array_equal(OK[:, :N], om)
        kap = np.column_stack([r.kappa(Y[:, n]) for n, r in enumerate(start)])
        np.testing.assert_array_equal(OK[:, eng.ldn:eng.ldn + N], kap - om * o)        # (kappa = y - b(y) / 2 is exact in fp64 here)
        check(res, oracle(om), "injected omega")
    # the device's own draw
    res = eng.sweep(a, W, b, rho, *hyp, perm, u, z, seed=SW["seed"], sweep=SW["sweep"])
    OK = eng.datasets[0].OK[:T].cpu().numpy()
    Om, Kp = OK[:, :N], OK[:, eng.ldn:eng.ldn + N]
    plain = _engine(obs, 0, xi=xi, eta=eta if obs == "gaussian" else None)
    plain.sweep(a, W, b, rho, *hyp, perm, u, z, seed=SW["seed"], sweep=SW["sweep"])
    kap = plain.datasets[0].OK[:T, plain.ldn:plain.ldn + N].cpu().numpy()
    if obs == "gaussian":
        np.testing.assert_array_equal(Om, np.broadcast_to(1.0 / eta, (T, N)))
        np.testing.assert_allclose(Kp, (Y - o) / eta, rtol=1e-13, atol=1e-15)
    else:
        want = np.column_stack([orc.pg_draw(r.b_func(Y[:, n]), r.activation(X) + o[:, n], SW["seed"], orc.stream_id(n, SW["sweep"]))
                                for n, r in enumerate(start)])
        assert_pg_agree(Om, want, what="Omega at psi + o")
    np.testing.assert_array_equal(Kp, kap - Om * o)
    np.testing.assert_allclose(res[3], _numpy_ll(obs, start, X, Y, o), rtol=1e-12)
    check(res, oracle(Om), "the device's own omega")


# ------------------------------------------------------------------------------------------------------------------ nothing moved
def test_without_covariates_the_sweep_is_pgl_sweep(monkeypatch):
    """an engine with n_covariates = 0 calls pgl_sweep; the same sweep through pgl_sweep_offset with NULL, and with an array of NULL
    entries, has the same bits: state, ll, Omega and Kappa"""
    from pyglm_amd import engine as engine_mod
    N, T = SW["N"], SW["T"]
    X, Y, S, beta, a, W, b = _sweep_problem("bernoulli")
    hyp, (perm, u, z) = _hyp(N)
    rho = np.full((N, N), KW["rho"])
    eng = _engine("bernoulli", 0)
    seen = []

    def run(redirect):
        def call(name, *args, **kw):
            seen.append(name)
            if name == "pgl_sweep" and redirect is not None:
                sw, seed, sweep, st = args
                return engine_mod._lib.call("pgl_sweep_offset", sw, redirect(), seed, sweep, st)
            return engine_mod._lib.call(name, *args, **kw)
        monkeypatch.setattr(engine_mod, "call", call)
        res = eng.sweep(a, W, b, rho, *hyp, perm, u, z, seed=SW["seed"], sweep=SW["sweep"])
        return res + (eng.datasets[0].OK[:T].cpu().numpy(),)
    base = run(None)
    assert "pgl_sweep" in seen and "pgl_sweep_offset" not in seen
    for redirect in (lambda: None, lambda: (ctypes.c_void_p * 1)(None)):
        for x, y in zip(base, run(redirect)):
            np.testing.assert_array_equal(x, y)


def test_zero_weights_change_nothing():
    """K = 2, beta = 0, S arbitrary: a, W, b, ll, Omega of the K = 0 engine bit for bit; Kappa equal as values (a -0.0 may become 0.0)"""
    N, T = SW["N"], SW["T"]
    X, Y, S, beta, a, W, b = _sweep_problem("negbin")
    hyp, (perm, u, z) = _hyp(N)
    rho = np.full((N, N), KW["rho"])
    out = []
    for K in (0, 2):
        eng = _engine("negbin", K)
        res = eng.sweep(a, W, b, rho, *hyp, perm, u, z, seed=SW["seed"], sweep=SW["sweep"])
        out.append(res + (eng.datasets[0].OK[:T].cpu().numpy(),))
    for x, y in zip(*out):
        np.testing.assert_array_equal(x, y)
    assert out[0][3].shape == (N,) and np.all(out[0][1] == out[1][1])


# ------------------------------------------------------------------------------------------------------------------ the whole step
ST = dict(N=4, B=1, T=2000, K=2)


@functools.lru_cache(maxsize=None)
def _step_data():
    rng = np.random.default_rng(3)
    N, T = ST["N"], ST["T"]
    t = np.arange(T)
    S = np.column_stack([np.sin(2 * np.pi * t / 100.0), (t % 400 >= 200).astype(float)])
    bt = np.array([[1.0, -1.0], [-1.0, 1.0], [0.5, 0.5], [0.0, -1.0]])
    Y = (rng.random((T, N)) < orc.logistic(-1.5 + cov.offset_host(S, bt))).astype(float)
    return Y, S


@functools.lru_cache(maxsize=None)
def _step_data_gaussian():
    """the covariates of _step_data driving real-valued observations at noise variance 0.5"""
    _, S = _step_data()
    rng = np.random.default_rng(8)
    bt = np.array([[1.0, -1.0], [-1.0, 1.0], [0.5, 0.5], [0.0, -1.0]])
    return 0.3 + cov.offset_host(S, bt) + np.sqrt(0.5) * rng.standard_normal((ST["T"], ST["N"])), S


def _model(K=2, seed=5, obs="bernoulli", **kw):
    from pyglm_amd import models
    cls = {"bernoulli": models.SparseBernoulliGLM, "gaussian": models.SparseGaussianGLM}[obs]
    return cls(ST["N"], B=ST["B"], seed=seed, n_covariates=K, **kw)


@pytest.mark.parametrize("obs", ["bernoulli", "gaussian"])
def test_whole_step_follows_the_host_law(obs):
    """five resample_model() calls: after each, beta equals covariate_step_host fed the device's own [Omega | Kappa], the state the sweep
    left, the offset it ran under and the step's normals.  In the Gaussian model the eta step runs behind the covariate step and must
    leave beta as drawn (and eta must move).  Tolerance: the fold's bounds on Lambda and r -- r's widened by what the host's
    psi_net may differ from the device's, (D + 2) 2^-53 (sum |x w| + |b|) per cell -- carried through the solve,
    ||Lambda^-1|| (||dLambda|| ||beta|| + ||dr||), plus the draw's 8 K 2^-53 kappa_2 ||beta||."""
    N, T, K, D = ST["N"], ST["T"], ST["K"], ST["N"] * ST["B"]
    Y, S = _step_data() if obs == "bernoulli" else _step_data_gaussian()
    m = _model(obs=obs)
    m.add_data(Y, covariates=S)
    eng = m.engine
    X = eng.design_matrix(0).reshape(T, D)
    _, _, Lambda0, h0 = cov.prior_terms(K)
    aS = np.abs(S)
    moved = 0.0
    for it in range(5):
        before = m.covariate_weights
        eta_before = np.array([r.eta for r in m.regressions]) if obs == "gaussian" else None
        m.resample_model()
        if obs == "gaussian":
            assert np.all(np.array([r.eta for r in m.regressions]) != eta_before)
        got = m.covariate_weights
        OK = eng.datasets[0].OK[:T].cpu().numpy()
        Om, Kp = OK[:, :N], OK[:, eng.ldn:eng.ldn + N]
        o = cov.offset_host(S, before)
        w = (m.adjacency[:, :, None] * m.weights).reshape(N, D)
        psi_net = X.dot(w.T) + m.biases
        z = cov.covariate_draws(m.seed, m.sweeps_done - 1, range(N), K)
        want = cov.covariate_step_host([(S, Om, Kp, o, psi_net)], Lambda0, h0, z)
        Lam, r = cov.covariate_stats_host(S, Om, Kp, o, psi_net)
        dpsi = (D + 2) * U * (np.abs(X).dot(np.abs(w).T) + np.abs(m.biases))
        dL = (T + 8) * U * np.einsum("tn,tj,tk->njk", Om, aS, aS)
        dr = (T + 8) * U * np.einsum("tn,tk->nk", np.abs(Kp) + Om * (np.abs(o) + np.abs(psi_net)), aS) + np.einsum("tn,tk->nk", Om * dpsi, aS)
        for n in range(N):
            A = Lam[n] + Lambda0
            nb = np.linalg.norm(want[n])
            tol = np.linalg.norm(np.linalg.inv(A), 2) * (np.linalg.norm(dL[n]) * nb + np.linalg.norm(dr[n])) + 8 * K * U * np.linalg.cond(A) * nb
            err = np.linalg.norm(got[n] - want[n])
            print("sweep %d neuron %d: |beta - host| %.2e, tolerance %.2e" % (it, n, err, tol))
            assert err <= tol
        np.testing.assert_array_equal(eng.beta, got)
        np.testing.assert_array_equal(eng.datasets[0].Off[:, :N].cpu().numpy(), cov.offset_host(S, got))     # the offsets were rebuilt
        moved += np.abs(got - before).sum()
    assert moved > 0.1 and m.sweeps_done == 5


def test_read_outs_follow_beta_like_a_bias_shift():
    """S = 1, K = 1: o is the constant beta_n, i.e. the model without covariates at the bias b + beta.  log_likelihood(), means, the
    summary's rate_mean and the time-rescaling histogram of the two go through the same kernels at psi rounded in another order:
    equal to 1e-12 (integers: equal)."""
    N, T = ST["N"], ST["T"]
    Y, _ = _step_data()
    rng = np.random.default_rng(1)
    a = rng.random((N, N)) < 0.6
    W = rng.standard_normal((N, N, ST["B"])) * 0.4
    b, shift = rng.standard_normal(N) * 0.3 - 1.5, rng.standard_normal(N) * 0.5
    mc, m0 = _model(K=1), _model(K=0)
    mc.add_data(Y, covariates=np.ones((T, 1)))
    m0.add_data(Y)
    mc._store_rows(0, N, a, W, b)
    m0._store_rows(0, N, a, W, b + shift)
    mc.covariate_weights = shift[:, None]
    np.testing.assert_allclose(mc.log_likelihood(), m0.log_likelihood(), rtol=1e-12)
    np.testing.assert_allclose(mc.means[0], m0.means[0], rtol=1e-12)
    sc, s0 = mc.summarize(), m0.summarize()
    np.testing.assert_allclose(sc.collect(), s0.collect(), rtol=1e-12)
    np.testing.assert_allclose(sc.rate_mean[0], s0.rate_mean[0], rtol=1e-12)
    np.testing.assert_array_equal(sc.covariate_mean, shift[:, None])
    assert sc.covariate_var.shape == (N, 1) and not sc.covariate_var.any() and s0.covariate_mean.shape == (N, 0)
    tc, t0 = mc.time_rescaling(), m0.time_rescaling()
    tc.collect(), t0.collect()
    np.testing.assert_array_equal(tc.intervals, t0.intervals)
    np.testing.assert_allclose(tc.zsum_last, t0.zsum_last, rtol=1e-10)
    np.testing.assert_allclose(tc.ks_last, t0.ks_last, rtol=1e-6, atol=1e-9)
    # the conditional simulation's base comes through the same walk
    cc = mc.conditional_simulate([1], replicates=1, seed=3, stop=200)
    c0 = m0.conditional_simulate([1], replicates=1, seed=3, stop=200)
    np.testing.assert_allclose(cc.base, c0.base, rtol=1e-12, atol=1e-13)


def test_held_out_log_likelihood_against_numpy():
    N, T, B = ST["N"], ST["T"], ST["B"]
    Y, S = _step_data()
    rng = np.random.default_rng(2)
    m = _model()
    m.add_data(Y[:1500], covariates=S[:1500])
    a = rng.random((N, N)) < 0.6
    W = rng.standard_normal((N, N, B)) * 0.4
    b, beta = rng.standard_normal(N) * 0.3 - 1.5, rng.standard_normal((N, 2)) * 0.5
    m._store_rows(0, N, a, W, b)
    m.covariate_weights = beta
    Yh, Sh = Y[1500:], S[1500:]
    Xh = orc.convolve_with_basis(Yh, m.basis).reshape(len(Yh), N * B)
    psi = Xh.dot((a[:, :, None] * W).reshape(N, N * B).T) + b + cov.offset_host(Sh, beta)
    want = np.sum(Yh * psi - np.log1p(np.exp(psi)))
    np.testing.assert_allclose(m.log_likelihood(datas=[Yh], covariates=[Sh]), want, rtol=1e-12)
    m.covariate_weights = beta * 0.5                      # the cached held-out engine follows beta
    psi = psi - cov.offset_host(Sh, beta) + cov.offset_host(Sh, beta * 0.5)
    np.testing.assert_allclose(m.log_likelihood(datas=[Yh], covariates=[Sh]), np.sum(Yh * psi - np.log1p(np.exp(psi))), rtol=1e-12)
    with pytest.raises(ValueError, match="is required"):
        m.log_likelihood(datas=[Yh])


def test_two_shards_have_the_bits_of_the_whole():
    """neurons [0, 2) and [2, 4) as two models on one GPU against the whole model, three resample_model() calls: a, W, b and beta of each
    shard's rows bit for bit.  A shard model moves its own rows only, so its network step sees stale rows of the other shard: each
    shard is put on the whole model's state before every call, as the rank exchange would leave it"""
    N = ST["N"]
    Y, S = _step_data()
    whole = _model()
    parts = [_model(shard=(0, 2)), _model(shard=(2, 4))]
    for m in [whole] + parts:
        m.add_data(Y, covariates=S)
    for _ in range(3):
        st = whole.get_state()                         # (the first: a model's initial state is drawn from NumPy's global generator)
        whole.resample_model()
        for m in parts:
            m.set_state(st)
            m.resample_model()
        for lo, m in zip((0, 2), parts):
            sl = slice(lo, lo + 2)
            np.testing.assert_array_equal(m.covariate_weights[sl], whole.covariate_weights[sl])
            np.testing.assert_array_equal(m.adjacency[sl], whole.adjacency[sl])
            np.testing.assert_array_equal(m.weights[sl], whole.weights[sl])
            np.testing.assert_array_equal(m.biases[sl], whole.biases[sl])
    assert np.abs(whole.covariate_weights).min() > 0


# ------------------------------------------------------------------------------------------------------------------ recovery
def test_recovery_of_the_covariate_weights():
    """N = 4, T = 10 000, K = 2, true beta of +-1 on a sinusoid and a step; 300 sweeps, the first 100 discarded: every posterior mean lies
    within 4 posterior standard deviations of the truth (8 numbers).  The seed (tests/_covariate_engine.py: RECOVERY) was fixed after the
    same chain had been run on the CPU through covariate_step_host (CovariateOracleEngine): the first seed tried, 2024, held the criterion
    there with max |z| = 1.41."""
    from pyglm_amd import models
    R = RECOVERY
    Y, S, beta_true = recovery_problem()
    m = models.SparseBernoulliGLM(R["N"], B=1, seed=R["seed"], n_covariates=R["K"])
    m.add_data(Y, covariates=S)
    samples = []
    for it in range(R["sweeps"]):
        m.resample_model()
        if it >= R["burn"]:
            samples.append(m.covariate_weights)
    ok, zs = recovery_verdict(np.array(samples), beta_true)
    print("recovery: (mean - truth) / sd =\n%s" % np.round(zs, 2))
    assert ok
