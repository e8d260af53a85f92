"""Latent common input: a low-rank drive shared by the population and inferred with the network, with a time-parallel Gibbs step.

The external covariates (pyglm_amd/covariates.py) remove a confound that was recorded.  The one nobody recorded -- input from unobserved
neurons, a brain state, slow drift -- makes two neurons look coupled, and the spike-and-slab prior puts an edge between them.  A latent
factor is a covariate column whose values are sampled instead of given: a model has K_obs >= 0 observed covariates and 1 <= Q <= LATENT_MAX
latent ones, K = K_obs + Q <= COVARIATE_MAX, and every data set's S (T, K) on the device is [S_obs | X], the latent columns the last Q
(col0 = K_obs).  This module is the law in NumPy, which the kernels of pgl_latents.hip (include/pyglm_hip_latents.h) are held to:

    prior            x_t ~ N(0, I_Q), independent over t; X starts at zero.  The loadings C_n = beta_n[col0:] are drawn by the covariate
                     step unchanged, under latent_loading_prior = (mu, Sigma), default (0, I), joined block-diagonally with
                     covariate_prior into the one K x K prior that step takes (joint_prior).
    order            sweep (W, b | omega, beta, x); the latent step x | omega, W, b, beta; the covariate step beta | omega, W, b, x_new
                     (which rebuilds Off); eta, xi and the network as before.  The latent step runs BEFORE the covariate step, so that Off
                     still holds the offset the sweep ran under -- the covariate fold needs it to recover kappa -- and does not touch Off.
    latent step      with Omega and the REDUCED Kappa as the sweep left them, psi_net = Psi + bias at the state after the sweep and x_old
                     the latent columns the sweep ran under:
                        c[t][n]   = Kappa[t][n] + Omega[t][n] (sum_q x_old[t][q] C_n[q] - psi_net[t][n])
                        Lambda_t[j][k] = sum_n Omega[t][n] C_n[j] C_n[k]          (k <= j, packed like covariates.tri_pack)
                        r_t[q]    = sum_n C_n[q] c[t][n]
                        x_t       = A^-1 r_t + L^-T z_t,      A = I_Q + Lambda_t = L L'
                     (Kappa + Omega o_sweep is the model's kappa and o_sweep = o_obs + o_lat_old, so kappa - omega (psi_net + o_obs) =
                     Kappa + Omega (o_lat_old - psi_net): the step does not need Off.)
    normals          z_t[q] from the device's Philox stream: purpose PURPOSE_LATENT, key = seed, stream = sweep, element = elem0 + t; call q
                     yields (u0, u1) and z = sqrt(-2 log u0) cos(2 pi u1) (latent_normals_host).

    temporal prior   latent_ar = phi replaces x_t ~ N(0, I_Q), independent over t, by a stationary AR(1) process per factor; the statistics
                     stay, the draw becomes one joint Gaussian over a data set's bins (below: check_ar ... latent_ar_step_host;
                     pgl_latent_dynamics.hip).  phi = 0 is the law above, launch for launch.

X and C alone are defined only up to rotation and sign; the identifiable quantity is the common input X C' (T, N)."""
import ctypes

import numpy as np

from . import covariates as _cov
from ._lib import call, load, ptr
from .engine import I32, _StepScratch, _on_device

LATENT_MAX = 8              # pgl_latent_max(): one 8 x 8 diagonal block of the covariate fold
PURPOSE_LATENT = 6          # PGL_PURPOSE_LATENT (purposes 1 .. 5: pgl_rng.h, the dispersion header, the SBM header)


def check_count(Q, K_obs=0):
    """n_latents -> int Q, 0 <= Q <= LATENT_MAX and K_obs + Q <= COVARIATE_MAX, or a ValueError"""
    if int(Q) != Q or not 0 <= int(Q) <= LATENT_MAX:
        raise ValueError("n_latents = %r: an integer from 0 to %d is required" % (Q, LATENT_MAX))
    if int(Q) and int(K_obs) + int(Q) > _cov.COVARIATE_MAX:
        raise ValueError("n_covariates + n_latents = %d + %d: at most %d columns together" % (K_obs, Q, _cov.COVARIATE_MAX))
    return int(Q)


def joint_prior(K_obs, Q, covariate_prior=None, latent_loading_prior=None):
    """(mu (K,), Sigma (K, K)) of beta_n = [observed weights | loadings]: covariate_prior and latent_loading_prior, each (mu, Sigma) or
    None for (0, I), joined block-diagonally"""
    K = K_obs + Q
    mu, Sigma = np.zeros(K), np.zeros((K, K))
    for lo, n, prior, name in ((0, K_obs, covariate_prior, "covariate_prior"), (K_obs, Q, latent_loading_prior, "latent_loading_prior")):
        if n == 0:
            if prior is not None:
                raise ValueError("%s was given, but the model has none of its columns" % name)
            continue
        try:
            m, S, _, _ = _cov.prior_terms(n, prior)
        except ValueError as e:
            raise ValueError(str(e).replace("covariate_prior", name))
        mu[lo:lo + n], Sigma[lo:lo + n, lo:lo + n] = m, S
    return mu, Sigma


def check_latents(X, T, Q, what="set_latents"):
    """latents of one data set -> (T, Q) contiguous finite float64, or a ValueError that says what is wrong"""
    X = np.asarray(X, dtype=np.float64)
    if X.shape != (T, Q):
        raise ValueError("%s: latents of shape %s; (%d, %d) is required" % (what, X.shape, T, Q))
    if not np.all(np.isfinite(X)):
        raise ValueError("%s: latents must be finite" % what)
    return np.ascontiguousarray(X)


def latent_normals_host(seed, sweep, elem0, T, Q):
    """z (T, Q): the standard normals of the latent step as the device draws them -- Philox4x32-10, key = seed, counter = (q | PURPOSE_LATENT
    << 24, elem0 + t, sweep lo, sweep hi); words (0, 1) of call q make u0, words (2, 3) u1, z = sqrt(-2 log u0) cos(2 pi u1)"""
    from . import simulate as _sim
    z = np.empty((T, Q))
    for q in range(Q):
        w = _sim.philox_words(seed, PURPOSE_LATENT, q, elem0, sweep, T)
        u0, u1 = _sim._unit(w[:, 0], w[:, 1]), _sim._unit(w[:, 2], w[:, 3])
        z[:, q] = np.sqrt(-2.0 * np.log(u0)) * np.cos(2.0 * np.pi * u1)
    return z


def latent_stats_host(C, x_old, Omega, Kappa, psi_net, dtype=np.float64):
    """Lambda_t and r_t of ONE data set -> (Lambda (T, Q, Q), r (T, Q)), in `dtype` (np.longdouble: the reference the device fold is
    measured against).  C (N, Q) the loadings; x_old (T, Q); Omega, Kappa (the reduced one), psi_net (bias included) all (T, N)."""
    C, x = np.asarray(C, dtype=dtype), np.asarray(x_old, dtype=dtype)
    Om, Kp, p = (np.asarray(v, dtype=dtype) for v in (Omega, Kappa, psi_net))
    c = Kp + Om * (x.dot(C.T) - p)
    Lam = np.einsum("tn,nj,nk->tjk", Om, C, C)
    r = c.dot(C)
    return Lam, r


def latent_draw_host(Lam, r, z):
    """x (T, Q) = A_t^-1 r_t + L^-T z_t with A_t = I + Lam[t] = L L'.  np.linalg.LinAlgError where an A_t is not positive definite."""
    Lam, r, z = np.asarray(Lam, dtype=np.float64), np.asarray(r, dtype=np.float64), np.asarray(z, dtype=np.float64)
    x = np.empty_like(r)
    I = np.eye(r.shape[1])
    for t in range(r.shape[0]):
        L = np.linalg.cholesky(Lam[t] + I)
        y = np.linalg.solve(L, r[t])
        x[t] = np.linalg.solve(L.T, y + z[t])
    return x


def latent_step_host(C, x_old, Omega, Kappa, psi_net, z):
    """the whole step of one data set on the host -> x_new (T, Q)"""
    Lam, r = latent_stats_host(C, x_old, Omega, Kappa, psi_net)
    return latent_draw_host(Lam, r, z)


# ---- the temporal prior (include/pyglm_hip_latent_dynamics.h, pgl_latent_dynamics.hip) ------------------------------
# latent_ar = phi: per factor q and per data set x_0 ~ N(0, 1), x_t = phi_q x_{t-1} + sqrt(1 - phi_q^2) eps_t -- stationary with marginal
# variance 1, so the loadings' prior and the common-input variances keep their meaning.  With s_q = 1 - phi_q^2 a factor's prior precision
# is tridiagonal: (1 + phi_q^2) / s_q on the diagonal, 1 / s_q at t = 0 and t = T - 1 (T = 1: exactly 1), -phi_q / s_q beside it.  Lambda_t
# and r_t are the statistics above, unchanged (their derivation does not use the prior), and a data set's X | rest is N(J^-1 h, J^-1) with
# J[t][t] = Lambda_t + diag(prior diagonal at t), J[t + 1][t] = -diag(phi_q / s_q), h_t = r_t.  phi = 0 is the law above.

def check_ar(phi, Q):
    """latent_ar -> (Q,) float64 with 0 <= phi_q < 1 (None: zeros; a scalar: every factor's), or a ValueError that says what is required"""
    if phi is None:
        return np.zeros(int(Q))
    if not int(Q):
        raise ValueError("latent_ar was given, but n_latents=0")
    try:
        p = np.asarray(phi, dtype=np.float64)
    except (TypeError, ValueError):
        p = None
    if p is None or p.ndim > 1 or (p.ndim == 1 and p.shape[0] != Q) or not np.all((p >= 0.0) & (p < 1.0)):
        raise ValueError("latent_ar = %r: a scalar or a sequence of n_latents = %d numbers with 0 <= phi < 1 is required" % (phi, Q))
    return np.ascontiguousarray(np.broadcast_to(p, (int(Q),)), dtype=np.float64)


def ar_prior_blocks(T, phi):
    """the prior precision of one data set's latents -> (its diagonal (T, Q), e (Q,)): the precision of factor q is tridiagonal with
    diagonal[:, q] and e[q] beside it"""
    phi = np.atleast_1d(np.asarray(phi, dtype=np.float64))
    s = 1.0 - phi * phi
    d = np.tile((1.0 + phi * phi) / s, (int(T), 1))
    if T == 1:
        d[0] = 1.0
    elif T > 1:
        d[0] = d[-1] = 1.0 / s
    return d, -phi / s


def ar_precision_dense(Lam, phi):
    """J (T Q, T Q) of one data set, bin-major (row t Q + q), from Lam (T, Q, Q): tests"""
    Lam = np.asarray(Lam)
    T, Q = Lam.shape[0], Lam.shape[1]
    d, e = ar_prior_blocks(T, check_ar(phi, Q))
    J = np.zeros((T * Q, T * Q), dtype=Lam.dtype)
    for t in range(T):
        J[t * Q:(t + 1) * Q, t * Q:(t + 1) * Q] = Lam[t] + np.diag(d[t])
        if t + 1 < T:
            J[(t + 1) * Q:(t + 2) * Q, t * Q:(t + 1) * Q] = np.diag(e)
            J[t * Q:(t + 1) * Q, (t + 1) * Q:(t + 2) * Q] = np.diag(e)
    return J


def _chain_serial(D, E, h, z):
    """x of a block-tridiagonal chain (D (n, Q, Q), E (n - 1, Q, Q) = J[i + 1][i], h, z (n, Q)): block Cholesky forward, backward"""
    n, Q = h.shape
    Ls, Ws, ys = [], [], []
    Dt, g = D[0], h[0]
    for i in range(n):
        L = np.linalg.cholesky(Dt)
        y = np.linalg.solve(L, g)
        Ls.append(L), ys.append(y)
        if i + 1 < n:
            W = np.linalg.solve(L, E[i].T).T
            Ws.append(W)
            Dt, g = D[i + 1] - W.dot(W.T), h[i + 1] - W.dot(y)
    x = np.empty((n, Q))
    nxt = np.zeros(Q)
    for i in range(n - 1, -1, -1):
        t = ys[i] + z[i] - (Ws[i].T.dot(nxt) if i + 1 < n else 0.0)
        nxt = x[i] = np.linalg.solve(Ls[i].T, t)
    return x


def _chain_draw(D, E, h, z, seg):
    """the same chain by segments and separators (the elimination order of pgl_latent_ar_draw, which decides the map z -> x; the law is
    the same for every seg): bins seg - 1, 2 seg - 1, ... are separators, every interior is eliminated on its own (dense, which is the
    block recursion: a Cholesky factor is unique), the separators' chain is drawn likewise until it has fewer than 2 seg blocks, and
    every interior is drawn given its separators.  Only tests call it with a seg (they compare host and device on the same z), and it
    has to track ar_plan and the kernels of pgl_latent_dynamics.hip in what decides the map: group g owns bins [g seg, g seg + seg - 2],
    a chain of n < 2 seg blocks is the base, the next chain has floor(n / seg) blocks, and a separator takes its left segment's partial
    before its right segment's."""
    n, Q = h.shape
    if seg is None or n < 2 * seg:
        return _chain_serial(D, E, h, z)
    ns = n // seg
    sep = np.arange(ns) * seg + seg - 1
    Dn, hn, En = D[sep].copy(), h[sep].copy(), np.zeros((ns - 1, Q, Q))
    kept = []
    for gi in range(ns + 1):
        a, b = gi * seg, (gi * seg + seg - 2 if gi < ns else n - 1)
        m = b - a + 1
        if m <= 0:
            kept.append(None)
            continue
        JI, hI = np.zeros((m * Q, m * Q)), h[a:b + 1].reshape(-1)
        for i in range(m):
            JI[i * Q:(i + 1) * Q, i * Q:(i + 1) * Q] = D[a + i]
            if i + 1 < m:
                JI[(i + 1) * Q:(i + 2) * Q, i * Q:(i + 1) * Q] = E[a + i]
                JI[i * Q:(i + 1) * Q, (i + 1) * Q:(i + 2) * Q] = E[a + i].T
        L = np.linalg.cholesky(JI)
        BL, BR = np.zeros((m * Q, Q)), np.zeros((m * Q, Q))        # J[interior][left separator], J[interior][right separator]
        if gi >= 1:
            BL[:Q] = E[a - 1]
        if gi < ns:
            BR[-Q:] = E[b].T
        UL, UR, y = np.linalg.solve(L, BL), np.linalg.solve(L, BR), np.linalg.solve(L, hI)
        if gi < ns:                                                  # the left segment's partial first, then the right segment's
            Dn[gi] -= UR.T.dot(UR)
            hn[gi] -= UR.T.dot(y)
        if gi >= 1:
            Dn[gi - 1] -= UL.T.dot(UL)
            hn[gi - 1] -= UL.T.dot(y)
        if 1 <= gi < ns:
            En[gi - 1] = -UR.T.dot(UL)
        kept.append((a, b, L, UL, UR, y))
    xs = _chain_draw(Dn, En, hn, z[sep], seg)
    x = np.empty((n, Q))
    x[sep] = xs
    for gi, k in enumerate(kept):
        if k is None:
            continue
        a, b, L, UL, UR, y = k
        t = y + z[a:b + 1].reshape(-1)
        if gi >= 1:
            t = t - UL.dot(xs[gi - 1])
        if gi < ns:
            t = t - UR.dot(xs[gi])
        x[a:b + 1] = np.linalg.solve(L.T, t).reshape(-1, Q)
    return x


def latent_ar_draw_host(Lam, r, z, phi, seg=None):
    """x (T, Q) ~ N(J^-1 r, J^-1), J = ar_precision_dense(Lam, phi), as x = J^-1 r + M z with M M' = J^-1: a serial block-Cholesky forward
    and backward pass over the T bins.  seg >= 2: the same law eliminated by segments and separators, which is the map z -> x of
    pgl_latent_ar_draw(seg) (seg=None is the device's seg >= T).  np.linalg.LinAlgError where a pivot block is not positive definite."""
    Lam, r, z = np.asarray(Lam, dtype=np.float64), np.asarray(r, dtype=np.float64), np.asarray(z, dtype=np.float64)
    T, Q = r.shape
    if T == 0:
        return np.empty((0, Q))
    d, e = ar_prior_blocks(T, check_ar(phi, Q))
    D = Lam + d[:, :, None] * np.eye(Q)
    E = np.tile(np.diag(e), (max(T - 1, 0), 1, 1))
    return _chain_draw(D, E, r, z, seg)


def latent_ar_step_host(C, x_old, Omega, Kappa, psi_net, z, phi, seg=None):
    """the whole step of one data set under the temporal prior on the host -> x_new (T, Q)"""
    Lam, r = latent_stats_host(C, x_old, Omega, Kappa, psi_net)
    return latent_ar_draw_host(Lam, r, z, phi, seg=seg)


def common_input_host(X, C):
    """(T, N) = X C': the drive the latents give every neuron, by covariates.offset_host's rule (what the device adds to psi)"""
    return _cov.offset_host(X, C)


class _DeviceStep(_StepScratch):
    """the latent step on a GibbsEngine's GPU under either prior, with its scratch (engine._StepScratch); an engine_factory's engine brings its own"""

    def _alloc(self, T, eng):
        Q, P = eng.Q, eng.Q * (eng.Q + 1) // 2
        ar_bytes = int(load().pgl_latent_ar_scratch(T, Q, 0)) if np.any(eng.latent_ar > 0.0) else 0
        eng.reserve("latents: the step's scratch needs", 8 * T * (P + Q) + 4 + ar_bytes)
        return dict(Lam=eng._z(max(T, 1), P), r=eng._z(max(T, 1), Q), status=eng._z(1, dtype=I32), ar_bytes=ar_bytes,
                    ar=eng._z(ar_bytes // 8) if ar_bytes else None, phi=(ctypes.c_double * Q)(*eng.latent_ar))

    @_on_device
    def latent_step(self, a, W, b, seed, sweep, keep=False):
        """the module head's step right behind a sweep and BEFORE the covariate step: per data set ONE fold and ONE draw (the joint one
        where some phi_q > 0) into S -- the draw in front of the next data set's fold (Lambda and r are ONE buffer), so the launch holds
        both stages and times each itself.  Off is NOT touched: the covariate step (psi_ready=True) needs the offset the sweep ran under.
        keep=True (tests): self.last_latent_stats = [(Lambda (T, P), r (T, Q)), ...] on the host.  A bad pivot raises LinAlgError."""
        eng = self.eng
        eng._need_latents("latent_step()")
        if eng.likelihood_only or eng.design_only:
            raise ValueError("latent_step(): an engine with sweep buffers is required")
        Q, nl, c, kept, ar = eng.Q, eng.nloc, self._scratch(), [], bool(np.any(eng.latent_ar > 0.0))
        draw = "latent_ar_draw" if ar else "latent_draw"
        more = dict(phi=ctypes.cast(c.phi, ctypes.c_void_p), seg=0, scratch=ptr(c.ar), scratch_bytes=c.ar_bytes) if ar else {}
        c.status.zero_()
        eng._upload_weights(a, W, b)

        def launch(i, ds, st, first):
            h = eng._tic("latent_fold", float(ds.T) * nl)
            call("pgl_latent_fold", Psi=ptr(ds.Psi), ldn=eng.ldn, bias=ptr(eng.bias), Omega=ptr(ds.OK), ldo=2 * eng.ldn,
                 Kappa=ptr(ds.OK[:, eng.ldn:]), ldk=2 * eng.ldn, S=ptr(ds.S), lds=eng.K, col0=eng.K_obs,
                 Beta=ptr(eng.beta_dev), ldb=eng.ldn, T=ds.T, nloc=nl, Q=Q, Lambda=ptr(c.Lam), r=ptr(c.r), hip_stream=st)
            eng._toc(h)
            if keep:
                kept.append((c.Lam[:ds.T].cpu().numpy(), c.r[:ds.T].cpu().numpy()))
            h = eng._tic(draw, float(ds.T))
            call("pgl_" + draw, Lambda=ptr(c.Lam), r=ptr(c.r), z_override=None, seed=int(seed) & (2 ** 64 - 1), sweep=int(sweep) & (2 ** 64 - 1),
                 elem0=ds.elem0, S=ptr(ds.S), lds=eng.K, col0=eng.K_obs, status=ptr(c.status), T=ds.T, Q=Q, hip_stream=st, **more)
            eng._toc(h)
        eng.fold_data(None, launch, offset=False)
        if keep:
            self.last_latent_stats = kept
        if int(c.status.item()):
            raise np.linalg.LinAlgError("latent step: %s is not positive definite for some time bin (are the loadings, omega and "
                                        "the activation finite?)" % ("the latents' precision" if ar else "I + Lambda_t"))
