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

X and C alone are defined only up to rotation and sign; the identifiable quantity is the common input X C' (T, N)."""
import numpy as np

from . import covariates as _cov

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


def common_input_host(X, C):
    """(T, N) = X C': the drive the latents give every neuron, by covariates.offset_host's rule (what the device adds to psi)"""
    return _cov.offset_host(X, C)
