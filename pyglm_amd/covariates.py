"""External covariates: stimulus regressors shared by all neurons, with a Gibbs step of their own.

The reference explains a neuron from the population's spike history and a constant bias; nothing that happened outside the recorded
population can enter.  This is the project's own extension (like xi and the learned network priors): data set i carries covariates S_i
(T_i, K), fp64, 1 <= K <= COVARIATE_MAX, given by the user as they are (a stimulus filter is passed as lagged copies); neuron n has weights
beta_n in R^K with the prior beta_n ~ N(mu0, Sigma0), the same for every neuron.  This module is the law in NumPy, which the kernels of
pgl_covariates.hip (include/pyglm_hip_covariates.h) are held to:

    offset           o[t][n] = sum_{k = 0 .. K-1} S[t][k] * beta_n[k], from 0.0, k ascending, a rounded product and a rounded sum per term
                     (offset_host; the device equals it bit for bit), and psi = X . vec(a * W) + b + o.
    sweep            omega is drawn at psi including o; then Kappa <- Kappa - Omega * o (one product, one difference); the ll returned is the
                     one at psi including o.  With psi = psi_net + o the augmented likelihood in (W, b) is the usual one with kappa
                     replaced by kappa - omega * o, so the Gram, the flips and the weight draw never see the covariates.
    covariate step   beta_n | omega, W, b, right after the sweep, from the omega the sweep has just drawn (a systematic-scan Gibbs step):
                        Lambda_n = Lambda0 + sum_i sum_t Omega[t][n] S[t] S[t]'
                        r_n      = Lambda0 mu0 + sum_i sum_t S[t] (Kappa[t][n] + Omega[t][n] (o[t][n] - psi_net[t][n]))
                        beta_n   = Lambda_n^-1 r_n + L^-T z_n,    Lambda_n = L L'
                     Kappa is the REDUCED one the sweep left, o the offset that sweep ran under, psi_net = X . vec(a * W) + b at the state
                     after the sweep (Kappa + Omega o is the model's own kappa again; kappa - omega psi_net is what is left for S beta to
                     explain).  z_n: K standard normals keyed like engine.make_draws by (seed, sweep, GLOBAL neuron) on counter lane 3
                     (covariate_draws), so a neuron's beta does not depend on the shard.
"""
import numpy as np
import torch

from ._lib import call, load, ptr
from .engine import I32, _StepScratch, _on_device

COVARIATE_MAX = 32          # pgl_covariate_max()
COV_LANE = 3                # the Philox counter lane of z_n (lanes 1 and 2: the noise variance eta and the dispersion xi)


def check_count(K):
    """n_covariates -> int K, 0 <= K <= COVARIATE_MAX, or a ValueError"""
    if int(K) != K or not 0 <= int(K) <= COVARIATE_MAX:
        raise ValueError("n_covariates = %r: an integer from 0 to %d is required" % (K, COVARIATE_MAX))
    return int(K)


def check_covariates(S, T, K, what="add_data"):
    """the covariates of one data set of T bins for a model of K covariates -> (T, K) contiguous float64, or a ValueError that says what is
    wrong: any S with K = 0, a missing S with K > 0, another shape, a value that is not finite"""
    if K == 0:
        if S is not None:
            raise ValueError("%s: covariates were given, but the model was built with n_covariates=0" % what)
        return None
    if S is None:
        raise ValueError("%s: the model was built with n_covariates=%d; covariates=S of shape (%d, %d) is required" % (what, K, T, K))
    S = np.asarray(S, dtype=np.float64)
    if S.shape != (T, K):
        raise ValueError("%s: covariates of shape %s; (%d, %d) is required" % (what, S.shape, T, K))
    if not np.all(np.isfinite(S)):
        raise ValueError("%s: covariates must be finite" % what)
    return np.ascontiguousarray(S)


def prior_terms(K, prior=None):
    """covariate_prior = (mu0 (K,), Sigma0 (K, K)) or None (mu0 = 0, Sigma0 = I) -> (mu0, Sigma0, Lambda0 = Sigma0^-1, h0 = Lambda0 mu0).
    Sigma0 must be symmetric; that it is positive definite is NOT checked here: the draw's status flag reports it (a LinAlgError at the
    first covariate step), as the sweep's flags report a bad weight prior."""
    if prior is None:
        mu0, Sigma0 = np.zeros(K), np.eye(K)
    else:
        mu0 = np.array(np.broadcast_to(np.asarray(prior[0], dtype=np.float64), (K,)))
        Sigma0 = np.array(prior[1], dtype=np.float64)
        if Sigma0.ndim == 0:
            Sigma0 = float(Sigma0) * np.eye(K)
        if Sigma0.shape != (K, K) or not np.allclose(Sigma0, Sigma0.T):
            raise ValueError("covariate_prior: Sigma0 must be a symmetric (%d, %d) matrix" % (K, K))
    Lambda0 = np.linalg.inv(Sigma0)
    Lambda0 = 0.5 * (Lambda0 + Lambda0.T)
    return mu0, Sigma0, Lambda0, Lambda0.dot(mu0)


def covariate_draws(seed, sweep, neuron_ids, K):
    """z (len(neuron_ids), K): the standard normals of the covariate step, keyed like engine.make_draws on counter lane COV_LANE"""
    z = np.empty((len(neuron_ids), K))
    for i, n in enumerate(neuron_ids):
        rng = np.random.Generator(np.random.Philox(key=int(seed) & (2 ** 64 - 1), counter=[int(sweep), int(n), COV_LANE, 0]))
        z[i] = rng.standard_normal(K)
    return z


def offset_host(S, beta):
    """o (T, N) = S (T, K) . beta (N, K)' by the rule of the module's head: from 0.0, k ascending, product and sum rounded one after the other"""
    S, beta = np.asarray(S, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    o = np.zeros((S.shape[0], beta.shape[0]))
    for k in range(S.shape[1]):
        o = o + S[:, k:k + 1] * beta[None, :, k]
    return o


def tri_pack(M):
    """(n, K, K) symmetric -> (n, K (K + 1) / 2): the lower triangle row by row, entry (j, k <= j) at j (j + 1) / 2 + k -- the layout of
    pgl_covariate_fold's Lambda"""
    j, k = np.tril_indices(M.shape[-1])
    return np.ascontiguousarray(M[..., j, k])


def tri_unpack(P, K):
    """the inverse of tri_pack: (n, K (K + 1) / 2) -> (n, K, K) symmetric"""
    P = np.asarray(P)
    j, k = np.tril_indices(K)
    M = np.zeros(P.shape[:-1] + (K, K), dtype=P.dtype)
    M[..., j, k] = P
    M[..., k, j] = P
    return M


def covariate_stats_host(S, Omega, Kappa, off, psi_net, dtype=np.float64):
    """the likelihood parts of Lambda_n and r_n of ONE data set -> (Lambda (N, K, K), r (N, K)), in `dtype` (np.longdouble: the reference
    the device fold is measured against).  S (T, K); Omega, Kappa (the reduced one), off, psi_net (bias included) all (T, N)."""
    S = np.asarray(S, dtype=dtype)
    Om, Kp, o, p = (np.asarray(v, dtype=dtype) for v in (Omega, Kappa, off, psi_net))
    c = Kp + Om * (o - p)
    Lam = np.einsum("tn,tj,tk->njk", Om, S, S)
    r = np.einsum("tn,tk->nk", c, S)
    return Lam, r


def covariate_draw_host(Lam, r, Lambda0, h0, z):
    """beta (N, K) = Lambda_n^-1 r_n + L^-T z_n with Lambda_n = Lambda0 + Lam[n] = L L', r_n = h0 + r[n].  np.linalg.LinAlgError where a
    Lambda_n is not positive definite."""
    Lam, r, z = np.asarray(Lam, dtype=np.float64), np.asarray(r, dtype=np.float64), np.asarray(z, dtype=np.float64)
    beta = np.empty_like(r)
    for n in range(r.shape[0]):
        L = np.linalg.cholesky(Lam[n] + Lambda0)
        y = np.linalg.solve(L, r[n] + h0)
        beta[n] = np.linalg.solve(L.T, y + z[n])
    return beta


def covariate_step_host(datasets, Lambda0, h0, z):
    """the whole step on the host: datasets = [(S, Omega, Kappa, off, psi_net), ...], one tuple per data set as covariate_stats_host takes
    them, added in the order given -> beta (N, K)"""
    Lam = r = None
    for d in datasets:
        Li, ri = covariate_stats_host(*d)
        Lam, r = (Li, ri) if Lam is None else (Lam + Li, r + ri)
    return covariate_draw_host(Lam, r, Lambda0, h0, z)


class _DeviceStep(_StepScratch):
    """the covariate step on a GibbsEngine's GPU, with its scratch (engine._StepScratch); an engine_factory's engine brings its own"""

    def _alloc(self, T, eng):
        K, nl, P = eng.K, eng.nloc, eng.K * (eng.K + 1) // 2
        need = load().pgl_covariate_work_bytes(nl, T, K)
        eng.reserve("covariates: the step's scratch needs", need + 8 * nl * (P + 3 * K) + 4 * nl + 8 * K * (K + 1))
        Lambda0, h0 = (torch.from_numpy(np.ascontiguousarray(v)).to(eng.dev) for v in eng.cov_prior[2:])
        return dict(work=torch.empty(need, dtype=torch.uint8, device=eng.dev), Lam=eng._z(nl, P), r=eng._z(nl, K), z=eng._z(nl, K),
                    beta=eng._z(nl, K), status=eng._z(nl, dtype=I32), Lambda0=Lambda0, h0=h0)

    @_on_device
    def covariate_step(self, a, W, b, seed, sweep, keep=False, psi_ready=False):
        """the module head's step right behind a sweep -> the new beta (nloc, K), the offsets rebuilt from it; a Lambda_n that is not positive
        definite raises LinAlgError naming the neurons and leaves both.  keep=True (tests): self.last_covariate_stats = (Lambda (nloc, K (K + 1)
        / 2), r (nloc, K), z) on the host.  psi_ready=True: Psi and the device's weights are at (a, W, b) (the latent step has just run)."""
        eng = self.eng
        if not eng.K or eng.likelihood_only or eng.design_only:
            raise ValueError("covariate_step(): an engine with n_covariates > 0 and sweep buffers is required")
        K, nl, c = eng.K, eng.nloc, self._scratch()
        z = covariate_draws(seed, sweep, range(eng.n0, eng.n1), K)
        c.z.copy_(torch.from_numpy(z)), c.status.zero_(), c.beta.copy_(torch.from_numpy(eng.beta))
        if not psi_ready:
            eng._upload_weights(a, W, b)
        st = eng.fold_data("covariate_fold", lambda i, ds, st, first: call(
            "pgl_covariate_fold", Psi=ptr(ds.Psi), ldn=eng.ldn, bias=ptr(eng.bias), Omega=ptr(ds.OK), ldo=2 * eng.ldn,
            Kappa=ptr(ds.OK[:, eng.ldn:]), ldk=2 * eng.ldn, Off=ptr(ds.Off), S=ptr(ds.S), lds=K, T=ds.T, nloc=nl, K=K,
            Lambda=ptr(c.Lam), r=ptr(c.r), accumulate=int(not first), work=ptr(c.work), hip_stream=st), offset=False, activate=not psi_ready)
        h = eng._tic("covariate_draw")
        call("pgl_covariate_draw", Lambda=ptr(c.Lam), r=ptr(c.r), Lambda0=ptr(c.Lambda0), h0=ptr(c.h0), z=ptr(c.z), Beta_out=ptr(c.beta),
             status=ptr(c.status), nloc=nl, K=K, hip_stream=st)
        eng._toc(h)
        bad = np.nonzero(c.status.cpu().numpy())[0]
        if keep:
            self.last_covariate_stats = (c.Lam.cpu().numpy(), c.r.cpu().numpy(), z)
        if bad.size:
            err = np.linalg.LinAlgError("covariate step: Lambda_n is not positive definite for neurons %s (is covariate_prior's Sigma0 "
                                        "positive definite?)" % ((bad[:8] + eng.n0).tolist(),))
            err.neurons, err.beta = (bad + eng.n0).tolist(), c.beta.cpu().numpy()
            raise err
        eng.beta_dev[:, :nl].copy_(c.beta.t())           # (into the k-major array the offset kernel reads: a strided device copy)
        h = eng._tic("covariate_offset")
        for ds in eng.datasets:
            eng._offset(ds, st)
        eng._toc(h)
        eng.beta = c.beta.cpu().numpy()
        return eng.beta.copy()
