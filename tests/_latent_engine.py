"""TEST-ONLY: the oracle engine with covariates (tests/_covariate_engine.py, left as it is) plus latent common input, composed on the host from
pyglm_amd/latents.py.  It lets the model's side of the latents -- where the step sits in resample_model(), the state, the read-outs, the
refusals -- run without a GPU, and is the CPU chain the recovery comparisons were confirmed on.  Never imported by the product."""
import numpy as np

from pyglm_amd import covariates as cov
from pyglm_amd import latents as lat
from tests._covariate_engine import CovariateOracleEngine


RECOVERY = dict(N=16, T=800, B=1, sweeps=50, burn=20, seed=11, data_seed=5, smooth=3, loading=1.5, bias=-1.0)


def recovery_problem():
    """two populations of 8 Bernoulli neurons with NO coupling, both driven by one common input nobody recorded (Gaussian noise smoothed over
    3 bins, unit variance: the previous bin of every other neuron says something about it) with loadings of opposite sign in the two
    populations -> (Y (T, N), drive (T,), loadings (N,))"""
    N, T, sm = RECOVERY["N"], RECOVERY["T"], RECOVERY["smooth"]
    rng = np.random.default_rng(RECOVERY["data_seed"])
    g = np.convolve(rng.standard_normal(T + 2 * sm), np.ones(sm) / np.sqrt(sm), mode="valid")[:T]
    g = (g - g.mean()) / g.std()
    load = np.r_[np.full(N // 2, RECOVERY["loading"]), np.full(N - N // 2, -RECOVERY["loading"])]
    psi = RECOVERY["bias"] + g[:, None] * load[None, :]
    Y = (rng.random((T, N)) < 1.0 / (1.0 + np.exp(-psi))).astype(float)
    return Y, g, load


def recovery_model(Q, **kw):
    """the model of the recovery comparisons with Q latents (kw: engine_factory= for the CPU chain, device= for the GPU one)"""
    from pyglm_amd import models
    return models.SparseBernoulliGLM(RECOVERY["N"], B=RECOVERY["B"], seed=RECOVERY["seed"], regression_kwargs=dict(S_w=2.0, mu_b=RECOVERY["bias"]),
                                     **(dict(n_latents=Q) if Q else {}), **kw)


def recovery_run(model, Y):
    """the chain of the recovery comparisons -> (edge probability (N, N), mean common input (T, N) or None) over the kept sweeps"""
    np.random.seed(RECOVERY["seed"])                     # (the default network draws its initial state from NumPy's global generator)
    model.add_data(Y)
    edge, common, kept = 0.0, 0.0, 0
    for it in range(RECOVERY["sweeps"]):
        model.resample_model()
        if it >= RECOVERY["burn"]:
            edge = edge + model.adjacency
            if model.Q:
                common = common + model.common_input()
            kept += 1
    return edge / kept, (common / kept if model.Q else None)


def between_within(P):
    """mean edge probability (between the two populations, within one, the diagonal left out)"""
    N = P.shape[0]
    across = np.zeros((N, N), dtype=bool)
    across[:N // 2, N // 2:] = across[N // 2:, :N // 2] = True
    within = ~across & ~np.eye(N, dtype=bool)
    return float(P[across].mean()), float(P[within].mean())


def recovery_verdict(P0, P1, common, Y, drive, load):
    """the comparisons, stated once for the CPU and the GPU chain -> (ok, figures): the between-population edge probability with one latent
    is below that without; the mean common input of every neuron correlates with its true drive, positively and better than any single
    neuron's spike train does with the drive it follows"""
    b0, b1 = between_within(P0)[0], between_within(P1)[0]
    truth = drive[:, None] * load[None, :]
    c_lat = np.array([np.corrcoef(common[:, n], truth[:, n])[0, 1] for n in range(Y.shape[1])])
    c_spk = np.array([abs(np.corrcoef(Y[:, n], drive)[0, 1]) for n in range(Y.shape[1])])
    fig = dict(between_0=b0, between_1=b1, corr_common=c_lat.tolist(), corr_spikes=c_spk.tolist())
    return bool(b1 < b0 and c_lat.min() > 0 and c_lat.min() > c_spk.max()), fig


class LatentOracleEngine(CovariateOracleEngine):
    def __init__(self, N, B, n0=0, n1=None, obs="bernoulli", xi=1.0, n_covariates=0, covariate_prior=None, n_latents=0, **kw):
        super().__init__(N, B, n0, n1, obs=obs, xi=xi, n_covariates=int(n_covariates) + int(n_latents), covariate_prior=covariate_prior, **kw)
        self.K_obs, self.Q = int(n_covariates), int(n_latents)

    def add_data(self, Y, X=None, basis=None, covariates=None):
        T = Y.shape[0]
        S_obs = cov.check_covariates(covariates, T, self.K_obs)
        S = np.zeros((T, self.K))
        if self.K_obs:
            S[:, :self.K_obs] = S_obs
        super().add_data(Y, X=X, basis=basis, covariates=S if self.K else None)

    def latents(self, i=0):
        return self.S[i][:, self.K_obs:].copy()

    def set_latents(self, i, X):
        S = self.S[i].copy()
        S[:, self.K_obs:] = lat.check_latents(X, S.shape[0], self.Q)
        self.S[i] = S
        self.off[i] = cov.offset_host(S, self.beta)

    def latent_step(self, a, W, b, seed, sweep, keep=False):
        """x | omega, W, b, beta from what the last sweep left; the offsets (self.off, and the ones kept in self.last) stay as they are"""
        Om, Kp, _ = self.last
        e0, C = 0, self.beta[:, self.K_obs:]
        self.last_latent = []
        for d in range(len(self.datasets)):
            T = self.S[d].shape[0]
            z = lat.latent_normals_host(seed, sweep, e0, T, self.Q)
            x_old, psi_net = self.S[d][:, self.K_obs:], self.psi_net(a, W, b, d)
            S = self.S[d].copy()
            S[:, self.K_obs:] = lat.latent_step_host(C, x_old, Om[d], Kp[d], psi_net, z)
            self.last_latent.append((x_old.copy(), psi_net, z))
            self.S[d] = S
            e0 += T

    def covariate_step(self, a, W, b, seed, sweep, keep=False, psi_ready=False):
        return super().covariate_step(a, W, b, seed, sweep)
