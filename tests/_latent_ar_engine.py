"""TEST-ONLY: the oracle engine with latents (tests/_latent_engine.py, left as it is) under the temporal prior of pyglm_amd/latents.py: its
latent step is latent_ar_step_host.  The CPU chain of the AR(1) latents, and the one the recovery comparison's seed was settled on.  Never
imported by the product."""
import numpy as np

from pyglm_amd import latents as lat
from tests._latent_engine import RECOVERY, LatentOracleEngine

AR_RECOVERY = dict(phi_true=0.98, phi=0.95, drive_seed=17)


def ar_recovery_problem():
    """the two-population problem of tests/_latent_engine.py (same sizes, loadings, bias) with the drive replaced by a stationary AR(1)
    process, phi_true = 0.98, unit variance -> (Y (T, N), drive (T,), loadings (N,))"""
    N, T, phi = RECOVERY["N"], RECOVERY["T"], AR_RECOVERY["phi_true"]
    rng = np.random.default_rng(AR_RECOVERY["drive_seed"])
    g = np.empty(T)
    g[0] = rng.standard_normal()
    for t in range(1, T):
        g[t] = phi * g[t - 1] + np.sqrt(1.0 - phi * phi) * rng.standard_normal()
    load = np.r_[np.full(N // 2, RECOVERY["loading"]), np.full(N - N // 2, -RECOVERY["loading"])]
    psi = RECOVERY["bias"] + g[:, None] * load[None, :]
    Y = (rng.random((T, N)) < 1.0 / (1.0 + np.exp(-psi))).astype(float)
    return Y, g, load


def ar_recovery_model(latent_ar, **kw):
    """the model of tests/_latent_engine.recovery_model with one latent and the given latent_ar (None: independent bins)"""
    from pyglm_amd import models
    return models.SparseBernoulliGLM(RECOVERY["N"], B=RECOVERY["B"], seed=RECOVERY["seed"], regression_kwargs=dict(S_w=2.0, mu_b=RECOVERY["bias"]),
                                     n_latents=1, latent_ar=latent_ar, **kw)


def ar_recovery_corr(common, drive, load):
    """the correlation of the posterior-mean common input with the true drive, over all (bin, neuron) cells"""
    truth = drive[:, None] * load[None, :]
    return float(np.corrcoef(common.ravel(), truth.ravel())[0, 1])


class LatentAROracleEngine(LatentOracleEngine):
    def __init__(self, N, B, n0=0, n1=None, latent_ar=None, n_latents=0, **kw):
        super().__init__(N, B, n0, n1, n_latents=n_latents, **kw)
        self.latent_ar = lat.check_ar(latent_ar, self.Q)

    def latent_step(self, a, W, b, seed, sweep, keep=False):
        """x | omega, W, b, beta under the AR(1) prior from what the last sweep left; the offsets stay as they are"""
        Om, Kp, _ = self.last
        e0, C = 0, self.beta[:, self.K_obs:]
        self.last_latent = []
        for d in range(len(self.datasets)):
            T = self.S[d].shape[0]
            z = lat.latent_normals_host(seed, sweep, e0, T, self.Q)
            x_old, psi_net = self.S[d][:, self.K_obs:], self.psi_net(a, W, b, d)
            S = self.S[d].copy()
            S[:, self.K_obs:] = lat.latent_ar_step_host(C, x_old, Om[d], Kp[d], psi_net, z, self.latent_ar)
            self.last_latent.append((x_old.copy(), psi_net, z))
            self.S[d] = S
            e0 += T
