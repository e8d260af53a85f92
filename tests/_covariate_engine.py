"""TEST-ONLY: the oracle engine (tests/_oracle_engine.py, left as it is) with external covariates, composed on the host from the oracle's own
pieces and pyglm_amd/covariates.py.  It lets the model's side of the covariates -- where the step sits in resample_model(), the state, the
rank exchange, the read-outs -- run without a GPU, and is the CPU chain the recovery test's seed was confirmed on.  Never imported by the
product."""
import numpy as np

from oracle import pyglm_oracle as orc
from pyglm_amd import covariates as cov
from tests._oracle_engine import OracleEngine


RECOVERY = dict(N=4, T=10000, K=2, sweeps=300, burn=100, seed=2024, data_seed=7)


def recovery_problem():
    """the recovery test's data: N = 4 uncoupled Bernoulli neurons at a bias of -2, driven by a sinusoid and a step with true beta of +-1
    -> (Y (T, N), S (T, 2), beta_true (N, 2))"""
    N, T = RECOVERY["N"], RECOVERY["T"]
    rng = np.random.default_rng(RECOVERY["data_seed"])
    t = np.arange(T)
    S = np.column_stack([np.sin(2 * np.pi * t / 200.0), (t % 1000 >= 500).astype(float)])
    beta_true = np.array([[1.0, -1.0], [-1.0, 1.0], [1.0, 1.0], [-1.0, -1.0]])
    psi = -2.0 + cov.offset_host(S, beta_true)
    Y = (rng.random((T, N)) < orc.logistic(psi)).astype(float)
    return Y, S, beta_true


def recovery_verdict(samples, beta_true):
    """samples (n, N, K) after the burn-in -> (ok, z): every posterior mean within 4 posterior standard deviations of the truth"""
    mean, sd = samples.mean(axis=0), samples.std(axis=0, ddof=1)
    z = (mean - beta_true) / sd
    return bool(np.all(np.abs(z) <= 4.0)), z


class CovariateOracleEngine(OracleEngine):
    def __init__(self, N, B, n0=0, n1=None, obs="bernoulli", xi=1.0, n_covariates=0, covariate_prior=None, **kw):
        super().__init__(N, B, n0, n1, obs=obs, xi=xi, **kw)
        self.K = int(n_covariates)
        self.cov_prior = cov.prior_terms(self.K, covariate_prior)
        self.beta = np.zeros((self.nloc, self.K))
        self.S, self.off, self.last = [], [], None
        self.xi_loc = self._local_xi(xi)

    def _local_xi(self, xi):
        v = np.asarray(xi, dtype=np.float64).reshape(-1)
        if v.size == 1:
            return np.full(self.nloc, float(v[0]))
        return (v[self.n0:self.n1] if v.size == self.N else v).copy()

    def set_obs_param(self, xi):
        """one xi per local neuron, as a model that learns xi pushes it before every sweep"""
        self.xi_loc = self._local_xi(xi)

    def _reg(self, a, W, b, i, **hyp):
        r = orc.Regression(self.N, self.B, obs=self.obs, xi=float(self.xi_loc[i]), eta=self.eta[i], **hyp)
        r.a, r.W, r.b = np.asarray(a[i]).astype(bool).copy(), np.asarray(W[i], float).copy(), np.atleast_1d(np.asarray(b, float)[i]).copy()
        return r

    def add_data(self, Y, X=None, basis=None, covariates=None):
        super().add_data(Y, X=X, basis=basis)
        self.S.append(cov.check_covariates(covariates, Y.shape[0], self.K))
        self.off.append(cov.offset_host(self.S[-1], self.beta))

    def set_covariate_weights(self, beta):
        self.beta = np.asarray(beta, dtype=np.float64).reshape(self.nloc, self.K).copy()
        self.off = [cov.offset_host(S, self.beta) for S in self.S]

    def psi_net(self, a, W, b, i=0):
        return OracleEngine.psi(self, a, W, b, i)

    def psi(self, a, W, b, i=0):
        """like GibbsEngine.psi of an engine with covariates: the activation WITH the offset (the oracle's includes the bias)"""
        return self.psi_net(a, W, b, i) + self.off[i]

    def log_likelihood(self, a, W, b):
        out = np.zeros(self.nloc)
        for i in range(self.nloc):
            r = self._reg(a, W, b, i)
            for d, (X, Y) in enumerate(self.datasets):
                y, psi = Y[:, self.n0 + i], r.activation(X) + self.off[d][:, i]
                if self.obs == "gaussian":
                    out[i] += np.sum(-0.5 * np.log(2 * np.pi * r.eta) - 0.5 * (y - psi) ** 2 / r.eta)
                else:
                    out[i] += np.sum(r.log_c_func(y) + r.a_func(y) * psi - r.b_func(y) * np.log1p(np.exp(psi)))
        return out

    def sse(self, a, W, b):
        out = np.zeros(self.nloc)
        for i in range(self.nloc):
            r = self._reg(a, W, b, i)
            out[i] = sum(np.sum((Y[:, self.n0 + i] - (r.activation(X) + self.off[d][:, i])) ** 2) for d, (X, Y) in enumerate(self.datasets))
        return out

    def sweep(self, a, W, b, rho, Jw, hw, Jb, hb, c0, perm, u, z, seed, sweep, omega_override=None, host_overlap=None):
        """the sweep under the offsets: omega at psi + o, h reduced by [X, 1]' (omega * o); leaves (Omega, reduced Kappa, o) per data set in
        self.last for the covariate step"""
        a_new, W_new, b_new, ll = [], [], [], self.log_likelihood(a, W, b)
        if hasattr(Jw, "dense"):
            Jw, hw, c0 = Jw.dense()
        if host_overlap is not None:
            host_overlap()
        Om = [np.zeros((X.shape[0], self.nloc)) for X, _ in self.datasets]
        Kp = [np.zeros((X.shape[0], self.nloc)) for X, _ in self.datasets]
        D = self.D
        for i in range(self.nloc):
            S_w = np.linalg.inv(Jw[i])
            mu_w = np.einsum("mij,mj->mi", S_w, hw[i])
            r = self._reg(a, W, b, i, rho=rho[i], S_w=S_w, mu_w=mu_w, S_b=1.0 / Jb[i], mu_b=hb[i] / Jb[i])
            n = self.n0 + i
            datas, oms, e0 = [], [], 0
            J_prior, h_prior = r.prior_stats()
            dh = np.zeros(D + 1)
            for d, (X, Y) in enumerate(self.datasets):
                y, o = Y[:, n], self.off[d][:, i]
                datas.append((X, y))
                if omega_override is not None:
                    om = np.asarray(omega_override[d])[:, i]
                elif self.obs == "gaussian":
                    om = r.omega_gaussian(X.shape[0])
                else:
                    om = orc.pg_draw(r.b_func(y), r.activation(X) + o, seed, orc.stream_id(n, sweep), e0)
                e0 += X.shape[0]
                oms.append(om)
                p = om * o
                Om[d][:, i], Kp[d][:, i] = om, r.kappa(y) - p
                dh[:D] += p.dot(r.flat(X))
                dh[D] += p.sum()
            J_l, h_l = r.lkhd_stats(datas, oms)
            J_post, h_post = J_prior + J_l, h_prior + h_l - dh
            if r.deterministic_sparsity():
                r.a = np.round(r.rho).astype(bool)
            else:
                r.collapsed_resample_a(J_prior, h_prior, J_post, h_post, perm[i], u[i])
            r.resample_W(J_post, h_post, z[i])
            a_new.append(r.a)
            W_new.append(r.W)
            b_new.append(r.b[0])
        self.last = (Om, Kp, [o.copy() for o in self.off])
        return np.array(a_new), np.array(W_new), np.array(b_new), ll

    def covariate_step(self, a, W, b, seed, sweep):
        Om, Kp, off = self.last
        sets = [(self.S[d], Om[d], Kp[d], off[d], self.psi_net(a, W, b, d)) for d in range(len(self.datasets))]
        z = cov.covariate_draws(seed, sweep, range(self.n0, self.n1), self.K)
        beta = cov.covariate_step_host(sets, self.cov_prior[2], self.cov_prior[3], z)
        self.set_covariate_weights(beta)
        return beta
