"""Hierarchical priors on the (adjacency, weight) network -- host side, with the reference's class names and interface
(pyglm/networks.py).  These touch only O(N^2 B) sufficient statistics per sweep, so they stay in NumPy; what matters for
the hot path is that their outputs (rho, mu_W, sigma_W) are handed to the regressions without the reference's
O(N^3 B^2) per-row rebuilds (networks.py:96-130 are re-evaluated N times at models.py:233-236).

`pybasicbayes.distributions.Gaussian` (NIW) is not vendored with the reference; `_NIW` restates its published conjugate
update and draw (PARITY UNPINNED against the third-party package, see oracle/pyglm_oracle.py).
"""
import warnings

import numpy as np
from scipy.linalg.lapack import dtrtrs

from .utils.utils import expand_scalar, expand_cov

# True (default): the network classes are constructed exactly as the reference constructs them, including three accidents of its code
# that decide the results a `network_kwargs` user gets (pinned by fixture G12, captured from the reference's own constructors):
#   * the mixins chain through `super().__init__(N, B)` (networks.py:83, 180, 196), so of all keyword arguments only `rho` / `rho_self`
#     (sparse networks) ever arrive: the NIW hyper-parameters are always the defaults mu_0 = 0, sigma_0 = I, kappa_0 = 1, nu_0 = 3, and a
#     FixedMean network always has mu = 0;
#   * the self-connection Gaussian gets nu_0 raw (networks.py:94) where the shared one gets max(nu_0, B + 2) (:89);
#   * `_FixedWeightsMixin` builds its covariance from `mu` (networks.py:159), i.e. Sigma = 0.
# Where that leaves the reference unable to run at all (nu_0 = 3 < B: pybasicbayes' inverse-Wishart draw fails for B > 3; Sigma = 0: the
# regressions cannot invert it) the first is floored at B + 2 with a warning and the second raises like the reference does.
# False: keyword arguments reach the mixin they are meant for, both Gaussians get max(nu_0, B + 2), Sigma comes from `sigma`.
REFERENCE_QUIRKS = True


def set_reference_quirks(on):
    """switch the constructor behaviour described above (module-wide; affects networks constructed afterwards)"""
    global REFERENCE_QUIRKS
    REFERENCE_QUIRKS = bool(on)


def _dropped(cls, kw, keep=()):
    lost = sorted(k for k in kw if k not in keep)
    if lost:
        warnings.warn("%s: keyword argument(s) %s never reach their mixin in the reference (pyglm/networks.py:83, 180, 196) and are ignored "
                      "here too; pyglm_amd.networks.set_reference_quirks(False) makes them take effect" % (cls, ", ".join(lost)), stacklevel=3)


def _sample_invwishart(S, nu, rng):
    n = S.shape[0]
    chol = np.linalg.cholesky(S)
    if (nu <= 81 + n) and (nu == np.round(nu)):
        x = rng.randn(int(nu), n)
    else:
        x = np.diag(np.sqrt(np.atleast_1d(rng.chisquare(nu - np.arange(n)))))
        x[np.triu_indices_from(x, 1)] = rng.randn(n * (n - 1) // 2)
    R = np.linalg.qr(x, "r")
    # (LAPACK's triangular solve called directly: scipy.linalg.solve_triangular is the same routine behind ~0.3 ms of argument checking,
    # which at BASELINE configs[0] was a quarter of a sweep)
    T, info = dtrtrs(np.ascontiguousarray(R.T), np.ascontiguousarray(chol.T), lower=1)
    if info != 0:
        raise np.linalg.LinAlgError("inverse-Wishart draw: singular triangular factor")
    T = T.T
    return T.dot(T.T)


def _mvn(rng, mean, cov):
    """rng.multivariate_normal(mean, cov) of NumPy's legacy generator, restated: standard_normal(d) pushed through the SVD factor of the
    covariance (numpy/random/mtrand.pyx: x = z . (sqrt(s)[:, None] v) + mean) -- the same numbers from the same stream, without the
    50 us of argument handling per call"""
    mean = np.asarray(mean, dtype=float)
    z = rng.standard_normal(mean.shape[0])
    _, sv, v = np.linalg.svd(cov)
    return mean + np.dot(z, np.sqrt(sv)[:, None] * v)


def _take(W, mask):
    """W[mask] for W (N, N, B), mask (N, N) bool -- the same rows in the same order, three times faster than boolean indexing"""
    return np.ascontiguousarray(W).reshape(-1, W.shape[-1]).take(np.flatnonzero(mask), axis=0)


class _NIW(object):
    """Gaussian with a normal-inverse-Wishart prior: resample(data) draws (mu, sigma) from the posterior."""

    def __init__(self, mu_0, sigma_0, kappa_0, nu_0, rng=None):
        self.mu_0, self.sigma_0 = np.asarray(mu_0, float), np.asarray(sigma_0, float)
        self.kappa_0, self.nu_0 = float(kappa_0), float(nu_0)
        self.rng = rng                     # None = NumPy's global generator (looked up at use: a module cannot be deep-copied)
        self.resample()

    def resample_stats(self, n, sw, Sww):
        """the same update from the data's sufficient statistics -- count n, sum sw (D,), sum of outer products Sww (D, D) -- as the ranks
        of a sharded model exchange them (pgl_row_stats): the scatter about the mean is Sww - n xbar xbar' (one pass; the weights it is used
        for are centred near 0, so nothing cancels)"""
        mu_n, sigma_n, kappa_n, nu_n = self.mu_0, self.sigma_0, self.kappa_0, self.nu_0
        n = float(n)
        if n > 0:
            xbar = np.asarray(sw, dtype=float) / n
            scatter = np.asarray(Sww, dtype=float) - n * np.outer(xbar, xbar)
            scatter = 0.5 * (scatter + scatter.T)
            dev = xbar - self.mu_0
            mu_n = (self.kappa_0 * self.mu_0 + n * xbar) / (self.kappa_0 + n)
            sigma_n = self.sigma_0 + scatter + self.kappa_0 * n / (self.kappa_0 + n) * np.outer(dev, dev)
            kappa_n, nu_n = self.kappa_0 + n, self.nu_0 + n
        rng = np.random if self.rng is None else self.rng
        self.sigma = _sample_invwishart(sigma_n, nu_n, rng)
        self.mu = _mvn(rng, mu_n, self.sigma / kappa_n)

    def resample(self, data=()):
        D = len(self.mu_0)
        data = np.asarray(data, dtype=float).reshape(-1, D)
        n = data.shape[0]
        mu_n, sigma_n, kappa_n, nu_n = self.mu_0, self.sigma_0, self.kappa_0, self.nu_0
        if n > 0:
            # same statistics as data.mean(0) and data - xbar, without NumPy's slow short-inner-loop paths on an (n, B) array (n ~ N^2):
            # the mean as a matrix-vector product, the centring on rows of 64 observations at a time
            xbar = np.ones(n).dot(data) / n
            centred = np.empty_like(data)
            n64 = n - n % 64
            if n64:
                np.subtract(data[:n64].reshape(n64 // 64, 64 * D), np.tile(xbar, 64), out=centred[:n64].reshape(n64 // 64, 64 * D))
            centred[n64:] = data[n64:] - xbar
            dev = xbar - self.mu_0
            mu_n = (self.kappa_0 * self.mu_0 + n * xbar) / (self.kappa_0 + n)
            sigma_n = self.sigma_0 + centred.T.dot(centred) + self.kappa_0 * n / (self.kappa_0 + n) * np.outer(dev, dev)
            kappa_n, nu_n = self.kappa_0 + n, self.nu_0 + n
        rng = np.random if self.rng is None else self.rng
        self.sigma = _sample_invwishart(sigma_n, nu_n, rng)
        self.mu = _mvn(rng, mu_n, self.sigma / kappa_n)


class _NetworkModel(object):
    """(networks.py:13-73) a prior over A in {0,1}^{NxN} and W in R^{NxNxB}; rows = postsynaptic (incoming)."""

    def __init__(self, N, B, **kwargs):
        self.N, self.B = N, B

    def resample(self, data=[]):
        assert isinstance(data, tuple)
        A, W = data
        assert A.shape == (self.N, self.N) and A.dtype == bool and W.shape == (self.N, self.N, self.B)

    def log_likelihood(self, x):
        return 0

    def rvs(self, size=[]):
        return None


class _IndependentGaussianMixin(_NetworkModel):
    """every weight ~ N(mu, Sigma) with a shared NIW prior; self-connections get their own (networks.py:76-149)"""

    def __init__(self, N, B, mu_0=0.0, sigma_0=1.0, kappa_0=1.0, nu_0=3.0, is_diagonal_weight_special=True, **kwargs):
        _NetworkModel.__init__(self, N, B)
        mu_0 = expand_scalar(mu_0, (B,))
        sigma_0 = expand_cov(sigma_0, (B, B))
        self._gaussian = _NIW(mu_0, sigma_0, kappa_0, max(nu_0, B + 2.))
        self.is_diagonal_weight_special = is_diagonal_weight_special
        if is_diagonal_weight_special:
            nu_self = max(nu_0, B + 2.)
            if REFERENCE_QUIRKS:
                # networks.py:94 passes nu_0 raw.  An inverse-Wishart with nu < B has no density, so for nu_0 < B the floor of :89 is applied here
                # too.  What the reference does in that case is UNVERIFIED: it hands nu_0 to pybasicbayes' Gaussian, whose source is not under
                # /root/reference (it may raise at construction, at the first draw, or go on with an improper prior)
                if nu_0 >= B:
                    nu_self = nu_0
                else:
                    warnings.warn("self-connection prior: nu_0 = %g < B = %d is no proper inverse-Wishart; nu_0 is floored at B + 2 as at networks.py:89 "
                                  "(the reference passes it raw to pybasicbayes at networks.py:94: behaviour unverified, package absent)" % (nu_0, B),
                                  stacklevel=3)
            self._self_gaussian = _NIW(mu_0, sigma_0, kappa_0, nu_self)

    def _rows(self, off, diag, n0, n1):
        out = np.empty((n1 - n0, self.N) + off.shape)
        out[:] = off
        if diag is not None:
            r = np.arange(n0, n1)
            out[r - n0, r] = diag
        return out

    def _set_rng(self, rng):
        """generator the NIW draws take their numbers from (None: NumPy's global one, looked up at use).  A population model hands in one
        keyed by (seed, sweep) for the duration of a sweep's network update, so that every rank draws the same parameters"""
        self._gaussian.rng = rng
        if self.is_diagonal_weight_special:
            self._self_gaussian.rng = rng

    def weight_blocks(self):
        """(mu, Sigma) of an ordinary connection and of a self-connection (None, None if not special): all there is to mu_W / sigma_W"""
        if self.is_diagonal_weight_special:
            return self._gaussian.mu, self._gaussian.sigma, self._self_gaussian.mu, self._self_gaussian.sigma
        return self._gaussian.mu, self._gaussian.sigma, None, None

    def mu_W_rows(self, n0, n1):
        return self._rows(self._gaussian.mu, self._self_gaussian.mu if self.is_diagonal_weight_special else None, n0, n1)

    def sigma_W_rows(self, n0, n1):
        return self._rows(self._gaussian.sigma, self._self_gaussian.sigma if self.is_diagonal_weight_special else None, n0, n1)

    @property
    def mu_W(self):
        return self.mu_W_rows(0, self.N)

    @property
    def sigma_W(self):
        return self.sigma_W_rows(0, self.N)

    def resample(self, data=[], stats=None):
        """stats: optional ((n, sum w, sum w w') of the active off-diagonal weight vectors, the same of the active self-connections), as a
        population model has them from its ranks' rows (models.py: resample_model); the (A, W) walk below is then skipped -- it is O(N^2 B)
        on every rank of a sharded run.  Same random numbers consumed either way."""
        super(_IndependentGaussianMixin, self).resample(data)
        A, W = data
        if stats is not None:
            (n_o, s_o, S_o), (n_d, s_d, S_d) = stats
            if self.is_diagonal_weight_special:
                self._gaussian.resample_stats(n_o, s_o, S_o)
                self._self_gaussian.resample_stats(n_d, s_d, S_d)
            else:
                self._gaussian.resample_stats(n_o + n_d, s_o + s_d, S_o + S_d)
            return
        if self.is_diagonal_weight_special:
            eye = np.eye(self.N, dtype=bool)
            self._gaussian.resample(_take(W, A & ~eye))
            self._self_gaussian.resample(_take(W, A & eye))
        else:
            self._gaussian.resample(_take(W, A))


class _FixedWeightsMixin(_NetworkModel):
    """(networks.py:151-173)"""

    def __init__(self, N, B, mu=0.0, sigma=1.0, mu_self=None, sigma_self=None, **kwargs):
        _NetworkModel.__init__(self, N, B)
        self._mu = expand_scalar(mu, (N, N, B))
        self._sigma = expand_cov(mu if REFERENCE_QUIRKS else sigma, (N, N, B, B))       # networks.py:159 builds Sigma from `mu`
        if (mu_self is not None) and (sigma_self is not None):
            r = np.arange(N)
            self._mu[r, r, :] = expand_scalar(mu_self, (N, B))
            self._sigma[r, r, :] = expand_cov(sigma_self, (N, B, B))

    mu_W = property(lambda self: self._mu)
    sigma_W = property(lambda self: self._sigma)

    def mu_W_rows(self, n0, n1):
        return self._mu[n0:n1]

    def sigma_W_rows(self, n0, n1):
        return self._sigma[n0:n1]


class _FixedAdjacencyMixin(_NetworkModel):
    """(networks.py:178-190)"""

    def __init__(self, N, B, rho=0.5, rho_self=None, **kwargs):
        _NetworkModel.__init__(self, N, B)
        self._rho = expand_scalar(rho, (N, N))
        if rho_self is not None:
            self._rho[np.diag_indices(N)] = rho_self

    rho = property(lambda self: self._rho)


class _DenseAdjacencyMixin(_NetworkModel):
    """(networks.py:194-204)"""

    def __init__(self, N, B, **kwargs):
        _NetworkModel.__init__(self, N, B)
        self._rho = np.ones((N, N))

    rho = property(lambda self: self._rho)


class _StochasticBlockAdjacencyMixin(_NetworkModel):
    """a learned prior on A (the reference's `# TODO: Define the stochastic block models`): K blocks, z_n ~ Cat(pi), A[n][m] ~ Bernoulli(P[z_n][z_m])
    off the diagonal and Bernoulli(rho_self) on it; pyglm_amd/sbm.py states the law and the update.  State: z (N,), P (K, K), pi (K,), rho_self.
    The initial state is drawn from the prior with NumPy's global generator unless z is given."""

    def __init__(self, N, B, K=8, a_0=1.0, b_0=1.0, alpha=1.0, a_self=1.0, b_self=1.0, rho_self=None, z=None, **kwargs):
        from . import sbm
        _NetworkModel.__init__(self, N, B)
        self.K = sbm.check_blocks(K)
        self.a_0, self.b_0, self.alpha, self.a_self, self.b_self = float(a_0), float(b_0), float(alpha), float(a_self), float(b_self)
        assert min(self.a_0, self.b_0, self.alpha, self.a_self, self.b_self) > 0
        self._rho_self_fixed = None if rho_self is None else float(rho_self)
        self.z = np.random.randint(self.K, size=N).astype(np.int64) if z is None else sbm._labels(z, self.K, N).copy()
        self.P, self.pi = sbm.clamp(np.random.beta(self.a_0, self.b_0, size=(self.K, self.K)), np.random.dirichlet(np.full(self.K, self.alpha / self.K)))
        self.rho_self = float(np.random.beta(self.a_self, self.b_self)) if rho_self is None else float(rho_self)
        self._rng = self._scan_ctx = self._driver = None

    def __deepcopy__(self, memo):
        """the chain state without the device buffers (a driver is rebuilt when it is next needed)"""
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__dict__.update({k: (None if k == "_driver" else copy.deepcopy(v, memo)) for k, v in self.__dict__.items()})
        return new

    def _set_rng(self, rng):
        """generator of the conjugate draws (None: NumPy's global one); handed on to the weights' mixin, which draws first"""
        self._rng = rng
        up = getattr(super(_StochasticBlockAdjacencyMixin, self), "_set_rng", None)
        if up is not None:
            up(rng)

    def _set_scan(self, seed, sweep=0, device=None):
        """a population model's hook beside _set_rng: the scan of the next resample() takes its uniforms from the Philox stream (seed, sweep)
        and runs on `device` (None: on the host).  _set_scan(None): back to NumPy's global generator and the host"""
        self._scan_ctx = None if seed is None else (int(seed), int(sweep), device)

    rho_diag = property(lambda self: self.rho_self, doc="what the diagonal of rho holds")
    block_sizes = property(lambda self: np.bincount(self.z, minlength=self.K))

    @property
    def rho(self):
        """(N, N) as pushed: P[z_n][z_m], rho_diag on the diagonal"""
        from .sbm import rho_of
        return rho_of(self.P, self.z, self.rho_diag)

    def resample(self, data=[], **kw):
        super(_StochasticBlockAdjacencyMixin, self).resample(data, **kw)      # the weights' draws first, exactly as without this mixin
        self._resample_adjacency(data[0])

    def _resample_adjacency(self, A):
        from . import sbm
        rng = np.random if self._rng is None else self._rng
        kw = dict(a_0=self.a_0, b_0=self.b_0, alpha=self.alpha, a_self=self.a_self, b_self=self.b_self, rho_self=self._rho_self_fixed)
        if self._scan_ctx is None:
            kw["u"] = np.random.random_sample(self.N)
        else:
            seed, sweep, device = self._scan_ctx
            kw.update(seed=seed, sweep=sweep)
            if device is not None and self.K > 1:
                if self._driver is None or str(self._driver.dev) != str(sbm._device("the block-model update", device)[0]):
                    self._driver = sbm.DeviceSBM(self.N, self.K, device=device)
                kw["driver"] = self._driver
        out = sbm.sbm_host(A, self.z, self.K, rng, **kw)
        self.z, self.P, self.pi, self.rho_self = out["z"], out["P"], out["pi"], out["rho_self"]


class _IndependentBernoulliMixin(_StochasticBlockAdjacencyMixin):
    """the reference's unfinished class (networks.py: `TODO: Implement the BetaBernoulli class`), finished: one learned connection
    probability p ~ Beta(a_0, b_0) -- the block model with K = 1 -- and, where the diagonal is special, rho_self ~ Beta(a_0, b_0) of its
    own; with the flag off the N self-connections pool with the rest"""

    def __init__(self, N, B, a_0=1.0, b_0=1.0, is_diagonal_conn_special=True, **kwargs):
        _StochasticBlockAdjacencyMixin.__init__(self, N, B, K=1, a_0=a_0, b_0=b_0, a_self=a_0, b_self=b_0)
        self.is_diagonal_conn_special = bool(is_diagonal_conn_special)

    p = property(lambda self: float(self.P[0, 0]), doc="the learned connection probability")
    rho_diag = property(lambda self: self.rho_self if self.is_diagonal_conn_special else float(self.P[0, 0]))

    def _resample_adjacency(self, A):
        if self.is_diagonal_conn_special:
            return _StochasticBlockAdjacencyMixin._resample_adjacency(self, A)
        from . import sbm
        rng = np.random if self._rng is None else self._rng
        total, cells = int(np.count_nonzero(A)), self.N * self.N
        self.P = sbm.clamp(np.reshape(rng.beta(self.a_0 + total, self.b_0 + cells - total), (1, 1)), self.pi)[0]
        self.rho_self = float(self.P[0, 0])


def _split(kw):
    return {k: v for k, v in kw.items() if k not in ("rho", "rho_self")}, {k: v for k, v in kw.items() if k in ("rho", "rho_self")}


def _split_named(kw, names):
    return {k: v for k, v in kw.items() if k not in names}, {k: v for k, v in kw.items() if k in names}


class FixedMeanDenseNetwork(_DenseAdjacencyMixin, _FixedWeightsMixin):
    def __init__(self, N, B, **kw):
        if REFERENCE_QUIRKS:
            _dropped("FixedMeanDenseNetwork", kw)
            kw = {}
        _FixedWeightsMixin.__init__(self, N, B, **kw)
        _DenseAdjacencyMixin.__init__(self, N, B)


class FixedMeanSparseNetwork(_FixedAdjacencyMixin, _FixedWeightsMixin):
    def __init__(self, N, B, **kw):
        wkw, akw = _split(kw)
        if REFERENCE_QUIRKS:
            _dropped("FixedMeanSparseNetwork", wkw)
            wkw = {}
        _FixedWeightsMixin.__init__(self, N, B, **wkw)
        _FixedAdjacencyMixin.__init__(self, N, B, **akw)


class NIWDenseNetwork(_DenseAdjacencyMixin, _IndependentGaussianMixin):
    def __init__(self, N, B, **kw):
        if REFERENCE_QUIRKS:
            _dropped("NIWDenseNetwork", kw)
            kw = {}
        _IndependentGaussianMixin.__init__(self, N, B, **kw)
        _DenseAdjacencyMixin.__init__(self, N, B)


class NIWSparseNetwork(_FixedAdjacencyMixin, _IndependentGaussianMixin):
    """(networks.py:283-285; see REFERENCE_QUIRKS for which keyword arguments arrive)"""

    def __init__(self, N, B, **kw):
        wkw, akw = _split(kw)
        if REFERENCE_QUIRKS:
            _dropped("NIWSparseNetwork", wkw)
            wkw = {}
        _IndependentGaussianMixin.__init__(self, N, B, **wkw)
        _FixedAdjacencyMixin.__init__(self, N, B, **akw)


class BetaBernoulliSparseNetwork(_IndependentBernoulliMixin, _IndependentGaussianMixin):
    """NIW weights under a learned connection probability.  The weight keywords are treated as for NIWSparseNetwork (REFERENCE_QUIRKS); the
    adjacency keywords (a_0, b_0, is_diagonal_conn_special) always arrive"""
    _ADJACENCY_KW = ("a_0", "b_0", "is_diagonal_conn_special")

    def __init__(self, N, B, **kw):
        wkw, akw = _split_named(kw, self._ADJACENCY_KW)
        if REFERENCE_QUIRKS:
            _dropped(type(self).__name__, wkw)
            wkw = {}
        _IndependentGaussianMixin.__init__(self, N, B, **wkw)
        _IndependentBernoulliMixin.__init__(self, N, B, **akw)


class SBMSparseNetwork(_StochasticBlockAdjacencyMixin, _IndependentGaussianMixin):
    """NIW weights under a stochastic block model of the adjacency.  The weight keywords are treated as for NIWSparseNetwork
    (REFERENCE_QUIRKS); the adjacency keywords (K, a_0, b_0, alpha, a_self, b_self, rho_self, z) always arrive"""
    _ADJACENCY_KW = ("K", "a_0", "b_0", "alpha", "a_self", "b_self", "rho_self", "z")

    def __init__(self, N, B, **kw):
        wkw, akw = _split_named(kw, self._ADJACENCY_KW)
        if REFERENCE_QUIRKS:
            _dropped(type(self).__name__, wkw)
            wkw = {}
        _IndependentGaussianMixin.__init__(self, N, B, **wkw)
        _StochasticBlockAdjacencyMixin.__init__(self, N, B, **akw)
