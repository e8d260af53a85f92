"""Population models with the reference's interface (pyglm/models.py): SparseBernoulliGLM & friends.

`add_data() / resample_model() / log_likelihood()` are drop-ins; underneath, the N per-neuron regressions are not
looped over in Python (models.py:169-171) but sent through the HIP kernels in batches by a `GibbsEngine`, and they
shard by postsynaptic neuron over the ranks of a torch.distributed process group (one process per GPU):

    rank r owns neurons [r*N/G, (r+1)*N/G)   -- its Y columns, its rows of (A, W, b); X is replicated.
    per sweep:  ONE all_gather_into_tensor of the shard's packed rows (W | b | eta or status flags | row statistics | a as bytes), taken from
                the device buffers the sweep updated and launched behind it on the stream (the network prior needs the full (A, W),
                models.py:230 -- and of W only the rows' sufficient statistics, which travel with them);
                all_reduce of the N per-neuron fp64 log-likelihoods (own entries, zeros elsewhere) in log_likelihood().
Random inputs are keyed by (seed, sweep, global neuron), so results do not depend on the number of ranks.
"""
import numpy as np
import numpy.random as npr

from . import networks as _networks
from . import regression as _regression


def _dist():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist
    except ImportError:
        pass
    return None


def state_row_layout(N, B, K=0):
    """byte layout of one neuron's row of the packed state the ranks exchange: W (N*B doubles) | b (1 double) | eta (1 double: noise variance,
    Gaussian model; 0 otherwise) | row statistics (1 + B + B^2 doubles: count, sum and sum of outer products of the row's active off-diagonal
    weight vectors -- the network prior's sufficient statistics, networks.py:132-149) | a (N bytes, padded to a multiple of 8) | with K > 0
    covariates, beta (K doubles: the last 8 K bytes of the row; K = 0 leaves the layout as it always was)
    ->  (offset of b, of eta, of the statistics, of a, bytes per row)"""
    D = N * B
    os_ = 8 * D + 16
    oa = os_ + 8 * (1 + B + B * B)
    return 8 * D, 8 * D + 8, os_, oa, oa + -(-N // 8) * 8 + 8 * K


def host_row_stats(a, W, n0):
    """the statistics pgl_row_stats forms on the device, on the host: [count, sum w, sum w w'] over the active presynaptic m != n0 + n of every row
    n of a (n, N) / W (n, N, B) -- for state that never was on a GPU (a network resampled from user-supplied (A, W), the CPU test engine)"""
    a = np.array(a, dtype=bool)
    n, N = a.shape
    B = W.shape[-1]
    r = np.arange(n)
    ok = n0 + r < N
    a[r[ok], n0 + r[ok]] = False
    out = np.empty((n, 1 + B + B * B))
    for i in range(n):                       # row by row: a row's numbers must not depend on how many rows are handed in together
        Wm = np.asarray(W[i], dtype=np.float64)[a[i]]
        out[i, 0] = Wm.shape[0]
        out[i, 1:1 + B] = Wm.sum(axis=0)
        out[i, 1 + B:] = Wm.T.dot(Wm).reshape(-1)
    return out


def shard_bounds(N, world, rank):
    """contiguous, balanced neuron ranges"""
    base, rem = divmod(N, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class NonlinearAutoregressiveModel(object):
    """(models.py:8-201) y_n[t] ~ p(f(w_n . x[t])), x = basis-filtered history of all neurons."""
    DRAW_AHEAD_MIN_SIZE = 0            # N*N*B from which the next sweep's host draws are made while the GPU is busy (every size: a small model's sweep leaves the host idle for most of a millisecond)

    def __init__(self, N, regressions, basis=None, B=10, device=None, engine_factory=None, seed=None, engine_kwargs=None, shard=None,
                 n_covariates=0, covariate_prior=None, n_latents=0, latent_loading_prior=None, latent_ar=None):
        """n_covariates = K > 0: every data set carries external covariates S (T, K) shared by all neurons (add_data(..., covariates=S)),
        neuron n the weights beta_n (model.covariate_weights, (N, K)) with the prior beta_n ~ N(mu0, Sigma0), covariate_prior = (mu0,
        Sigma0), default (0, I); psi = X . vec(a * W) + b + S beta_n, and resample_model() draws beta right behind the regressions'
        sweep (pyglm_amd/covariates.py states the law).
        n_latents = Q > 0 (1 .. 8, n_covariates + Q <= 32): Q latent factors shared by the population, x_t ~ N(0, I) per time bin, inferred
        with the network -- the common input nobody recorded (pyglm_amd/latents.py states the law).  Neuron n's loadings C_n
        (model.latent_loadings, (N, Q)) have the prior latent_loading_prior = (mu, Sigma), default (0, I), and are drawn by the covariate
        step; resample_model() draws x | omega, W, b, beta between the sweep and that step.  model.latents, model.common_input().
        latent_ar = phi (a scalar or Q values, 0 <= phi_q < 1; None: zeros): a temporal prior on the factors, per factor and data set
        x_0 ~ N(0, 1), x_t = phi_q x_{t-1} + sqrt(1 - phi_q^2) eps_t -- stationary with variance 1, for common input that changes slowly.
        A hyper-parameter (model.latent_ar), not chain state; all zeros is the model without it, bit for bit."""
        from . import covariates as _cov
        from . import latents as _lat
        self.N = N
        self.K_obs = _cov.check_count(n_covariates)      # observed covariates; K: all columns of S, the latent ones behind the observed
        self.Q = _lat.check_count(n_latents, self.K_obs)
        self.K = self.K_obs + self.Q
        self.latent_ar = _lat.check_ar(latent_ar, self.Q)
        if self.K_obs:
            _cov.prior_terms(self.K_obs, covariate_prior)     # (a mis-shaped prior is refused here, not at the first data set)
        elif covariate_prior is not None:
            raise ValueError("covariate_prior was given, but n_covariates=0")
        if not self.Q and latent_loading_prior is not None:
            raise ValueError("latent_loading_prior was given, but n_latents=0")
        # the engine's prior of all K weights: the user's own without latents, the two priors joined block-diagonally with them
        self._covariate_prior = _lat.joint_prior(self.K_obs, self.Q, covariate_prior, latent_loading_prior) if self.Q else covariate_prior
        self._beta = np.zeros((N, self.K))
        self.covariates_list = []                        # S of every data set, parallel to data_list (None without covariates)
        assert len(regressions) == N
        self.regressions = regressions
        if basis is None:
            basis = np.eye(B)
        else:
            assert basis.ndim == 2
        self.basis = basis
        self.B = self.basis.shape[1]
        self.data_list = []
        # ---- device / distribution
        dist = _dist()
        self.world = dist.get_world_size() if dist else 1
        self.rank = dist.get_rank() if dist else 0
        self.n0, self.n1 = shard_bounds(N, self.world, self.rank)
        # shard=(n0, n1): this process sweeps neurons [n0, n1) only, whatever the process group says, and exchanges nothing -- the other
        # rows of (A, W, b) keep their values.  What ONE rank of a job too large for the GPUs at hand does (bench.py --neurons).
        self._shard_override = shard is not None
        if self.Q and (self.world > 1 or shard is not None):
            raise ValueError("n_latents=%d with %s: a time bin's sums run over ALL neurons, so sharded ranks would need an ordered all-reduce of "
                             "T x %d numbers per sweep; latents across ranks are not supported"
                             % (self.Q, "shard=%r" % (shard,) if shard is not None else "%d ranks" % self.world, self.Q * (self.Q + 3) // 2))
        if shard is not None:
            self.n0, self.n1 = int(shard[0]), int(shard[1])
            assert 0 <= self.n0 < self.n1 <= N
        self._device = device
        self._engine_factory = engine_factory
        self._engine_kwargs = engine_kwargs or {}
        self._engine = None
        # like the reference's PG samplers (regression.py:476) the stream seed comes from NumPy's global RNG
        self.seed = int(npr.randint(2 ** 31)) if seed is None else int(seed)
        if dist and seed is None:
            import torch
            t = torch.tensor([self.seed], dtype=torch.int64)
            if dist.get_backend() == "nccl":
                t = t.to(self._comm_dev())
            dist.broadcast(t, 0)
            self.seed = int(t.item())
        self._adopt_state()
        self.sweeps_done = 0
        self._fresh_stats = self._stats_kept = None      # per-row statistics for the network prior (resample_regressions -> resample_network)
        self.comm_seconds = 0.0        # wall time this rank has spent inside collectives (all_gather of rows, scalar all_reduce)
        self.collectives = 0           # collectives issued by this rank (one per sweep + one per log_likelihood())

    def _comm_dev(self):
        """device the RCCL collectives of this rank stage through: the shard's GPU"""
        import torch
        if self._engine is not None and hasattr(self._engine, "dev"):
            return self._engine.dev
        return torch.device(self._device) if self._device else torch.device("cuda", torch.cuda.current_device())

    # ---- engine
    @property
    def engine(self):
        if self._engine is None:
            # the observation model of ALL the regressions (regression.device_obs), kept: a regression of another kind swapped in later
            # is an error at the next sweep (_check_obs), not a silent run of the old model
            self._engine_mode = _regression.device_obs(self.regressions)
            obs, xi = self._engine_mode
            kw = dict(obs=obs, xi=xi)
            if self.K:
                kw.update(n_covariates=self.K_obs, covariate_prior=self._covariate_prior)
            if self.Q:
                kw.update(n_latents=self.Q)
            ar = bool(np.any(self.latent_ar > 0.0))
            if ar:                                   # (only then: a factory from before the temporal prior keeps working)
                kw.update(latent_ar=self.latent_ar.copy())
            kw.update(self._engine_kwargs)
            if self._engine_factory is not None:
                eng = self._engine_factory(self.N, self.B, self.n0, self.n1, **kw)
                if ar and not np.array_equal(np.asarray(getattr(eng, "latent_ar", ()), dtype=np.float64), self.latent_ar):
                    raise ValueError("a model with latent_ar needs an engine that takes it: %s does not accept the keyword latent_ar "
                                     "(its attribute latent_ar does not hold the coefficients it was given)" % type(eng).__name__)
                if self.Q and not hasattr(eng, "latent_step"):
                    raise ValueError("a model with latents needs an engine that samples them: %s has no latent_step(a, W, b, seed, sweep)"
                                     % type(eng).__name__)
                self._engine = eng
            else:
                from .engine import GibbsEngine
                import torch
                dev = self._device or ("cuda:%d" % torch.cuda.current_device())
                self._engine = GibbsEngine(self.N, self.B, self.n0, self.n1, device=dev, **kw)
            # the Gibbs steps, held (scratch and all) as long as the engine: device classes, or (engine_factory) xi's host twin and the engine's own
            from . import covariates as _cov, dispersion as _disp, latents as _lat
            from .summary import device_engine
            eng, dev = self._engine, device_engine(self._engine)
            self._xi_step = _disp._DeviceStep(eng) if dev else _disp._HostStep(eng, self)
            self._cov_step, self._lat_step = (_cov._DeviceStep(eng), _lat._DeviceStep(eng)) if dev else (eng, eng)
        return self._engine

    # ---- chain state: three arrays of the model, of which every regression's (a, W, b) are row views (regression._adopt)
    def _adopt_state(self):
        """(re)build the model's state arrays from its regressions and make their a / W / b views of them.  Cheap when nothing changed hands:
        N identity checks.  A regression that was swapped in from outside (`model.regressions[n] = other`) is adopted here."""
        N = self.N
        st = getattr(self, "_st", None)
        regs = self.regressions
        if st is not None and all(r._store is not None and r._store[0] is st[0] and r._store[3] == n for n, r in enumerate(regs)):
            return st
        st = (np.zeros((N, N), dtype=bool), np.zeros((N, N, self.B)), np.zeros((N, 1)))
        for n, r in enumerate(regs):
            r._adopt(st[0], st[1], st[2], n)
        self._st = st
        return st

    # ---- state read-backs (models.py:54-64): row = postsynaptic.  Copies, like the reference's np.array([...])
    @property
    def weights(self):
        return self._adopt_state()[1].copy()

    @property
    def adjacency(self):
        return self._adopt_state()[0].copy()

    @property
    def biases(self):
        return self._adopt_state()[2].ravel().copy()

    # ---- external covariates (pyglm_amd/covariates.py)
    @property
    def covariate_weights(self):
        """(N, K) the weights beta of the observed covariates, row = neuron; a copy.  Assignable: model.covariate_weights = beta"""
        return self._beta[:, :self.K_obs].copy()

    @covariate_weights.setter
    def covariate_weights(self, beta):
        new = self._beta.copy()                      # (_beta: all K columns, the latents' loadings behind the observed covariates' weights)
        new[:, :self.K_obs] = np.broadcast_to(np.asarray(beta, dtype=np.float64), (self.N, self.K_obs))
        self._beta = new

    # ---- latent common input (pyglm_amd/latents.py)
    def _need_latents(self, what):
        if not self.Q:
            raise ValueError("%s: this model was built with n_latents=0" % what)

    @property
    def latents(self):
        """[X_i (T_i, Q)]: the latent factors of every data set at the current state; copies.  X and the loadings are defined only up to
        rotation and sign: common_input() is the identifiable quantity"""
        self._need_latents("latents")
        return [self.engine.latents(i) for i in range(len(self.data_list))]

    def set_latents(self, i, X):
        """X (T_i, Q) becomes the latent factors of data set i"""
        self._need_latents("set_latents()")
        self._sync_covariates()
        self.engine.set_latents(range(len(self.data_list))[i], X)

    @property
    def latent_loadings(self):
        """(N, Q) the loadings C, row = neuron; a copy"""
        self._need_latents("latent_loadings")
        return self._beta[:, self.K_obs:].copy()

    def common_input(self, data=0):
        """(T, N) = X C': the drive the latent factors give every neuron of data set `data` at the current state -- what they add to psi"""
        from . import latents as _lat
        self._need_latents("common_input()")
        return _lat.common_input_host(self.engine.latents(range(len(self.data_list))[data]), self._beta[:, self.K_obs:])

    def _refuse_heldout_latents(self, what, datas):
        if self.Q and datas is not None:
            raise ValueError("%s: held-out datas= in a model with latents (n_latents=%d) is not supported -- the latent factors of a recording "
                             "the chain never saw are unknown" % (what, self.Q))

    def _sync_covariates(self, eng=None):
        """this shard's beta onto engine eng (default: the model's own) where it holds another: after set_state(), an assignment to
        covariate_weights, and for a held-out engine, which was built at an earlier beta.  N K numbers compared; nothing without covariates"""
        if not self.K:
            return
        eng = self.engine if eng is None else eng
        loc = self._beta[self.n0:self.n1]
        if not hasattr(eng, "set_covariate_weights"):
            raise ValueError("a model with covariates needs an engine that takes them: %s has no set_covariate_weights(beta)" % type(eng).__name__)
        if not np.array_equal(eng.beta, loc):
            eng.set_covariate_weights(loc)

    def _refuse_covariates(self, what, covariates=None, latents=None, keywords=False):
        """the first check of generate(), simulate() and predictive_check(): a model with observed covariates needs covariates=, one with
        latents needs latents= (keywords: the caller takes the two, and the message says so); generate() takes neither"""
        if (self.K_obs and covariates is None) or (self.Q and latents is None):
            hint = ""
            if keywords:
                hint = "; or pass " + " and ".join(
                    ["covariates=S (T, %d), one row per simulated bin" % self.K_obs] * bool(self.K_obs and covariates is None) +
                    ["latents='prior', 'fitted' or an array (T, %d)" % self.Q] * bool(self.Q and latents is None))
            raise ValueError("%s: free-running simulation of a model with covariates (n_covariates=%d%s) is not supported -- it needs covariates "
                             "for bins that were never recorded; conditional_simulate() / conditional_check() work%s"
                             % (what, self.K_obs, ", n_latents=%d" % self.Q if self.Q else "", hint))
        if covariates is not None and not self.K_obs:
            raise ValueError("%s: covariates= was given, but the model was built with n_covariates=0: there is no weight to apply them with" % what)
        if latents is not None and not self.Q:
            raise ValueError("%s: latents= was given, but the model was built with n_latents=0: there is no loading to apply them with" % what)

    def _drive(self, what, T, R, covariates, latents, data):
        """the checked covariates= / latents= / data= of simulate() -> simulate.Drive, or None for a model with neither term"""
        from . import covariates as _cov
        from . import latents as _lat
        from . import simulate as _sim
        if not self.K:
            return None
        T = int(T)
        S = X = None
        if self.K_obs:
            if isinstance(covariates, str):
                if covariates != "data":
                    raise ValueError("%s: covariates=%r; an array (T, %d) or 'data' is required" % (what, covariates, self.K_obs))
                S = self.covariates_list[range(len(self.data_list))[data]]
                if T > S.shape[0]:
                    raise ValueError("%s: covariates='data' covers the %d bins of data set %d; T = %d is more" % (what, S.shape[0], data, T))
                S = S[:T]
            S = _cov.check_covariates(covariates if S is None else S, T, self.K_obs, what)
        if self.Q:
            if isinstance(latents, str):
                if latents not in ("prior", "fitted"):
                    raise ValueError("%s: latents=%r; 'prior', 'fitted' or an array (T, %d) or (replicates, T, %d) is required"
                                     % (what, latents, self.Q, self.Q))
                X = latents
                if latents == "fitted":
                    X = self.engine.latents(range(len(self.data_list))[data])
                    if T > X.shape[0]:
                        raise ValueError("%s: latents='fitted' covers the %d bins of data set %d; T = %d is more" % (what, X.shape[0], data, T))
                    X = X[:T][None]
            else:
                X = np.asarray(latents, dtype=np.float64)
                if X.ndim == 2:
                    X = X[None]
                if X.ndim != 3 or X.shape[0] not in (1, int(R)):
                    raise ValueError("%s: latents of shape %s; (%d, %d) or (replicates = %d, %d, %d) is required"
                                     % (what, np.shape(latents), T, self.Q, R, T, self.Q))
                X = np.stack([_lat.check_latents(x, T, self.Q, what) for x in X])
        return _sim.Drive(self._beta, S_obs=S, latents=X, phi=self.latent_ar)

    def add_data(self, data, X=None, covariates=None):
        """(models.py:66-80)  covariates: S (T, K) of this data set, required with n_covariates = K > 0 and refused without"""
        from . import covariates as _cov
        N, B = self.N, self.B
        assert isinstance(data, np.ndarray) and data.ndim == 2 and data.shape[1] == self.N
        T = data.shape[0]
        if X is not None:
            assert X.shape == (T, N, B)
        S = _cov.check_covariates(covariates, T, self.K_obs, "add_data")
        _regression.check_counts(self.regressions, data)
        self._sync_covariates()
        ckw = dict(covariates=S) if self.K_obs else {}
        ds = self.engine.add_data(data, X=X, basis=self.basis, **ckw, **self._obs_terms_kw(data))
        self.covariates_list.append(S)
        dist = _dist()
        if dist is not None and hasattr(self.engine, "drop_int8"):
            # gram="auto" looks at the free memory of ITS GPU: make the choice collective (integer path only if every rank can take it), so
            # that results never depend on which rank a neuron lives on
            import torch
            t = torch.tensor([int(bool(getattr(ds, "int8", False)))], dtype=torch.int32)
            if dist.get_backend() == "nccl":
                t = t.to(self._comm_dev())
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            if not int(t.item()):
                self.engine.drop_int8(len(self.engine.datasets) - 1)
        self.data_list.append((_LazyX(self.engine, len(self.engine.datasets) - 1) if X is None else X, data))

    def _obs_terms_kw(self, Y):
        """engine.add_data's obs_terms for data Y (T, N) in hooks mode -- a(y), b(y), log c(y) of this rank's neurons -- else nothing"""
        if self.engine_obs() != "hooks":
            return {}
        return dict(obs_terms=_regression.obs_terms(self.regressions[self.n0:self.n1], np.asarray(Y)[:, self.n0:self.n1]))

    def _check_obs(self):
        """the engine was built for one observation model: a regression swapped in since (model.regressions[n] = other) must not change it"""
        if self._engine is None:
            return
        mode = _regression.device_obs(self.regressions)
        if mode[0] == self._engine_mode[0] == "negbin" and np.ndim(self._engine_mode[1]) and _regression.learns_xi(self.regressions):
            self._engine_mode = mode          # a learned xi moves (and a user may set r.xi): the model kind is what stays guarded
            return
        if not _regression.same_obs(mode, self._engine_mode):
            raise ValueError("the regressions now call for the device observation model %r (param %r), but this model's engine was built for %r "
                             "(param %r): build a new model for the new regressions" % (mode[0], mode[1], self._engine_mode[0], self._engine_mode[1]))

    # ---- the negative-binomial dispersion, where regressions learn it (pyglm_amd/dispersion.py)
    def _learns_xi(self):
        """does any regression of the WHOLE model learn its xi?  (every rank answers alike: they take the same exchange path)"""
        return self.engine_obs() == "negbin" and _regression.learns_xi(self.regressions)

    def _push_xi(self, eng=None):
        """the shard's current xi into the engine's per-neuron device array: the learned values, and whatever set_state() or a user's
        `r.xi = ...` put there since the last sweep"""
        eng = self.engine if eng is None else eng
        if not hasattr(eng, "set_obs_param"):
            raise ValueError("a regression with xi_prior needs an engine that takes a new xi: %s has no set_obs_param(xi)" % type(eng).__name__)
        eng.set_obs_param([r.xi for r in self.regressions[self.n0:self.n1]])

    def _resample_xi(self, a, W, b):
        """xi of the shard's regressions after the CRT step under the weights (a, W, b) the sweep just drew -> (nloc,): the table counts and
        sum_t log(1 + e^psi) from self._xi_step; the gamma variates from the host, keyed by the global neuron.  Without xi_prior xi stays."""
        from . import dispersion as _disp
        regs = self.regressions[self.n0:self.n1]
        L, S = self._xi_step.stats(a, W, b, self.seed, self.sweeps_done)
        xi = np.array([r.xi for r in regs], dtype=np.float64)
        for i, r in enumerate(regs):
            if getattr(r, "xi_prior", None) is not None:
                xi[i] = _disp.draw_xi(r, int(L[i]), float(S[i]), self.seed, self.sweeps_done, self.n0 + i)
        return xi

    def _store_xi(self, lo, xi):
        """xi (k,) of neurons lo .. lo + k - 1 onto the regressions that learn it; the engine and the cached device mode follow"""
        for n, r in enumerate(self.regressions[lo:lo + len(xi)]):
            if getattr(r, "xi_prior", None) is not None:
                r.xi = float(xi[n])
        self._push_xi()
        self._engine_mode = _regression.device_obs(self.regressions)

    # ---- local <-> global state
    def _local_state(self):
        # views, not copies: engine.sweep uploads them before it returns, and the model's arrays are only written after it has
        A, W, b = self._adopt_state()
        return A[self.n0:self.n1], W[self.n0:self.n1], b[self.n0:self.n1, 0]

    def _store_rows(self, lo, hi, a, W, b):
        """rows [lo, hi) of the chain state <- (a, W, b): three array assignments (the regressions' a / W / b are views of these arrays).
        a may be boolean or 0/1 integers / bytes, W (rows, N, B) or (rows, N*B), contiguous or strided: one pass over each"""
        A_, W_, b_ = self._adopt_state()
        A_[lo:hi] = a
        W_[lo:hi].reshape(hi - lo, -1)[...] = np.asarray(W).reshape(hi - lo, -1) if getattr(W, "ndim", 2) == 3 else W
        b_[lo:hi, 0] = np.asarray(b).reshape(-1)

    def _gather_rows(self, arr):
        """all_gather of per-neuron rows over the shard axis (ranks may own different counts)"""
        dist = _dist()
        if dist is None or self._shard_override:
            return arr
        import time
        import torch
        t0 = time.perf_counter()
        nccl = dist.get_backend() == "nccl"
        counts = [shard_bounds(self.N, self.world, r) for r in range(self.world)]
        maxc = max(hi - lo for lo, hi in counts)
        was_bool = arr.dtype == np.bool_
        if was_bool:
            arr = arr.astype(np.uint8)           # (bytes travel; not every collective backend takes bool tensors)
        pad = np.zeros((maxc,) + arr.shape[1:], dtype=arr.dtype)
        pad[:arr.shape[0]] = arr
        t = torch.from_numpy(np.ascontiguousarray(pad))
        if nccl:
            t = t.to(self._comm_dev())
        outs = [torch.empty_like(t) for _ in range(self.world)]
        dist.all_gather(outs, t)
        out = np.concatenate([o.cpu().numpy()[: hi - lo] for o, (lo, hi) in zip(outs, counts)], axis=0)
        if was_bool:
            out = out.astype(bool)
        self.comm_seconds += time.perf_counter() - t0
        self.collectives += 1
        return out

    # ---- the per-sweep exchange: one packed all_gather
    def _pack_rows_host(self, a, W, b, eta=None, stats=None, beta=None):
        """host (a, W, b[, eta]) of the local rows and their statistics -> packed uint8 rows (state_row_layout); beta (rows, K) rides behind
        each row in a model with covariates"""
        ob, oe, os_, oa, rb = state_row_layout(self.N, self.B, self.K)
        nl = a.shape[0]
        buf = np.zeros((nl, rb), dtype=np.uint8)
        buf[:, :ob] = np.ascontiguousarray(W, dtype=np.float64).reshape(nl, -1).view(np.uint8)
        buf[:, ob:oe] = np.ascontiguousarray(b, dtype=np.float64).reshape(nl, 1).view(np.uint8)
        if eta is not None:
            buf[:, oe:os_] = np.ascontiguousarray(eta, dtype=np.float64).reshape(nl, 1).view(np.uint8)
        if stats is not None:
            buf[:, os_:oa] = np.ascontiguousarray(stats, dtype=np.float64).reshape(nl, -1).view(np.uint8)
        buf[:, oa:oa + self.N] = np.asarray(a).astype(np.uint8)
        if self.K:
            buf[:, rb - 8 * self.K:] = np.ascontiguousarray(beta, dtype=np.float64).reshape(nl, self.K).view(np.uint8)
        return buf

    def _unpack_rows(self, buf):
        """-> (a, W, b, eta, row statistics, beta) of the rows in buf (n, row bytes): a (n, N) as bytes and W (n, N*B) are strided VIEWS of buf
        -- the caller stores them into the model's arrays in one pass (_store_rows) --, b, eta and the statistics small copies; beta (n, K) a
        copy in a model with covariates, None in one without"""
        ob, oe, os_, oa, rb = state_row_layout(self.N, self.B, self.K)
        n = buf.shape[0]
        W = buf[:, :ob].view(np.float64)
        b = buf[:, ob:oe].view(np.float64).reshape(n).copy()
        eta = buf[:, oe:os_].view(np.float64).reshape(n).copy()
        stats = buf[:, os_:oa].view(np.float64).copy()
        a = buf[:, oa:oa + self.N]
        beta = None
        if self.K:
            beta = np.ascontiguousarray(buf[:, rb - 8 * self.K:rb]).view(np.float64).reshape(n, self.K).copy()
        return a, W, b, eta, stats, beta

    def _gather_start(self, packed):
        """packed: torch uint8 (local rows, row bytes), on the shard's GPU or on the host.  Starts ONE all_gather_into_tensor of it (ranks
        may own different counts: rows are padded to the largest shard) and returns a handle for _gather_finish.  RCCL takes the device
        tensor as it is -- the collective is queued behind whatever the current stream still has to do --, gloo a host copy."""
        import time
        import torch
        dist = _dist()
        nccl = dist.get_backend() == "nccl"
        if not nccl and packed.is_cuda:
            # gloo works from host memory, and the copy to the host waits for the whole sweep: it is made in _gather_finish -- after the
            # host has drawn the next sweep's random inputs (host_overlap) -- and is not counted as time inside the collective
            return ("deferred", packed)
        t0 = time.perf_counter()
        counts = [shard_bounds(self.N, self.world, r) for r in range(self.world)]
        # rows per rank in the gathered buffer: the largest shard (N not a multiple of the world size: smaller shards are padded with zero
        # rows); _gather_min_rows (test hook) forces padding where every shard is equal -- e.g. on the one rank a one-GPU box has
        maxc = max(max(hi - lo for lo, hi in counts), int(getattr(self, "_gather_min_rows", 0)))
        if nccl and not packed.is_cuda:
            packed = packed.to(self._comm_dev())
        if packed.shape[0] < maxc:
            pad = torch.zeros((maxc, packed.shape[1]), dtype=torch.uint8, device=packed.device)
            pad[:packed.shape[0]] = packed
            packed = pad
        out = torch.empty((self.world * maxc, packed.shape[1]), dtype=torch.uint8, device=packed.device)
        work = dist.all_gather_into_tensor(out, packed.contiguous(), async_op=True)
        self.comm_seconds += time.perf_counter() - t0
        self.collectives += 1
        return work, out, counts, maxc, packed

    def _gather_finish(self, handle):
        """-> (A, W, b, eta, row statistics, beta or None) of ALL neurons as host arrays"""
        import time
        if handle[0] == "deferred":
            handle = self._gather_start(handle[1].cpu())         # (the wait for the sweep is the sweep's time, not the collective's)
        t0 = time.perf_counter()
        work, out, counts, maxc, _keep = handle
        work.wait()
        if out.is_cuda:
            # into a pinned buffer kept across sweeps (a fresh pageable 43 MB array per sweep costs several times the transfer)
            import torch
            hb = getattr(self, "_gather_host", None)
            if hb is None or hb.shape != out.shape:
                hb = self._gather_host = torch.empty(out.shape, dtype=torch.uint8).pin_memory()
            hb.copy_(out)
            host = hb.numpy()
        else:
            host = out.numpy()
        if all(hi - lo == maxc for lo, hi in counts):
            rows = host                                    # equal shards, no padding: the gathered buffer IS the N rows
        else:
            rows = np.concatenate([host[r * maxc: r * maxc + (hi - lo)] for r, (lo, hi) in enumerate(counts)], axis=0)
        self.comm_seconds += time.perf_counter() - t0
        return self._unpack_rows(rows)

    def log_likelihood(self, datas=None, covariates=None):
        """(models.py:82-96) sum over datasets and neurons; `datas` other than the stored data is evaluated through a
        temporary engine.  covariates: with datas, in a model with covariates: [S, ...] parallel to datas."""
        self._refuse_heldout_latents("log_likelihood()", datas)
        if datas is None:
            if covariates is not None:
                raise ValueError("log_likelihood(): covariates= goes with datas=; the stored data carry their own")
            eng = self.engine
        else:
            eng = self._heldout_engine(datas, covariates)
        self._sync_covariates(eng)
        a, W, b = self._local_state()
        if self.engine_obs() == "gaussian":
            eng.set_noise([r.eta for r in self.regressions[self.n0:self.n1]])
        elif self._learns_xi():
            self._push_xi(eng)
        ll_loc = np.asarray(eng.log_likelihood(a, W, b), dtype=np.float64).reshape(-1)       # one value per local neuron
        return float(np.sum(self._all_neurons(ll_loc)))

    def _all_neurons(self, loc):
        """per-neuron values of this rank's neurons, (nloc,) or (k, nloc) -> those of ALL neurons, (N,) or (k, N), on every rank.  No process
        group: `loc` itself.  Otherwise the only collective on the likelihood path: ONE all_reduce -- of the N per-neuron values, each rank
        contributing its own entries and zeros elsewhere (x + 0 is exact, so the reduction's order cannot matter); the caller sums them in
        neuron order on every rank: the total is the same to the last bit whatever the number of ranks (a scalar all_reduce of per-rank
        sums regroups the additions; 8 N bytes instead of 8 cost nothing on xGMI)"""
        dist = _dist()
        if dist is None:
            return loc
        import time
        import torch
        t0 = time.perf_counter()
        vec = np.zeros(loc.shape[:-1] + (self.N,))
        vec[..., self.n0:self.n1] = loc
        t = torch.from_numpy(vec)
        if dist.get_backend() == "nccl":
            t = t.to(self._comm_dev())
        dist.all_reduce(t)
        out = t.cpu().numpy()
        self.comm_seconds += time.perf_counter() - t0
        self.collectives += 1
        return out

    def summarize(self, rates=True, pointwise=False, datas=None, covariates=None):
        """a posterior accumulator bound to this model (pyglm_amd/summary.py): call its collect() after every sweep to be kept, read
        edge_prob / weight_mean / rate_mean / lppd() ... at the end.  Allocates its accumulators (on the device, next to the data);
        changes nothing in the chain.  datas, covariates: as for log_likelihood -- None: the stored data; a list: held-out data (and
        their covariates).  In a model with covariates the summary also keeps covariate_mean / covariate_var, (N, K)."""
        from .summary import PosteriorSummary
        self._refuse_heldout_latents("summarize()", datas)
        return PosteriorSummary(self, rates=rates, pointwise=pointwise, datas=datas, covariates=covariates)

    def diagnose(self, levels=8, weights=True, rb=True):
        """chain diagnostics bound to this model (pyglm_amd/diagnostics.py: ChainDiagnostics): call its collect() after every sweep to be
        kept, read mcse(...) / ess(...) / min_ess() / edge_prob_rb / rb_gain at the end, compare chains with diagnostics.rhat.  levels:
        dyadic batch sizes kept, 1 .. 16 (3 x levels doubles per entry, on the device).  weights=False leaves the N x N x B effective weights
        out.  rb: also average the sweep's conditional edge probabilities (the Rao-Blackwell estimator): turns the engine's keep_logodds
        on, which changes nothing in the chain; refused for a model with an engine_factory."""
        from .diagnostics import ChainDiagnostics
        return ChainDiagnostics(self, levels=levels, weights=weights, rb=rb)

    def _heldout_engine(self, datas, covariates=None):
        """likelihood-only engine (X', Y, Psi: no sweep buffers, no residue planes) for data other than the stored data, on THIS shard's
        device; cached by content, so evaluating the same held-out set every iteration uploads it once.  covariates: [S, ...] parallel to
        datas in a model with covariates (required there, refused elsewhere); the engine gets the model's current beta"""
        from .utils.utils import fingerprint
        from .engine import GibbsEngine
        from . import covariates as _cov
        self._refuse_heldout_latents("held-out data", datas)
        items = []
        if covariates is not None and len(covariates) != len(datas):
            raise ValueError("covariates: %d entries for %d held-out data sets" % (len(covariates), len(datas)))
        for j, d in enumerate(datas):
            X, Y = d if isinstance(d, tuple) else (None, d)
            if isinstance(X, _LazyX):
                X = None
            S = _cov.check_covariates(None if covariates is None else covariates[j], np.asarray(Y).shape[0], self.K_obs, "held-out data set %d" % j)
            items.append((X, np.asarray(Y), S))
        key = tuple((None if X is None else fingerprint(X), fingerprint(Y), None if S is None else fingerprint(S)) for X, Y, S in items)
        cache = getattr(self, "_heldout_cache", None)
        if cache is None or cache[0] != key:
            self._heldout_cache = None
            obs, xi = self._engine_mode if self._engine is not None else _regression.device_obs(self.regressions)
            kw = dict(obs=obs, xi=xi, likelihood_only=True)
            if self.K:
                kw.update(n_covariates=self.K, covariate_prior=self._covariate_prior)
            if self._engine_factory is not None:
                eng = self._engine_factory(self.N, self.B, self.n0, self.n1, **kw)
            else:
                eng = GibbsEngine(self.N, self.B, self.n0, self.n1, device=self.engine.dev, **kw)
            for X, Y, S in items:
                _regression.check_counts(self.regressions, Y)
                ckw = dict(covariates=S) if self.K else {}
                eng.add_data(Y, X=X, basis=self.basis, **ckw, **self._obs_terms_kw(Y))
            cache = self._heldout_cache = (key, eng)
        self._sync_covariates(cache[1])
        if self._learns_xi():
            self._push_xi(cache[1])              # (the cached engine was built at an earlier xi)
        return cache[1]

    def engine_obs(self):
        """the device observation model of the whole list of regressions (regression.device_obs): "bernoulli", "negbin", "gaussian",
        "binomial" or "hooks" -- the one the engine was built with, once it is"""
        mode = self._engine_mode if self._engine is not None else _regression.device_obs(self.regressions)
        return mode[0]

    @property
    def means(self):
        """(models.py:153-163) E[y | X] per dataset, (T, N): per neuron, from its own observation model"""
        a, W, b = self._local_state()
        self._sync_covariates()
        obs, par = self._engine_mode if self._engine is not None else _regression.device_obs(self.regressions)
        if self._learns_xi():
            obs, par = _regression.device_obs(self.regressions)      # xi as it is now (a user may have set r.xi since the last sweep)
        regs = self.regressions[self.n0:self.n1]
        if np.ndim(par):
            par = np.asarray(par, dtype=np.float64)[self.n0:self.n1]
        mus = []
        for i in range(len(self.data_list)):
            psi = self.engine.psi(a, W, b, i)
            mu = _regression.means_of_psi(regs, (obs, par), psi, X=lambda: np.asarray(self.data_list[i][0]))
            mus.append(self._gather_rows(np.ascontiguousarray(mu.T)).T)
        return mus

    def _generate_obs(self, gpu):
        """which device path generate(gpu=...) takes: simulate.OBS_BERNOULLI / OBS_GAUSSIAN, or None for the host loop.  The device draws
        exactly what the built-in Bernoulli and Gaussian rvs draw; any other rvs (negative binomial: npr.negative_binomial uses the stream
        according to the values it draws; a user's override) keeps the host loop, and so does a model with an engine_factory"""
        if gpu is False:
            return None
        reg = self.regressions[0]
        model = _regression.builtin_model(reg, "rvs")
        obs = None if model is None else model.generate
        if obs is None or self._engine_factory is not None:
            if gpu:
                raise ValueError("generate(gpu=True): the device path simulates the built-in Bernoulli and Gaussian observations of a model "
                                 "without an engine_factory; %s.rvs%s keeps the host loop (gpu=None or False)"
                                 % (type(reg).__name__, "" if self._engine_factory is None else " with an engine_factory"))
            return None
        if not gpu:
            import torch
            if not torch.cuda.is_available():
                return None
        return obs

    def generate(self, keep=True, T=100, verbose=False, intvl=10, gpu=None):
        """(models.py:98-151) forward simulation, serial in t.  gpu=None: on the GPU (pyglm_amd/simulate.py, pgl_generate) whenever one is
        available and the observation model is the built-in Bernoulli or Gaussian one, else the host loop; gpu=True: on the GPU or an
        error; gpu=False: the host loop.  Both paths draw NumPy's global generator in the same order and return the same (X, Y)."""
        self._refuse_covariates("generate()")
        if T == 0:
            return np.zeros((0, self.N))
        assert isinstance(T, int), "Size must be an integer number of time bins"
        N, B = self.N, self.B
        L = self.basis.shape[0]
        flipped = self.basis[::-1]                      # row 0 of the basis = previous bin
        assert not np.allclose(flipped, self.basis)
        Wm = self.weights.reshape(N, N * B)               # as the reference: the stored W, not a*W
        bias = self.biases
        obs = self._generate_obs(gpu) if T > 0 else None
        if obs is not None:
            from . import simulate
            # (only regressions[0].rvs is called, for every neuron -- the reference's quirk -- and so only its eta is the noise)
            scale = float(np.sqrt(self.regressions[0].eta)) if obs == simulate.OBS_GAUSSIAN else 0.0
            X, Y = simulate.generate(Wm, bias, self.basis, T, obs, scale, device=self._device, verbose=verbose, intvl=intvl)
            if keep:
                self.add_data(Y, X=X)
            return X, Y
        Y = np.zeros((T + L, N))
        X = np.zeros((T + L, N, B))
        for t in range(L, T + L):
            if verbose and t % intvl == 0:
                print("Generate t={}".format(t))
            X[t] = Y[t - L:t].T.dot(flipped)
            psi = Wm.dot(X[t].reshape(N * B)) + bias
            Y[t] = self.regressions[0].rvs(psi=psi)
        if keep:
            self.add_data(Y[L:], X=X[L:])
        return X[L:], Y[L:]

    def simulate(self, T, replicates=1, seed=0, first_replicate=0, history=None, keep_paths=True, gpu=None, t0=None, lags=0, lagged_on_device=False,
                 isi=0, covariates=None, latents=None, data=0):
        """Posterior predictive simulation: `replicates` independent trajectories of T bins from the model's CURRENT state, every neuron
        drawing from its own regression's observation model (Bernoulli, Gaussian, negative binomial, binomial; mixed lists work).  Unlike
        generate() -- which stays the reference's loop, quirks included -- the activation is that of `means` and log_likelihood(),
        psi = (a*W) . x + b, and the random numbers are the package's own Philox stream keyed by (seed, replicate, neuron, time bin): replicate
        r = first_replicate + i depends on (seed, r, the state, its initial history) and on nothing else -- not on NumPy's global generator,
        on `replicates`, or on where the run is cut into calls (pyglm_amd/simulate.py states the law).

        Returns a simulate.Simulation: Y (R, T, N) float64, or None with keep_paths=False; sum and sumsq (R, N), the sums of y and y^2 over
        the bins; history (R, L, N), the last L bins of every replicate; t0, t1.  It unpacks as (Y, sum, sumsq, history).
        history: None -- from silence at bin t0 (default 0); a Simulation -- continue its trajectories from its t1 (T1 bins, then T2 bins from
        the result, are the T1 + T2 bins of one call); an array (rows, N) -- e.g. the last L rows of a recording, shared by all replicates:
        a forecast -- or (R, rows, N); an array starts at bin t0.
        gpu=None: on the device (pgl_simulate) when there is one, else the NumPy path; True: the device or a PglError; False: NumPy.  Both
        follow the same law; a model with an engine_factory takes the NumPy path.  With keep_paths=True the device path checks that the
        paths fit into free device memory first and raises with the number of bytes needed.  A negative-binomial draw that reaches
        simulate.NEGBIN_CAP raises PglError naming bin, replicate and neuron.
        lags = K > 0 (K <= simulate.PGL_LAG_MAX, K - 1 < T): the Simulation also carries `lagged` (R, K, N, N), lagged[r, l, i, j] =
        sum_t Y_r[t, i] Y_r[t+l, j] over the T bins of this call (never pairing a bin with the initial history), and correlogram().  On the
        device the sums are folded after every launch by pgl_lagged_products -- on the int8 matrix cores, exactly, when the neurons are
        Bernoulli or binomial; negative-binomial neurons fall back to fp64 for the chunks in which a count passes 127; fp64 if a neuron is
        Gaussian -- with keep_paths=False too; the memory they need is checked first.  lagged_on_device leaves `lagged` a torch tensor.
        isi = D (2 <= D <= simulate.PGL_ISI_MAX_BINS): the Simulation also carries `isi` (R, N, D) and `isi_moments` (R, N, 3), the
        inter-spike-interval histogram and (M, sum d, sum d^2) of every train (simulate.isi_host), and isi_density(), isi_mean(), isi_cv().
        A bin with a positive count is one event, whatever the count; a Gaussian neuron has no events and is refused by name.  The
        intervals are those between the events of the T bins of this call: continuing from a `history=` does not count the interval from
        the history's last event.  On the device pgl_isi_fold folds them after every launch.
        A model with n_covariates = K_obs > 0 needs covariates=: an array (T, K_obs), finite, row k for the k-th simulated bin (bin t0 + k),
        shared by all replicates ('data': the first T rows of data set `data`'s own).  A model with n_latents = Q > 0 needs latents=:
        'prior' -- every replicate draws its own path from the model's prior, N(0, I) per bin or the stationary AR(1) process of latent_ar
        (simulate.latent_prior_host; a forecast restarts the factors from the stationary law) --, 'fitted' -- the current sampled latents of
        data set `data`, shared by all replicates, T <= its length --, or an array (T, Q) or (replicates, T, Q), used as given.  The
        activation then is psi = ((a*W) . x + b) + o, o = covariates.offset_host([covariates | latents], [covariate_weights |
        latent_loadings]).  The Simulation carries latents (with keep_paths=True) and latent_last; continuing from it with latents='prior'
        continues the factors' paths as well.  Without the keyword its term needs, such a model raises the ValueError it always raised.
        On a sharded model every rank holds the gathered state: each rank computes the same result on its own device, with no collective."""
        from . import simulate as _sim
        self._refuse_covariates("simulate()", covariates, latents, keywords=True)
        drive = self._drive("simulate()", T, replicates, covariates, latents, data)
        A, W, b = self._adopt_state()
        kind, par = _sim.observation_kinds(self.regressions)
        if _sim.check_isi_bins(isi):
            self._refuse_gaussian_intervals("simulate(isi=%d)" % isi)
        if self._engine_factory is not None and gpu:
            raise ValueError("simulate(gpu=True): a model with an engine_factory takes the NumPy path (gpu=None or False)")
        Wm = (W * A[:, :, None]).reshape(self.N, self.N * self.B)
        return _sim.simulate(Wm, b.ravel(), np.asarray(self.basis, dtype=np.float64), kind, par, T, replicates=replicates, seed=seed,
                             first_replicate=first_replicate, history=history, keep_paths=keep_paths, t0=t0, on_device=self._on_gpu(gpu, "simulate"),
                             device=self._device, lags=lags, lagged_on_device=lagged_on_device, isi=isi, **(dict(drive=drive) if drive else {}))

    def _refuse_gaussian_intervals(self, what):
        from . import simulate as _sim
        bad = _sim.first_without_events(_sim.observation_models(self.regressions))
        if bad is not None:
            raise ValueError("%s: neuron %d is Gaussian; an inter-spike interval needs events, which a Gaussian neuron does not have" % (what, bad))

    def _on_gpu(self, gpu, method, host_only=False):
        """the tri-state gpu= of `method` -> bool.  A model with an engine_factory (or host_only) stays on the host; None: the GPU if there is
        one; True: the GPU or a PglError"""
        if self._engine_factory is not None or host_only or not (gpu is None or gpu):
            return False
        import torch
        if not torch.cuda.is_available():
            if gpu:
                from ._lib import PglError
                raise PglError("%s(gpu=True) needs a ROCm GPU (torch.cuda.is_available() is False)" % method)
            return False
        return True

    def isi_histogram(self, data=0, bins=64, gpu=None):
        """the inter-spike-interval statistics of data set `data` -> (hist (N, bins), moments (N, 3)), int64 (simulate.isi_host states them: a
        bin with a positive count is one event).  gpu as for simulate(); on the device they come from one pgl_isi_fold call."""
        from . import simulate as _sim
        D = _sim.check_isi_bins(bins)
        if D < 2:
            raise ValueError("isi_histogram(): bins >= 2 is required")
        self._refuse_gaussian_intervals("isi_histogram()")
        Y = np.asarray(self.data_list[data][1], dtype=np.float64)
        return _sim.isi_device(Y, D, device=self._device) if self._on_gpu(gpu, "isi_histogram") else _sim.isi_host(Y, D)

    def cross_correlogram(self, data=0, lags=1, gpu=None):
        """the observed lagged cross-correlogram of data set `data`, (lags, N, N): c[l, i, j] says whether neuron i firing at t predicts neuron j
        firing l bins later (simulate.correlogram).  gpu as for simulate(); on the device the sums come from pgl_lagged_products, on the int8
        matrix cores if the data are integers of [-127, 127]."""
        from . import simulate as _sim
        Y = np.asarray(self.data_list[data][1], dtype=np.float64)
        K = _sim.check_lags(lags, Y.shape[0])
        if K < 1:
            raise ValueError("cross_correlogram(): lags >= 1 is required")
        S = _sim.lagged_products_device(Y, K, device=self._device) if self._on_gpu(gpu, "cross_correlogram") else _sim.lagged_products_host(Y, K)
        return _sim.correlogram(S, Y.sum(axis=0), (Y * Y).sum(axis=0), Y.shape[0])

    def predictive_check(self, replicates=8, seed=0, data=0, gpu=None, lags=0, isi=0, covariates=None, latents=None):
        """a posterior predictive check of data set `data` bound to this model (simulate.PredictiveCheck): call its collect() after every
        sweep to be kept -- it simulates `replicates` fresh trajectories of the data set's length from the current state --, read
        rate_quantiles(q) / fano_quantiles(q) / pvalue("rate" | "fano") at the end.  lags = K > 0 adds the lagged cross-correlogram, the
        statistic that sees the coupling: pvalue("xcorr"), xcorr_mean, xcorr_std, each (K, N, N).  isi = D >= 2 adds the statistics of the
        single train, which see refractoriness and bursting: pvalue("isi"), isi_mean, isi_std, each (N, D), and pvalue("cv"), cvs,
        cv_quantiles(q); a Gaussian neuron is refused by name.  Changes nothing in the chain.
        A model with covariates needs covariates= -- 'data', the data set's own, or an array of its shape --, one with latents needs latents=
        -- 'prior', fresh paths from the prior for every replicate: the check of the model as a generative one; or 'fitted', the data set's
        current sampled latents, shared by the replicates: the check given the inferred drive.  Every collect() hands them to simulate()."""
        from .simulate import PredictiveCheck, check_isi_bins
        self._refuse_covariates("predictive_check()", covariates, latents, keywords=True)
        if latents is not None and not (isinstance(latents, str) and latents in ("prior", "fitted")):
            raise ValueError("predictive_check(): latents=%r; 'prior' or 'fitted' is required" % (latents,))
        if self.K:
            data = range(len(self.data_list))[data]
            self._drive("predictive_check()", self.data_list[data][1].shape[0], replicates, covariates, latents, data)    # (refuses a wrong shape now, not at the first collect())
        if check_isi_bins(isi):
            self._refuse_gaussian_intervals("predictive_check(isi=%d)" % isi)
        return PredictiveCheck(self, replicates=replicates, seed=seed, data=data, gpu=gpu, lags=lags, isi=isi, covariates=covariates, latents=latents)

    def _conditional_inputs(self, free, data, start, stop):
        """what the conditional law (simulate.conditional_host) takes, read from the current state and data set `data` for the checked `free`
        and window -> dict(Wff (F, F*B), base (T', F), basis, kind, par (F,), hist (L, F), Y: the recording).  base comes from engine.psi on
        the state with the free columns of the adjacency set to zero, gathered over the shards as `means` gathers"""
        from . import simulate as _sim
        A, W, b = self._adopt_state()
        N, B = self.N, self.B
        L = self.basis.shape[0]
        kind, par = _sim.observation_kinds([self.regressions[n] for n in free])
        Wm = (W * A[:, :, None]).reshape(N, N * B)
        cols = (free[:, None] * B + np.arange(B)[None, :]).ravel()
        a, Wl, bl = self._local_state()
        self._sync_covariates()                          # (base comes through fold_data: it carries the covariates' offset)
        a = np.array(a, dtype=bool)
        a[:, free] = False
        if _dist() is None or self._shard_override:     # every column is local: only the window's free columns leave the engine
            if free[0] < self.n0 or free[-1] >= self.n1:
                raise ValueError("conditional simulation: this model holds neurons [%d, %d) only; free neuron %d is outside"
                                 % (self.n0, self.n1, free[0] if free[0] < self.n0 else free[-1]))
            eng = self.engine
            if hasattr(eng, "psi_columns"):
                base = eng.psi_columns(a, Wl, bl, data, free - self.n0, start, stop)
            else:
                base = np.asarray(eng.psi(a, Wl, bl, data), dtype=np.float64)[start:stop][:, free - self.n0]
        else:
            psi = np.asarray(self.engine.psi(a, Wl, bl, data), dtype=np.float64)[start:stop]
            base = self._gather_rows(np.ascontiguousarray(psi.T)).T[:, free]
        Y = np.asarray(self.data_list[data][1], dtype=np.float64)
        hist = np.zeros((L, free.size))
        h = Y[max(0, start - L):start][:, free]
        hist[L - h.shape[0]:] = h
        return dict(Wff=np.ascontiguousarray(Wm[free][:, cols]), base=np.ascontiguousarray(base, dtype=np.float64),
                    basis=np.asarray(self.basis, dtype=np.float64), kind=kind, par=par, hist=hist, Y=Y)

    def conditional_simulate(self, free, data=0, replicates=1, seed=0, first_replicate=0, start=0, stop=None, keep_paths=True, gpu=None):
        """Conditional simulation: the neurons `free` (distinct indices, at most simulate.PGL_COND_MAX_FREE) are drawn from the model's CURRENT
        state while every other neuron is clamped to the recording of data set `data`, over the window [start, stop) of its bins -- what
        the model says neuron j does GIVEN the rest of the population.  `means` does not answer that (it feeds the neuron's own recorded
        history through its self-coupling) and simulate() simulates everybody.  pyglm_amd/simulate.py (conditional_host) states the law: the
        clamped neurons enter through base = bias + their columns of a*W against the data set's regressors X -- a data set added with a
        caller's own X uses THAT X for the clamped part --, the free neurons through their own simulated history, which before `start` is
        the recording's; the random stream is simulate()'s, keyed by the global neuron index, so replicate r = first_replicate + i depends on
        (seed, r, the state, the recording, free, the window) and on nothing else.
        Returns a simulate.ConditionalSimulation: free; Y (R, T', F) or None (keep_paths=False); sum, sumsq (R, F), rate(), fano(); history
        (R, L, F); base (T', F); t0, t1; paths(r) -> (T', N), the recording's window with the free columns replaced by replicate r.
        gpu as for simulate(): None -- the device (pgl_conditional_simulate: one workgroup per replicate, no grid barrier) when there is
        one, True -- the device or a PglError, False -- NumPy; a model with an engine_factory takes the NumPy path.  An empty `free`, more
        than 256 free neurons, a duplicate, an index out of range and a window outside the recording are ValueErrors that name the offender.
        On a sharded model base is gathered; every rank then simulates the same thing."""
        from . import simulate as _sim
        data = range(len(self.data_list))[data]
        free = _sim.check_free(free, self.N)
        start, stop = _sim.check_window(start, stop, self.data_list[data][1].shape[0])
        if self._engine_factory is not None and gpu:
            raise ValueError("conditional_simulate(gpu=True): a model with an engine_factory takes the NumPy path (gpu=None or False)")
        on_device = self._on_gpu(gpu, "conditional_simulate")
        inp = self._conditional_inputs(free, data, start, stop)
        sim = _sim.conditional_simulate(inp["Wff"], inp["base"], inp["basis"], inp["kind"], inp["par"], free, replicates, seed, first_replicate,
                                        inp["hist"], start, keep_paths, on_device, self._device)
        sim._recording = inp["Y"]
        return sim

    def conditional_check(self, free, replicates=8, seed=0, data=0, start=0, stop=None, gpu=None):
        """the population-conditioned prediction of the neurons `free` of data set `data` bound to this model (simulate.ConditionalPrediction):
        call its collect() after every sweep to be kept -- it simulates `replicates` fresh conditional replicates over [start, stop) from the
        current state --, read rate_mean / rate_std (T', F), log_score() -> dict(total, per_neuron, per_bin) and count at the end.  Changes
        nothing in the chain."""
        from .simulate import ConditionalPrediction
        if self._engine_factory is not None and gpu:
            raise ValueError("conditional_check(gpu=True): a model with an engine_factory takes the NumPy path (gpu=None or False)")
        return ConditionalPrediction(self, free, replicates=replicates, seed=seed, data=data, start=start, stop=stop, gpu=gpu)

    def time_rescaling(self, bins=64, seed=0, coef=1.36, datas=None, covariates=None):
        """the time-rescaling goodness-of-fit test of the data under this model's chain (pyglm_amd/rescale.py: TimeRescaling): call its
        collect() after every sweep to be kept -- it reads the recorded data against the current rates, no replicate is simulated --, read
        ks_mean / band / exceed_fraction / failing() at the end.  bins: of the histogram of the rescaled z per neuron, whose binned
        Kolmogorov-Smirnov distance from the uniform law is the statistic; coef / sqrt(M) is the band (1.36: 95 %).  datas: as for
        summarize -- None: the stored data; a list: held-out recordings (covariates: theirs, in a model with covariates).  A Gaussian
        neuron is refused by name.  Changes nothing in the chain."""
        from .rescale import TimeRescaling
        self._refuse_heldout_latents("time_rescaling()", datas)
        return TimeRescaling(self, bins=bins, seed=seed, coef=coef, datas=datas, covariates=covariates)

    def rescaled_intervals(self, data=0, bins=64, seed=0, gpu=None):
        """the rescaled intervals of data set `data` at the CURRENT state -> (hist (N, bins) int64, zsum (N, 2) = (sum z, sum z^2))
        (rescale.rescale_host states them; Philox call 0 of `seed`).  gpu=None: through pgl_rescale_fold when there is a GPU, else the NumPy
        path from engine.psi; True: the device or a PglError; False: NumPy.  A model with an engine_factory takes the NumPy path."""
        from . import rescale as _rs
        D = _rs.check_bins(bins)
        par = _rs.interval_par(self.regressions)[self.n0:self.n1]
        data = range(len(self.data_list))[data]
        eng = self.engine
        a, W, b = self._local_state()
        self._sync_covariates()
        if self._on_gpu(gpu, "rescaled_intervals", host_only=not _rs.device_engine(eng)):
            acc = _rs._DeviceFold(eng, D, par, seed=seed)
            acc.fold(eng, a, W, b, 1, only=data)
            out = acc.read()
            hist, zsum = out["hist"], out["zsum"]
        else:
            Y = np.asarray(self.data_list[data][1], dtype=np.float64)[:, self.n0:self.n1]
            elem0 = sum(d[1].shape[0] for d in self.data_list[:data])
            hist, zsum, _ = _rs.rescale_host(np.asarray(eng.psi(a, W, b, data), dtype=np.float64), Y, par, D, seed, 0, self.n0, elem0)
        return self._gather_rows(np.ascontiguousarray(hist)), self._gather_rows(np.ascontiguousarray(zsum))

    # ---- Gibbs
    def resample_model(self):
        self.resample_regressions()

    def _sweep_inputs(self):
        """everything engine.sweep needs for the shard at the current chain state: (a, W, b, rho, Jw, hw, Jb, hb, c0, perm, u, z)"""
        from .engine import make_draws, prior_terms
        regs = self.regressions[self.n0:self.n1]
        a, W, b = self._local_state()
        versions = tuple(r._hyp_version for r in regs)
        cache = getattr(self, "_hyper_cache", None)
        # the cached terms are those of a network push (or of the last sweep) and are only trusted while nobody outside holds one of the
        # live hyper-parameter arrays (regression._handed_out): such a holder may edit in place at any time, as users of the reference do
        if cache is not None and cache[0] == versions and not any(r._handed_out for r in regs):
            rho, Jw, hw, Jb, hb, c0 = cache[1]          # pushed by resample_network and untouched since
        else:
            hyp = [r._hyper() for r in regs]            # internal read: does not mark the terms stale (the public properties do)
            rho = np.array([h[0] for h in hyp])
            S_w = np.array([h[1] for h in hyp])
            mu_w = np.array([h[2] for h in hyp])
            S_b = np.array([h[3][0, 0] for h in hyp])
            mu_b = np.array([h[4][0] for h in hyp])
            Jw, hw, Jb, hb, c0 = prior_terms(S_w, mu_w, S_b, mu_b)
            self._hyper_cache = (versions, (rho, Jw, hw, Jb, hb, c0))
        # the non-PG random inputs depend on (seed, sweep, neuron) only: those of the NEXT sweep are drawn while the GPU works on
        # this one (engine.sweep's host_overlap hook) and picked up here
        key = (self.seed, self.sweeps_done, self.n0, self.n1)
        pre = getattr(self, "_draws_ahead", None)
        if pre is not None and pre[0] == key:
            perm, u, z = pre[1]
        else:
            perm, u, z = make_draws(self.seed, self.sweeps_done, range(self.n0, self.n1), self.N, self.N * self.B)
        return a, W, b, rho, Jw, hw, Jb, hb, c0, perm, u, z

    def resample_regressions(self):
        """(models.py:169-171) all local neurons through the GPU engine, then ONE all_gather of the new rows (packed on the device and
        launched behind the sweep on its stream; the host draws the next sweep's random inputs meanwhile)."""
        from .engine import make_draws
        self._check_obs()
        regs = self.regressions[self.n0:self.n1]
        a, W, b, rho, Jw, hw, Jb, hb, c0, perm, u, z = self._sweep_inputs()
        self._draws_ahead = None

        def draw_ahead():
            nxt = (self.seed, self.sweeps_done + 1, self.n0, self.n1)
            self._draws_ahead = (nxt, make_draws(self.seed, self.sweeps_done + 1, range(self.n0, self.n1), self.N, self.N * self.B))
        gaussian = self.engine_obs() == "gaussian"
        learns = self._learns_xi()
        if gaussian:
            self.engine.set_noise([r.eta for r in regs])
        elif learns:
            self._push_xi()
        self._sync_covariates()
        kw = dict(host_overlap=draw_ahead) if self.N * self.N * self.B >= self.DRAW_AHEAD_MIN_SIZE else {}
        exchange = _dist() is not None and not self._shard_override
        handle = []
        if exchange and not gaussian and not learns and not self.K and hasattr(self.engine, "packed_state"):
            # the shard's new rows never visit the host on their own: packed from the sweep's device buffers, gathered, read back once
            kw.update(after_queue=lambda eng: handle.append(self._gather_start(eng.packed_state())), readback=False)
        need_stats = hasattr(getattr(self, "network", None), "weight_blocks")
        if hasattr(self.engine, "_hout_np"):
            kw["copy"] = False             # (the rows are stored into the model's arrays below, before the engine is used again)
            if need_stats and "readback" not in kw:
                kw["want_stats"] = True    # (taken behind the sweep, back in the same wait as the state)
        a, W, b, self.last_loglik_local = self.engine.sweep(a, W, b, rho, Jw, hw, Jb, hb, c0, perm, u, z, self.seed, self.sweeps_done, **kw)
        if handle:
            A_all, W_all, b_all, flags, stats_all, _ = self._gather_finish(handle[0])
            if np.any(flags != 0):
                # (the eta slot of a non-Gaussian row carries the sweep's status flags: every rank sees them all and raises the same error,
                # with its state as it was before the sweep -- regression.py:369-370 raises LinAlgError from np.linalg.cholesky)
                bad = np.nonzero(flags)[0]
                err = np.linalg.LinAlgError("posterior system not positive definite for neurons %s (flags %s)"
                                            % (bad[:8].tolist(), flags[bad[:8]].astype(int).tolist()))
                err.neurons, err.flags, err.state = bad.tolist(), flags[bad].astype(int).tolist(), None
                raise err
            self.sweeps_done += 1
            self._store_rows(0, self.N, A_all, W_all, b_all)
            self._fresh_stats = stats_all
            return
        cov_beta = None
        if self.K:
            # the covariate weights, directly behind the sweep and before every other step (eta, xi, the network): from the omega the sweep
            # has just drawn and the weights it returned; the engine's offsets follow, so what comes next sees the new beta
            # -- with latents x | omega, W, b, beta first: Off must still hold the offset the sweep ran under when beta's fold recovers kappa,
            # and beta is then drawn given the new x; the latent step leaves Psi and the weights in place for it
            if self.Q:
                self._lat_step.latent_step(a, W, b, self.seed, self.sweeps_done)
            cov_beta = self._cov_step.covariate_step(a, W, b, self.seed, self.sweeps_done, **(dict(psi_ready=True) if self.Q else {}))
        if gaussian:
            # noise variances (regression.py:433-445): residual sums of squares under the NEW weights from the device, gamma draws
            # keyed by the global neuron index
            from .engine import make_gamma_draws
            T_total = sum(d[1].shape[0] for d in self.data_list)
            sse = self.engine.sse(a, W, b)
            eta = np.empty(len(regs))
            for i, r in enumerate(regs):
                alpha, beta = r.eta_posterior(T_total, sse[i])
                eta[i] = 1.0 / (make_gamma_draws(self.seed, self.sweeps_done, [self.n0 + i], alpha)[0] * (1.0 / beta))
        elif learns:
            # the dispersions (dispersion.py): the CRT table counts and sum log(1 + e^psi) under the NEW weights; with several ranks xi
            # rides in the rows' eta slot, on the exchange path the Gaussian model takes
            eta = self._resample_xi(a, W, b)
        self.sweeps_done += 1
        # the rows' sufficient statistics for the network prior (networks.py:132-149), from the state the sweep left on the device
        stats = None
        if need_stats:
            stats = getattr(self.engine, "last_row_stats", None)
            if stats is not None:
                stats = stats.copy()
            else:
                stats = self.engine.row_stats().cpu().numpy() if hasattr(self.engine, "row_stats") else host_row_stats(a, W, self.n0)
        if self._shard_override:
            # (only this shard's rows move: the statistics of the others are formed once and kept -- bench.py --neurons, tools)
            keep = getattr(self, "_stats_kept", None)
            if stats is not None:
                if keep is None:
                    A_, W_, _ = self._adopt_state()
                    keep = self._stats_kept = host_row_stats(A_, W_, 0)
                keep[self.n0:self.n1] = stats
            self._store_rows(self.n0, self.n1, a, W, b)
            if self.K:
                self._beta[self.n0:self.n1] = cov_beta
            self._fresh_stats = keep if stats is not None else None
            if gaussian:
                for i, r in enumerate(regs):
                    r.eta = float(eta[i])
            elif learns:
                self._store_xi(self.n0, eta)
            return
        if not exchange:
            A_all, W_all, b_all, eta_all, stats_all = a, W, b, (eta if gaussian or learns else None), stats
            if self.K:
                self._beta[self.n0:self.n1] = cov_beta
        else:
            import torch
            packed = torch.from_numpy(self._pack_rows_host(a, W, b, eta if gaussian or learns else None, stats, cov_beta))
            A_all, W_all, b_all, eta_all, stats_all, beta_all = self._gather_finish(self._gather_start(packed))
            if self.K:
                self._beta = beta_all
        self._store_rows(0, self.N, A_all, W_all, b_all)
        self._fresh_stats = stats_all
        if gaussian:
            for n, r in enumerate(self.regressions):
                r.eta = float(eta_all[n])
        elif learns:
            self._store_xi(0 if exchange else self.n0, eta_all)

    # ---- chain state (checkpoint / resume; also lets two samplers be run from one state)
    _STATE_ATTRS = ("regressions", "sweeps_done", "_hyper_cache", "network", "_beta")

    def get_state(self):
        """deep copy of everything a sweep reads or writes on the host: the regressions (a, W, b, hyper-parameters, noise variances), the
        network prior, the sweep counter (the random inputs are keyed by (seed, sweep, neuron)) and the cached natural-parameter terms.
        Device buffers hold no chain state between sweeps.  `set_state(get_state())` resumes the chain exactly."""
        import copy
        keep = {}
        for r in self.regressions:               # stand-alone engines hold device memory and are not chain state
            keep[id(r)] = (r.__dict__.pop("_engine_cache", None), r.__dict__.pop("_lik_engine_cache", None))
        try:
            st = {k: copy.deepcopy(getattr(self, k)) for k in self._STATE_ATTRS if hasattr(self, k)}
        finally:
            for r in self.regressions:
                r._engine_cache, r._lik_engine_cache = keep[id(r)]
        st["seed"] = self.seed
        if self.Q:
            st["latents"] = self.latents             # (the one piece of chain state that lives on the device: read back here)
        return st

    def set_state(self, state):
        import copy
        assert state["seed"] == self.seed, "state of a chain with another seed"
        for k in self._STATE_ATTRS:
            if k in state:
                setattr(self, k, copy.deepcopy(state[k]))
        for r in self.regressions:
            r._engine_cache = r._lik_engine_cache = None
        self._st = None                          # the restored regressions share copies of the state arrays: link the model to those
        r0 = self.regressions[0]
        if r0._store is not None and all(r._store is not None and r._store[0] is r0._store[0] for r in self.regressions):
            self._st = r0._store[:3]
        self._adopt_state()
        self._draws_ahead = None
        self._fresh_stats = self._stats_kept = None
        if self.Q and "latents" in state:
            self._sync_covariates()
            for i, X in enumerate(state["latents"]):
                self.engine.set_latents(i, X)

    def plot(self, *args, **kwargs):
        raise NotImplementedError("plotting is outside the scope of the MI355X hot path (SURVEY.md section 2, row 8)")


class _LazyX(object):
    """stands for the device-resident design matrix in data_list; materialises on the host only when indexed"""

    def __init__(self, engine, i):
        self.engine, self.i = engine, i

    def __array__(self, dtype=None, copy=None):
        return self.engine.design_matrix(self.i)

    @property
    def shape(self):
        ds = self.engine.datasets[self.i]
        return (ds.T, self.engine.N, self.engine.B)


class HierarchicalNonlinearAutoregressiveModel(NonlinearAutoregressiveModel):
    """(models.py:204-236) adds the network prior over the regressions' hyper-parameters."""

    def __init__(self, N, network, regressions, basis=None, B=10, **kw):
        super(HierarchicalNonlinearAutoregressiveModel, self).__init__(N, regressions, basis=basis, B=B, **kw)
        self.network = network
        self.network_gpu = None          # where a learned adjacency prior scans its block assignments: the tri-state gpu= of simulate()

    def resample_model(self):
        self._fresh_stats = None
        super(HierarchicalNonlinearAutoregressiveModel, self).resample_model()
        stats, self._fresh_stats = self._fresh_stats, None     # the rows' statistics of exactly the state the regressions' sweep just stored
        self.resample_network(_row_stats=stats)

    def _network_stats(self, row_stats):
        """((n, sum w, sum w w') off the diagonal, the same on it) from the per-row statistics every rank holds after the gather: N rows of
        1 + B + B^2 doubles added up in neuron order (the same bits whatever the sharding), and the N self-connections read off (A, W)"""
        A, W, _ = self._adopt_state()
        B = self.B
        tot = np.sum(np.asarray(row_stats, dtype=np.float64), axis=0)
        r = np.arange(self.N)
        d = A[r, r]
        Wd = W[r, r, :] * d[:, None]
        return (tot[0], tot[1:1 + B], tot[1 + B:].reshape(B, B)), (float(d.sum()), Wd.sum(axis=0), Wd.T.dot(Wd))

    def resample_network(self, _row_stats=None):
        """(models.py:228-236).  Every rank holds the full (A, W) after the all_gather and draws the same network
        parameters from an identically seeded host generator; the push evaluates mu_W / sigma_W / rho once
        instead of once per row.  Inside resample_model() the network's sufficient statistics come from the per-row statistics the ranks
        exchanged with their rows (_row_stats; O(N B^2) on every rank); called on its own -- the state may have been edited since the last
        sweep -- the network walks (A, W) as the reference does."""
        net = self.network
        if hasattr(net, "_set_rng"):
            # the package's own NIW networks draw from a generator keyed by (seed, sweep) -- identical on every rank, and 20 us to make where
            # re-seeding NumPy's global Mersenne twister and putting it back costs 110 (a sixth of a sweep at BASELINE configs[0])
            net._set_rng(np.random.RandomState(np.random.Philox(key=self.seed & (2 ** 64 - 1), counter=[self.sweeps_done, 0, 2, 0])))
            # a learned adjacency prior (networks._StochasticBlockAdjacencyMixin) scans its block assignments on the Philox stream
            # (seed, sweep), on this rank's device where there is one: the same update on every rank from the gathered state, no collective
            scan_hook = getattr(net, "_set_scan", None)
            if scan_hook is not None:
                scan_hook(self.seed, self.sweeps_done, self._network_device())
            try:
                if _row_stats is not None:
                    net.resample(self._adopt_state()[:2], stats=self._network_stats(_row_stats))
                else:
                    net.resample(self._adopt_state()[:2])         # (the network only reads them)
            finally:
                net._set_rng(None)
                if scan_hook is not None:
                    scan_hook(None)
        else:
            state = npr.get_state()
            npr.seed((self.seed * 1000003 + self.sweeps_done) % (2 ** 32))      # a user's network class draws from NumPy's global generator: identical on every rank
            try:
                net.resample(self._adopt_state()[:2])
            finally:
                npr.set_state(state)
        if hasattr(net, "weight_blocks"):
            # one shared block (+ one for self-connections): pushed as such -- the (N, N, B, B) expansion of sigma_W is 210 MB at N = 1024,
            # a fifth of a second of host time per sweep on every rank, and nothing on the hot path reads it
            mu_off, S_off, mu_self, S_self = net.weight_blocks()
            rho = net.rho
            for n, reg in enumerate(self.regressions):
                reg._push_block_prior(mu_off, S_off, mu_self, S_self, n, rho[n])
            self._cache_block_hypers(mu_off, S_off, mu_self, S_self, rho)
            return
        sigma, mu, rho = net.sigma_W, net.mu_W, net.rho
        for n, reg in enumerate(self.regressions):
            reg._set("_S_w", np.array(sigma[n]))      # (copies: the regression owns its hyper-parameters, as after the reference's setters)
            reg._set("_mu_w", np.array(mu[n]))
            reg._set("_rho", np.array(rho[n]))
        self._cache_pushed_hypers(sigma, mu, rho)

    def _network_device(self):
        """the device a learned adjacency prior updates on, or None for the host (an engine_factory, no GPU, network_gpu = False)"""
        if not self._on_gpu(self.network_gpu, "resample_network"):
            return None
        import torch
        return self._device or ("cuda:%d" % torch.cuda.current_device())

    def block_structure(self, gpu=None):
        """sbm.BlockStructure of this chain -- the co-assignment probabilities P(z_i = z_j), the mean of the pushed rho, the trace of
        occupied blocks -- for a network that learns a partition (SBMSparseNetwork, BetaBernoulliSparseNetwork).  collect() once per
        kept sweep.  gpu as for simulate(): the folds run on the device when there is one"""
        from .sbm import BlockStructure
        if not hasattr(self.network, "block_sizes"):
            raise TypeError("block_structure(): %s learns no partition" % type(self.network).__name__)
        return BlockStructure(self, device=self._device, gpu=self._on_gpu(gpu, "block_structure"))

    def _cache_block_hypers(self, mu_off, S_off, mu_self, S_self, rho):
        """natural-parameter terms of the shard's rows for a (shared block, self block) push: two table entries and the labels"""
        from .engine import prior_terms, BlockPrior
        n0, n1, N, B = self.n0, self.n1, self.N, self.B
        regs = self.regressions[n0:n1]
        nl = n1 - n0
        # (which block a pair takes never changes: the label table is built once per shard, not once per sweep)
        lkey = (n0, n1, N, S_self is not None)
        lc = getattr(self, "_label_cache", None)
        if lc is None or lc[0] != lkey:
            label = np.zeros((nl, N), dtype=np.int32)
            if S_self is not None:
                label[np.arange(nl), np.arange(n0, n1)] = 1
            lc = self._label_cache = (lkey, label)
        label = lc[1]
        S_u, mu_u = [S_off], [mu_off]
        if S_self is not None:
            S_u.append(S_self)
            mu_u.append(mu_self)
        Jw_u, hw_u, _, _, c0_u = prior_terms(np.array(S_u)[None], np.array(mu_u)[None], np.ones(1), np.zeros(1))
        prior = BlockPrior(Jw_u[0], hw_u[0], c0_u[0], label)
        S_b = np.array([r._S_b[0, 0] for r in regs])
        mu_b = np.array([r._mu_b[0] for r in regs])
        Jb = 1.0 / S_b
        self._hyper_cache = (tuple(r._hyp_version for r in regs), (np.array(rho[n0:n1], dtype=float), prior, None, Jb, Jb * mu_b, None))

    def _cache_pushed_hypers(self, sigma, mu, rho):
        """natural-parameter terms of the shard's rows for the hyper-parameters just pushed.  Network priors produce a
        handful of distinct (mu, Sigma) blocks (off-diagonal / self-connection), so the B x B inversions are done once per
        distinct block and scattered, instead of once per (n, m) pair."""
        from .engine import prior_terms
        n0, n1, N, B = self.n0, self.n1, self.N, self.B
        regs = self.regressions[n0:n1]
        sig = sigma[n0:n1].reshape(-1, B * B)
        mus = mu[n0:n1].reshape(-1, B)
        key = np.concatenate((sig, mus), axis=1)
        # label every row with the index of its distinct block: two frequent candidates first, np.unique for the rest
        label = np.full(key.shape[0], -1, dtype=np.int64)
        blocks = []
        for _ in range(2):
            todo = np.nonzero(label < 0)[0]
            if todo.size == 0:
                break
            cand = key[todo[0]]
            label[todo[np.all(key[todo] == cand, axis=1)]] = len(blocks)
            blocks.append(cand)
        todo = np.nonzero(label < 0)[0]
        if todo.size > 4 * (n1 - n0) + 8:                 # not a structured prior: let resample_regressions do the dense path
            self._hyper_cache = None
            return
        if todo.size:
            u_rest, inv = np.unique(key[todo], axis=0, return_inverse=True)
            label[todo] = len(blocks) + inv.reshape(-1)
            blocks.extend(list(u_rest))
        u = np.array(blocks)
        idx = label
        Jw_u, hw_u, _, _, c0_u = prior_terms(u[:, :B * B].reshape(1, -1, B, B), u[:, B * B:].reshape(1, -1, B), np.ones(1), np.zeros(1))
        nl = n1 - n0
        from .engine import BlockPrior
        prior = BlockPrior(Jw_u[0], hw_u[0], c0_u[0], idx.reshape(nl, N))      # tables + labels: never expanded to (nl, N, B, B)
        S_b = np.array([r._S_b[0, 0] for r in regs])
        mu_b = np.array([r._mu_b[0] for r in regs])
        Jb = 1.0 / S_b
        self._hyper_cache = (tuple(r._hyp_version for r in regs), (np.array(rho[n0:n1], dtype=float), prior, None, Jb, Jb * mu_b, None))


GLM = NonlinearAutoregressiveModel
NetworkGLM = HierarchicalNonlinearAutoregressiveModel


class _DefaultMixin(object):
    _network_class = None
    _regression_class = None

    def __init__(self, N, B=10, basis=None, network=None, network_kwargs=None, regressions=None, regression_kwargs=None, **kw):
        """(models.py:246-267)"""
        B = B if basis is None else basis.shape[1]
        if network is None:
            network = self._network_class(N, B, **(network_kwargs or {}))
        if regressions is None:
            regressions = [self._regression_class(N, B, **(regression_kwargs or {})) for _ in range(N)]
        super(_DefaultMixin, self).__init__(N, network, regressions, B=B, basis=basis, **kw)


class GaussianGLM(_DefaultMixin, NetworkGLM):
    """(models.py:270-272)"""
    _network_class = _networks.NIWDenseNetwork
    _regression_class = _regression.GaussianRegression


class SparseGaussianGLM(_DefaultMixin, NetworkGLM):
    """(models.py:274-276)"""
    _network_class = _networks.NIWSparseNetwork
    _regression_class = _regression.SparseGaussianRegression


class BernoulliGLM(_DefaultMixin, NetworkGLM):
    _network_class = _networks.NIWDenseNetwork
    _regression_class = _regression.BernoulliRegression


class SparseBernoulliGLM(_DefaultMixin, NetworkGLM):
    _network_class = _networks.NIWSparseNetwork
    _regression_class = _regression.SparseBernoulliRegression


class NegativeBinomialGLM(_DefaultMixin, NetworkGLM):
    _network_class = _networks.NIWDenseNetwork
    _regression_class = _regression.NegativeBinomialRegression


class SparseNegativeBinomialGLM(_DefaultMixin, NetworkGLM):
    _network_class = _networks.NIWSparseNetwork
    _regression_class = _regression.SparseNegativeBinomialRegression


class BinomialGLM(_DefaultMixin, NetworkGLM):
    _network_class = _networks.NIWDenseNetwork
    _regression_class = _regression.BinomialRegression


class SparseBinomialGLM(_DefaultMixin, NetworkGLM):
    _network_class = _networks.NIWSparseNetwork
    _regression_class = _regression.SparseBinomialRegression
