"""Posterior summaries accumulated sample by sample: edge probabilities, moments of the weights, the biases and the rates, and the pointwise
predictive density (lppd, WAIC).

The reference's workflow (examples/synthetic.py:51-84) appends log_likelihood(), weights, adjacency, biases and means[0] after every sweep,
stacks them on the host and takes .mean(0) / .std(0).  One sample of the rates is a (T, N) array -- 819 MB at N = 1024, T = 100 000 -- so here
the running moments live on the device and each collected sample is folded into them in one fused pass (pgl_summary_fold, pgl_summary_state):

    acc = model.summarize(rates=True, pointwise=True)
    for it in range(n_sweeps):
        model.resample_model()
        if it >= burn:
            acc.collect()
    acc.edge_prob, acc.weight_mean, acc.rate_mean[0], acc.lppd(), acc.waic()

The accumulators are one of two classes with one interface: _DeviceAccumulators owns them in the memory of the engine's GPU and folds through
the kernels; _HostAccumulators, for a model with an engine_factory, folds on the host from engine.psi(...), with the update formulas of the
kernels written in NumPy -- their specification, and what runs without a GPU.  The time-rescaling test (rescale.py) and the chain
diagnostics (diagnostics.py) are built the same way and share the three helpers below.
"""
import numpy as np
import torch

from . import regression as _regression
from ._lib import call, ptr
from .engine import I32, _on_device
from .regression import OBS_GAUSSIAN, OBS_HOOKS


def _welford(mean, M2, x, k):
    """step k (1-based) of the running mean / sum of squared deviations, in place -- the update of the kernels"""
    d = x - mean
    mean += d / k
    M2 += d * (x - mean)


def device_engine(eng):
    """whether the read-outs of the chain keep their accumulators on eng's GPU: a GibbsEngine, which walks its data sets on the device
    (fold_data); any other engine (an engine_factory's) gets the NumPy twins"""
    return hasattr(eng, "fold_data")


def model_data(model, datas, what, covariates=None):
    """what a read-out of the chain folds over -> (engine, [Y of every data set]): the model's own engine and stored data, or (datas: a
    list of held-out recordings; covariates: theirs, in a model with covariates) the model's held-out engine of them"""
    if datas is None and covariates is not None:
        raise ValueError("%s: covariates= goes with datas=; the stored data carry their own" % what)
    if datas is not None:
        eng = model._heldout_engine(datas, covariates)                   # held on to by the caller: the model's cache keeps one held-out engine only
        Ys = [np.asarray(d[1] if isinstance(d, tuple) else d) for d in datas]
    else:
        eng, Ys = model.engine, [d[1] for d in model.data_list]
    if not Ys:
        raise ValueError("%s: the model has no data" % what)
    return eng, Ys


class _HostAccumulators(object):
    """the accumulators and the per-sample fold in NumPy, for an engine without device accumulators.  The log-likelihood term l is formed from
    psi and the regressions' own a_func / b_func / c_func (eta for Gaussian observations), the rate from psi by the neuron's own model."""

    def __init__(self, summary, Ys):
        self.s = summary
        model = summary.model
        regs = model.regressions[model.n0:model.n1]
        self.Y = [np.asarray(Y, dtype=np.float64)[:, model.n0:model.n1] for Y in Ys]
        self.terms = None if summary.obs == "gaussian" else [_regression.obs_terms(regs, Y) for Y in self.Y]
        self._terms_xi = [float(getattr(r, "xi", 0.0)) for r in regs]
        self.reset()

    def reset(self):
        s, m = self.s, self.s.model
        nl, z = m.n1 - m.n0, np.zeros
        self.edge, self.w, self.b = z((nl, m.N)), (z((nl, m.N, m.B)), z((nl, m.N, m.B))), (z(nl), z(nl))
        self.rate = [(z(Y.shape), z(Y.shape)) for Y in self.Y] if s.rates else None
        self.pw = [tuple(z(Y.shape) for _ in range(4)) for Y in self.Y] if s.pointwise else None

    def _rate(self, psi):
        m = self.s.model
        regs = m.regressions[m.n0:m.n1]
        model = _regression.MODELS.get(self.s.obs)
        par = None if model is None else np.array([model.par(r) for r in regs])
        return _regression.means_of_psi(regs, (self.s.obs, par), psi)

    def fold(self, eng, a, W, b, k):
        s, m = self.s, self.s.model
        a, W, b = np.asarray(a).astype(bool), np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(-1)
        ll = np.asarray(eng.log_likelihood(a, W, b), dtype=np.float64).reshape(-1)
        for i, Y in enumerate(self.Y):
            if not (s.rates or s.pointwise):
                break
            psi = np.asarray(eng.psi(a, W, b, i), dtype=np.float64)
            if s.rates:
                _welford(self.rate[i][0], self.rate[i][1], self._rate(psi), k)
            if s.pointwise:
                if s.obs == "gaussian":
                    eta = np.array([r.eta for r in m.regressions[m.n0:m.n1]], dtype=np.float64)
                    l = -0.5 * np.log(2 * np.pi * eta) - (Y - psi) ** 2 / (2 * eta)
                else:
                    if i == 0 and m._learns_xi():
                        # b(y) = y + xi and log c(y) move with a learned xi: the terms are formed again when it has moved, as the Gaussian
                        # branch reads eta at every sample
                        regs = m.regressions[m.n0:m.n1]
                        xi_now = [float(getattr(r, "xi", 0.0)) for r in regs]
                        if xi_now != self._terms_xi:
                            self.terms, self._terms_xi = [_regression.obs_terms(regs, Yi) for Yi in self.Y], xi_now
                    A, Bv, logC = self.terms[i]
                    l = logC + A * psi - Bv * np.log1p(np.exp(psi))
                lmean, lM2, lm, ls = self.pw[i]
                _welford(lmean, lM2, l, k)
                if k == 1:
                    lm[...], ls[...] = l, 1.0
                else:
                    m1 = np.maximum(lm, l)
                    ls[...] = ls * np.exp(lm - m1) + np.exp(l - m1)
                    lm[...] = m1
        self.edge += a
        _welford(self.w[0], self.w[1], a[:, :, None] * W, k)
        _welford(self.b[0], self.b[1], b, k)
        return ll

    def state(self, k):
        return dict(edge_prob=self.edge / k, weight_mean=self.w[0].copy(), weight_var=self.w[1] / k, bias_mean=self.b[0].copy(),
                    bias_var=self.b[1] / k)

    def rates(self, i, k, std=False):
        return np.sqrt(self.rate[i][1] / k) if std else self.rate[i][0].copy()

    def pointwise_sums(self, k, var=False):
        out = 0.0
        for lmean, lM2, lm, ls in self.pw:
            V = lM2 / (k - 1) if var else lm + np.log(ls) - np.log(k)
            out = out + V.sum(axis=0)
        return out


class _DeviceAccumulators(object):
    """the same accumulators in the memory of a GibbsEngine's GPU, for the data sets the engine holds now: per data set the Welford (mean, M2)
    of the rates and, pointwise, of the log-likelihood term plus its streaming log-sum-exp (m, s); the edge counts and the moments of a * W
    and b.  Passes the engine's memory gate (reserve) BEFORE anything is allocated: MemoryError otherwise.
    link / link_par: per local neuron, the link code of pgl_summary_fold and its parameter -- required for the rates of the hooks mode,
    where the engine does not know the neurons' models; the built-in modes take theirs from the observation model."""

    @staticmethod
    def bytes(eng, rates=True, pointwise=False):
        """device bytes the accumulators take: (T_i x ldn) doubles per data set x 2 (rates) + 4 (pointwise), and the state's moments"""
        per = 2 * bool(rates) + 4 * bool(pointwise)
        cells = sum(ds.T for ds in eng.datasets) * eng.ldn
        return 8 * per * cells + 8 * (eng.nloc * eng.N + 2 * eng.nloc * eng.D + 2 * eng.nloc) + 4 * eng.nloc * eng.N

    def __init__(self, eng, rates=True, pointwise=False, link=None, link_par=None):
        self.eng, self.dev = eng, eng.dev
        eng.reserve("posterior summary: the accumulators need", self.bytes(eng, rates, pointwise))
        self.link0, self.link_par0, self.link, self.link_par = eng._LINK[eng.obs], float(eng.xi), None, eng.obs_param
        if eng.obs == OBS_HOOKS:
            self.link_par = None
            if rates:
                if link is None:
                    raise ValueError("the rates of the hooks mode need a link code per neuron")
                self.link = torch.from_numpy(np.ascontiguousarray(link, dtype=np.int32).reshape(eng.nloc)).to(eng.dev)
                self.link_par = torch.from_numpy(np.ascontiguousarray(link_par, dtype=np.float64).reshape(eng.nloc)).to(eng.dev)
        self.rate = [(eng._z(ds.T, eng.ldn), eng._z(ds.T, eng.ldn)) for ds in eng.datasets] if rates else None
        self.pw = [tuple(eng._z(ds.T, eng.ldn) for _ in range(4)) for ds in eng.datasets] if pointwise else None
        self.a = eng._z(eng.nloc, eng.N, dtype=I32)
        self.edge = eng._z(eng.nloc, eng.N)
        self.w = (eng._z(eng.nloc, eng.D), eng._z(eng.nloc, eng.D))
        self.b = (eng._z(eng.nloc), eng._z(eng.nloc))

    @_on_device
    def reset(self):
        for t in [self.edge, *self.w, *self.b] + [x for grp in (self.rate or []) + (self.pw or []) for x in grp]:
            t.zero_()

    @_on_device
    def fold(self, eng, a, W, b, k):
        """sample k (1-based) of the state (a, W, b): one upload of the weights, the walk (engine.fold_data) with ONE pgl_summary_fold per
        data set, then pgl_summary_state.  Returns what eng.log_likelihood(a, W, b) returns, to the last bit (the fold forms the
        per-neuron totals as pgl_pg_loglik_ex / pgl_gaussian_stats do).  Gaussian: set_noise first, as for log_likelihood."""
        assert eng is self.eng
        eng._upload_weights(a, W, b)
        self.a.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(a).reshape(eng.nloc, eng.N), dtype=np.int32)))
        none2, none4 = (None, None), (None,) * 4

        def launch(i, ds, st, first):
            r, p = self.rate[i] if self.rate else none2, self.pw[i] if self.pw else none4
            call("pgl_summary_fold", Psi=ptr(ds.Psi), ldn=eng.ldn, bias=ptr(eng.bias), Y=ptr(ds.Y), llpart=ptr(ds.llpart), ll_out=ptr(eng.ll),
                 accumulate=int(not first), T=ds.T, nloc=eng.nloc, obs=eng.obs, xi=eng.xi, param=ptr(eng.obs_param), hooks=ptr(ds.hooks),
                 ldh=eng.ldn, inv_eta=ptr(eng.inv_eta) if eng.obs == OBS_GAUSSIAN else None, rate_mean=ptr(r[0]), rate_M2=ptr(r[1]),
                 link=ptr(self.link), link0=self.link0, link_par=ptr(self.link_par), link_par0=self.link_par0, l_mean=ptr(p[0]), l_M2=ptr(p[1]),
                 lse_m=ptr(p[2]), lse_s=ptr(p[3]), k=int(k), hip_stream=st)
        st = eng.fold_data("summary_fold", launch)
        call("pgl_summary_state", a=ptr(self.a), Wt=ptr(eng.Wt), ldw=eng.ldn, bias=ptr(eng.bias), edge=ptr(self.edge), w_mean=ptr(self.w[0]),
             w_M2=ptr(self.w[1]), b_mean=ptr(self.b[0]), b_M2=ptr(self.b[1]), N=eng.N, B=eng.B, nloc=eng.nloc, k=int(k), hip_stream=st)
        return np.asarray(eng._ll_host(eng.ll), dtype=np.float64).reshape(-1)

    @_on_device
    def state(self, k):
        """-> host dict(edge_prob (nloc, N), weight_mean, weight_var (nloc, N, B), bias_mean, bias_var (nloc,)) after k samples"""
        shp = (self.eng.nloc, self.eng.N, self.eng.B)
        host = lambda t: t.cpu().numpy()           # (the divisions on the host: a count / k there is the correctly rounded quotient)
        return dict(edge_prob=host(self.edge) / k, weight_mean=host(self.w[0]).reshape(shp), weight_var=host(self.w[1]).reshape(shp) / k,
                    bias_mean=host(self.b[0]), bias_var=host(self.b[1]) / k)

    @_on_device
    def rates(self, i, k, std=False):
        """-> host (T_i, nloc): the mean of the rates of data set i over k samples, or their standard deviation (population: M2 / k)"""
        mean, M2 = self.rate[i]
        out = torch.sqrt(M2[:, :self.eng.nloc] / k) if std else mean[:, :self.eng.nloc]
        return out.cpu().numpy()

    @_on_device
    def pointwise_sums(self, k, var=False):
        """-> host (nloc,): per neuron, the sum over all bins of log mean_s exp(l) = m + log s - log k, or (var) of the sample variance
        M2 / (k - 1) of l.  Element-wise in torch; the sums over t through pgl_summary_colsum, in the fixed order of the log-likelihood's
        reduction (torch.sum's order may follow the width of the array)."""
        eng = self.eng
        out = eng._z(eng.nloc)
        st = eng._st()
        for i, ds in enumerate(eng.datasets):
            lmean, lM2, m, sm = self.pw[i]
            V = lM2 / (k - 1) if var else m + torch.log(sm) - float(np.log(k))
            call("pgl_summary_colsum", ptr(V), eng.ldn, ds.T, eng.nloc, ptr(ds.llpart), ptr(out), int(i > 0), st)
            torch.cuda.current_stream(eng.dev).synchronize()        # (V is released below; the launch must have read it)
        return out.cpu().numpy()


class PosteriorSummary(object):
    """running posterior summaries of a model's chain (model.summarize).  collect() folds the model's CURRENT state and returns what
    model.log_likelihood(datas) returns; the read-outs are properties.  Variances are population variances over the folded samples
    (np.var, ddof = 0).  With several ranks every rank accumulates its own neurons; the per-neuron read-outs are collective (one gather
    each, like model.means), lppd() / waic() all-reduce the N per-neuron values once and sum them in neuron order."""

    def __init__(self, model, rates=True, pointwise=False, datas=None, covariates=None):
        self.model, self.rates, self.pointwise = model, bool(rates), bool(pointwise)
        self.obs = model.engine_obs()
        regs = model.regressions[model.n0:model.n1]
        link = link_par = None
        if self.obs == "hooks" and self.rates:
            models = [_regression.builtin_model(r, "mean") for r in regs]
            if None in models:
                j = models.index(None)
                raise ValueError("regression %d (%s) has a mean of its own, which the accumulator cannot form from psi: the rates of the "
                                 "hooks mode need one of the built-in means; summarize(rates=False) works" % (model.n0 + j, type(regs[j]).__name__))
            link = [m.link for m in models]
            link_par = [m.par(r) for m, r in zip(models, regs)]
        self._eng, Ys = model_data(model, datas, "summarize()", covariates)
        Kc = getattr(model, "K", 0)
        self._beta = (np.zeros((model.n1 - model.n0, Kc)), np.zeros((model.n1 - model.n0, Kc)))      # N K numbers per sample: host Welford
        Qc = getattr(model, "Q", 0)                       # latents: ||C_n||^2, the variance of neuron n's common drive (x_t ~ N(0, I)) -- N numbers
        self._common = (np.zeros(model.n1 - model.n0), np.zeros(model.n1 - model.n0)) if Qc else None      # per sample, rotation-invariant
        self._nsets = len(Ys)
        if device_engine(self._eng):
            self._acc = _DeviceAccumulators(self._eng, self.rates, self.pointwise, link, link_par)
        else:
            self._acc = _HostAccumulators(self, Ys)
        self.count = 0
        self.log_likelihoods = []
        self._xi = (np.zeros(model.n1 - model.n0), np.zeros(model.n1 - model.n0))

    def reset(self):
        self._acc.reset()
        self.count = 0
        self.log_likelihoods = []
        self._xi = (np.zeros_like(self._xi[0]), np.zeros_like(self._xi[1]))
        self._beta = (np.zeros_like(self._beta[0]), np.zeros_like(self._beta[1]))
        if self._common is not None:
            self._common = (np.zeros_like(self._common[0]), np.zeros_like(self._common[1]))

    def collect(self):
        """fold the model's current state into the accumulators -> the log-likelihood of the summarised data at that state, equal to
        model.log_likelihood(datas).  One collective (the all-reduce log_likelihood has) with several ranks."""
        m = self.model
        if len(self._eng.datasets) != self._nsets:             # (the accumulators, host or device, are laid out for the data sets of then)
            raise RuntimeError("data was added to the model after summarize(): the accumulators cover %d data sets, the model holds %d "
                               "(build a new summary)" % (self._nsets, len(self._eng.datasets)))
        a, W, b = m._local_state()
        if self.obs == "gaussian":
            self._eng.set_noise([r.eta for r in m.regressions[m.n0:m.n1]])
        elif m._learns_xi():
            m._push_xi(self._eng)
        if getattr(m, "K", 0):
            m._sync_covariates(self._eng)
        ll_loc = self._acc.fold(self._eng, a, W, b, self.count + 1)
        self.count += 1
        if getattr(m, "K", 0):
            _welford(self._beta[0], self._beta[1], m._beta[m.n0:m.n1], float(self.count))
        if self._common is not None:
            _welford(self._common[0], self._common[1], np.sum(m._beta[m.n0:m.n1, m.K_obs:] ** 2, axis=1), float(self.count))
        # the dispersions are a handful of host numbers per sample: their moments stay on the host (NaN for a neuron without xi)
        xi = np.array([getattr(r, "xi", np.nan) for r in m.regressions[m.n0:m.n1]], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            _welford(self._xi[0], self._xi[1], xi, float(self.count))
        ll = float(np.sum(m._all_neurons(ll_loc)))
        self.log_likelihoods.append(ll)
        return ll

    # ---- read-outs
    def _need(self, k=1, pointwise=False, rates=False):
        if pointwise and not self.pointwise:
            raise RuntimeError("this summary keeps no pointwise accumulators: summarize(pointwise=True)")
        if rates and not self.rates:
            raise RuntimeError("this summary keeps no rates: summarize(rates=True)")
        if self.count < k:
            raise RuntimeError("%d sample%s folded so far; this read-out needs at least %d" % (self.count, "" if self.count == 1 else "s", k))

    def _state(self, key):
        self._need()
        return self.model._gather_rows(np.ascontiguousarray(self._acc.state(self.count)[key]))

    edge_prob = property(lambda self: self._state("edge_prob"), doc="(N, N) mean of the adjacency")
    weight_mean = property(lambda self: self._state("weight_mean"), doc="(N, N, B) mean of the effective weights a[:, :, None] * W")
    weight_var = property(lambda self: self._state("weight_var"), doc="(N, N, B) their population variance")
    bias_mean = property(lambda self: self._state("bias_mean"), doc="(N,)")
    bias_var = property(lambda self: self._state("bias_var"), doc="(N,)")

    def _xi_moment(self, i, scale):
        self._need()
        return self.model._gather_rows(np.ascontiguousarray(self._xi[i] * scale))

    xi_mean = property(lambda self: self._xi_moment(0, 1.0), doc="(N,) mean of the negative-binomial xi over the samples; NaN without xi")
    xi_var = property(lambda self: self._xi_moment(1, 1.0 / self.count), doc="(N,) its population variance")

    def _beta_moment(self, i, scale):
        self._need()
        Ko = getattr(self.model, "K_obs", self._beta[i].shape[1])       # (the latents' loadings ride behind: not identifiable one by one)
        return self.model._gather_rows(np.ascontiguousarray(self._beta[i][:, :Ko] * scale))

    def _common_moment(self, i, scale):
        self._need()
        if self._common is None:
            raise RuntimeError("this model has no latents: n_latents=0")
        return self._common[i] * scale

    common_input_var_mean = property(lambda self: self._common_moment(0, 1.0),
                                     doc="(N,) mean over the samples of ||C_n||^2, the variance of neuron n's common drive; models with latents")
    common_input_var_var = property(lambda self: self._common_moment(1, 1.0 / self.count), doc="(N,) its population variance")

    covariate_mean = property(lambda self: self._beta_moment(0, 1.0), doc="(N, K) mean of the covariate weights beta over the samples")
    covariate_var = property(lambda self: self._beta_moment(1, 1.0 / self.count), doc="(N, K) their population variance")

    def _rates(self, std):
        self._need(rates=True)
        return [self.model._gather_rows(np.ascontiguousarray(self._acc.rates(i, self.count, std=std).T)).T for i in range(self._nsets)]

    rate_mean = property(lambda self: self._rates(False), doc="per data set (T_i, N): mean of E[y | X] as model.means defines it")
    rate_std = property(lambda self: self._rates(True), doc="per data set (T_i, N): its population standard deviation")

    def lppd(self):
        """log pointwise predictive density: dict(total, per_neuron), per_neuron[n] = sum_t (logsumexp_s l - log S)"""
        self._need(pointwise=True)
        per = self.model._all_neurons(np.asarray(self._acc.pointwise_sums(self.count), dtype=np.float64))
        return dict(total=float(np.sum(per)), per_neuron=per)

    def waic(self):
        """dict(lppd, p_waic, waic, per_neuron): p_waic = sum over cells of the sample variance (ddof = 1) of l (Gelman et al.'s p_waic2),
        waic = -2 (lppd - p_waic); per_neuron the same per neuron.  Needs two samples."""
        self._need(k=2, pointwise=True)
        loc = np.stack([np.asarray(self._acc.pointwise_sums(self.count), dtype=np.float64),
                        np.asarray(self._acc.pointwise_sums(self.count, var=True), dtype=np.float64)])
        per = self.model._all_neurons(loc)
        lppd, p = float(np.sum(per[0])), float(np.sum(per[1]))
        return dict(lppd=lppd, p_waic=p, waic=-2.0 * (lppd - p), per_neuron=-2.0 * (per[0] - per[1]))
