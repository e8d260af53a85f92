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

A model with an engine_factory has no device accumulators: the same class then folds on the host from engine.psi(...), with the update
formulas of the kernels written in NumPy (_HostAccumulators) -- their specification, and what runs without a GPU.
"""
import numpy as np

from . import regression as _regression


def _welford(mean, M2, x, k):
    """step k (1-based) of the running mean / sum of squared deviations, in place -- the update of the kernels"""
    d = x - mean
    mean += d / k
    M2 += d * (x - mean)


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
    """the same interface on GibbsEngine's device accumulators (engine.summary_alloc / summary_fold)"""

    def __init__(self, summary, eng, link, link_par):
        self.eng = eng
        self.buf = eng.summary_alloc(rates=summary.rates, pointwise=summary.pointwise, link=link, link_par=link_par)

    def reset(self):
        self.eng.summary_reset(self.buf)

    def fold(self, eng, a, W, b, k):
        return np.asarray(eng.summary_fold(self.buf, a, W, b, k), dtype=np.float64).reshape(-1)

    def state(self, k):
        return self.eng.summary_state(self.buf, k)

    def rates(self, i, k, std=False):
        return self.eng.summary_rates(self.buf, i, k, std=std)

    def pointwise_sums(self, k, var=False):
        return self.eng.summary_pointwise(self.buf, k, var=var)


class PosteriorSummary(object):
    """running posterior summaries of a model's chain (model.summarize).  collect() folds the model's CURRENT state and returns what
    model.log_likelihood(datas) returns; the read-outs are properties.  Variances are population variances over the folded samples
    (np.var, ddof = 0).  With several ranks every rank accumulates its own neurons; the per-neuron read-outs are collective (one gather
    each, like model.means), lppd() / waic() all-reduce the N per-neuron values once and sum them in neuron order."""

    def __init__(self, model, rates=True, pointwise=False, datas=None):
        self.model, self.rates, self.pointwise = model, bool(rates), bool(pointwise)
        self.heldout = datas is not None
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
        if self.heldout:
            self._eng = model._heldout_engine(datas)         # held on to: the model's cache keeps one held-out engine only
            Ys = [np.asarray(d[1] if isinstance(d, tuple) else d) for d in datas]
        else:
            self._eng = model.engine
            Ys = [d[1] for d in model.data_list]
        if not Ys:
            raise ValueError("summarize(): the model has no data")
        self._ndata = len(model.data_list)
        self._nsets = len(Ys)
        if hasattr(self._eng, "summary_alloc"):
            self._acc = _DeviceAccumulators(self, self._eng, link, link_par)
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

    def collect(self):
        """fold the model's current state into the accumulators -> the log-likelihood of the summarised data at that state, equal to
        model.log_likelihood(datas).  One collective (the all-reduce log_likelihood has) with several ranks."""
        m = self.model
        if not self.heldout and len(m.data_list) != self._ndata:
            raise RuntimeError("data was added to the model after summarize(): the accumulators cover %d data sets, the model holds %d "
                               "(build a new summary)" % (self._ndata, len(m.data_list)))
        a, W, b = m._local_state()
        if self.obs == "gaussian":
            self._eng.set_noise([r.eta for r in m.regressions[m.n0:m.n1]])
        elif m._learns_xi():
            m._push_xi(self._eng)
        ll_loc = self._acc.fold(self._eng, a, W, b, self.count + 1)
        self.count += 1
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
