"""Time-rescaling goodness of fit of the recorded data under the posterior (Brown et al. 2002; for binned data Haslinger, Pipa & Brown 2010).

Under the model the intensity of a neuron integrated between two consecutive events is Exp(1).  In discrete time the intensity of bin t is
q[t] = -log P(y[t] = 0 | psi[t]) = par * log1p(exp(psi[t])) -- par = 1 (Bernoulli), xi (negative binomial), n (binomial): all three are
(1 - sigma(psi))^par --, and the position of the event inside its own bin is drawn from the exponential law cut at q[e], which removes the
bias of the binning.  So for consecutive events at bins s < e

    xi = sum_{s < t < e} q[t] + delta,    delta = -log1p(-r (-expm1(-q[e]))),    z = -expm1(-xi)

is uniform on [0, 1), and a Kolmogorov-Smirnov statistic of the z of a neuron says whether the model describes it.  Unlike the posterior
predictive checks of simulate.py the test needs no simulated replicates: it reads the data against the fitted rates, held-out data too.

    gof = model.time_rescaling(bins=64)
    for it in range(n_sweeps):
        model.resample_model()
        if it >= burn:
            gof.collect()
    gof.ks_mean, gof.band, gof.exceed_fraction, gof.failing()

rescale_host and ks_binned are THE DEFINITION of what pgl_rescale_fold / pgl_rescale_ks (csrc/pgl_rescale.hip) compute on the device; a model
with an engine_factory folds through them on the host from engine.psi(...).
"""
import numpy as np
import torch

from . import _lib
from . import simulate as _sim
from ._lib import call, ptr
from .engine import I32, _on_device
from .summary import _welford, device_engine, model_data

PURPOSE_RESCALE = 3
PGL_RESCALE_MAX_BINS = _lib.PGL_RESCALE_MAX_BINS    # bins of the histogram of z at most
_M32 = 0xFFFFFFFF


def check_bins(bins):
    """D = int(bins) of the histogram of z, 2 <= D <= PGL_RESCALE_MAX_BINS, else ValueError"""
    D = int(bins)
    if not 2 <= D <= PGL_RESCALE_MAX_BINS:
        raise ValueError("bins = %d: 2 <= bins <= PGL_RESCALE_MAX_BINS = %d is required" % (D, PGL_RESCALE_MAX_BINS))
    return D


def interval_par(regressions):
    """(N,) the factor of log1p(exp(psi)) in -log P(y = 0 | psi) per neuron, from its own observation model (simulate.observation_models):
    1 Bernoulli, xi negative binomial, n binomial; ValueError for a Gaussian neuron, which has no events"""
    models = _sim.observation_models(regressions)
    bad = _sim.first_without_events(models)
    if bad is not None:
        raise ValueError("time rescaling: neuron %d is Gaussian; a rescaled interval needs events, which a Gaussian neuron does not have" % bad)
    return np.array([m.par(r) for m, r in zip(models, regressions)], dtype=np.float64)


def event_uniforms(seed, draw, stream, elems):
    """the first uniform of Philox call `draw` of purpose PURPOSE_RESCALE of `stream` at the elements `elems`: words 0 and 1 of
    simulate.philox_words(seed, 3, draw, ., stream, .) through simulate._unit"""
    elems = np.asarray(elems, dtype=np.uint64) & np.uint64(_M32)
    w = _sim.philox4x32_10((int(draw) & 0xFFFFFF) | (PURPOSE_RESCALE << 24), elems, int(stream) & _M32, (int(stream) >> 32) & _M32, seed)
    return _sim._unit(w[0], w[1])


def rescale_host(psi, Y, par, D, seed, draw, neuron0, elem0):
    """THE DEFINITION.  psi, Y (T, N): the activation (bias added) and the observations of one data set, column j being global neuron
    neuron0 + j; par a scalar or (N,); elem0 the data set's offset in the stream (the bins of the data sets in front of it).
    -> (hist (N, D) int64, zsum (N, 2) = (sum z, sum z^2), [z of column j in time order]).  An event is a bin with Y > 0 (NaN and negative
    values are none); the stretch before a column's first event and the one after its last are dropped."""
    psi, Y = np.asarray(psi, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    D = check_bins(D)
    if psi.ndim != 2 or psi.shape != Y.shape:
        raise ValueError("rescale_host(): psi and Y (T, N) of one shape are required")
    T, N = psi.shape
    par = np.broadcast_to(np.asarray(par, dtype=np.float64), (N,))
    hist, zsum, zs = np.zeros((N, D), dtype=np.int64), np.zeros((N, 2)), []
    with np.errstate(over="ignore", invalid="ignore"):
        q = par[None, :] * np.log1p(np.exp(psi))
        for j in range(N):
            ev = np.flatnonzero(Y[:, j] > 0)
            if ev.size < 2:
                zs.append(np.zeros(0))
                continue
            s, e = ev[:-1] + 1, ev[1:]
            between = np.add.reduceat(q[:, j], np.column_stack([s, e]).ravel())[::2]     # sum of q[s:e]; an empty slice gives q[s]
            between = np.where(s < e, between, 0.0)
            r = event_uniforms(seed, draw, int(neuron0) + j, int(elem0) + e)
            xi = between + -np.log1p(-r * (-np.expm1(-q[e, j])))
            z = -np.expm1(-xi)
            b = np.where(np.isnan(z), 0.0, z * D).astype(np.int64)
            hist[j] = np.bincount(np.clip(b, 0, D - 1), minlength=D)
            zsum[j] = z.sum(), (z * z).sum()
            zs.append(z)
    return hist, zsum, zs


def ks_binned(hist):
    """the Kolmogorov-Smirnov distance of a histogram of z (..., D) from the uniform law, at the D - 1 interior edges: with C_d the count of
    bins 0 .. d - 1 and M the total, max_d |C_d D - d M| / (M D) -- the numerator in 64-bit integers, then ONE division: device and host
    agree to the last bit on equal histograms.  NaN where M = 0"""
    hist = np.asarray(hist, dtype=np.int64)
    D = hist.shape[-1]
    M = hist.sum(axis=-1)
    C = np.cumsum(hist, axis=-1)[..., :-1]
    num = np.abs(C * D - np.arange(1, D, dtype=np.int64) * M[..., None]).max(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(M > 0, num.astype(np.float64) / (M * D).astype(np.float64), np.nan)


def band(coef, M):
    """coef / sqrt(M): the large-sample KS band (coef = 1.36: 95 %, 1.63: 99 %); inf where M = 0"""
    with np.errstate(divide="ignore"):
        return float(coef) / np.sqrt(np.asarray(M, dtype=np.float64))


class _HostFold(object):
    """the accumulators and the per-sample fold in NumPy, for an engine without device accumulators: what pgl_rescale_fold and
    pgl_rescale_ks do, through rescale_host and ks_binned"""

    def __init__(self, gof, Ys):
        m = gof.model
        self.g = gof
        self.Y = [np.asarray(Y, dtype=np.float64)[:, m.n0:m.n1] for Y in Ys]
        self.elem0 = np.concatenate(([0], np.cumsum([Y.shape[0] for Y in self.Y])))[:-1]
        self.reset()

    def reset(self):
        nl, D = self.g.model.n1 - self.g.model.n0, self.g.D
        self.s = dict(hist=np.zeros((nl, D), dtype=np.int64), zsum=np.zeros((nl, 2)), ks=np.full(nl, np.nan), ks_mean=np.zeros(nl),
                      ks_M2=np.zeros(nl), exceed=np.zeros(nl, dtype=np.int64), hist_sum=np.zeros((nl, D), dtype=np.int64))

    def fold(self, eng, a, W, b, k):
        g, m, s = self.g, self.g.model, self.s
        s["hist"][...], s["zsum"][...] = 0, 0.0
        for i, Y in enumerate(self.Y):
            psi = np.asarray(eng.psi(a, W, b, i), dtype=np.float64)
            h, zs, _ = rescale_host(psi, Y, g.par, g.D, g.seed, k - 1, m.n0, self.elem0[i])
            s["hist"] += h
            s["zsum"] += zs
        s["ks"] = ks_binned(s["hist"])
        with np.errstate(invalid="ignore"):
            _welford(s["ks_mean"], s["ks_M2"], s["ks"], float(k))
            s["exceed"] += s["ks"] > band(g.coef, s["hist"].sum(axis=1))
        s["hist_sum"] += s["hist"]

    def set_par(self, par):
        pass                                                  # (fold reads the test's par at every sample)

    def read(self):
        return self.s


class _DeviceFold(object):
    """the same accumulators in the memory of a GibbsEngine's GPU, for the data sets the engine holds now: hist / zsum / ks of the last sample,
    the running ks_mean, ks_M2, exceed, hist_sum, and the fold's scratch.  par: per local neuron (or a scalar) the factor of
    log1p(exp(psi)) in -log P(y = 0 | psi), taken from the caller, not from the engine's observation model, so the hooks mode works.
    coef: the band is coef / sqrt(M).  Passes the engine's memory gate (reserve) BEFORE anything is allocated: MemoryError otherwise."""

    @staticmethod
    def bytes(eng, bins):
        """device bytes the accumulators take: the segments' records of the longest data set, and per neuron the two histograms,
        (sum z, sum z^2), the KS statistic with its moments, and the count of exceedances"""
        T = max([ds.T for ds in eng.datasets] or [0])
        return _lib.load().pgl_rescale_work_bytes(eng.nloc, T) + eng.nloc * (12 * int(bins) + 16 + 24 + 4 + 8)

    def __init__(self, eng, bins, par, coef=1.36, seed=0):
        self.eng, self.dev = eng, eng.dev
        self.D, self.coef, self.seed = int(bins), float(coef), int(seed)
        eng.reserve("time rescaling: the accumulators need", self.bytes(eng, self.D))
        self.qpar = None
        self.set_par(par)
        nl, z = eng.nloc, eng._z
        self.hist = z(nl, self.D, dtype=I32)
        self.hist_sum = z(nl, self.D, dtype=torch.int64)
        self.zsum = z(nl, 2)
        self.ks, self.ks_mean, self.ks_M2 = z(nl), z(nl), z(nl)
        self.exceed = z(nl, dtype=I32)
        T = max([ds.T for ds in eng.datasets] or [0])
        self.work = torch.empty(_lib.load().pgl_rescale_work_bytes(nl, T), dtype=torch.uint8, device=eng.dev)

    @_on_device
    def reset(self):
        for t in (self.hist, self.hist_sum, self.zsum, self.ks, self.ks_mean, self.ks_M2, self.exceed):
            t.zero_()

    @_on_device
    def set_par(self, par):
        """replace the factor of log1p(exp(psi)) (a model that learns xi: the factor moves with the chain)"""
        par = np.broadcast_to(np.asarray(par, dtype=np.float64).reshape(-1), (self.eng.nloc,))
        self.qpar0 = float(par[0])
        if self.qpar is not None:
            self.qpar.copy_(torch.from_numpy(np.array(par)))
        elif np.any(par != par[0]):
            self.qpar = torch.from_numpy(np.array(par)).to(self.eng.dev)

    @_on_device
    def fold(self, eng, a, W, b, k, only=None):
        """sample k (1-based) of the state (a, W, b): one upload of the weights, the walk (engine.fold_data) with ONE pgl_rescale_fold per
        data set (Philox call k - 1 of the seed; the data sets behind the first add to the sample's histogram), then pgl_rescale_ks.
        only = i: data set i alone."""
        assert eng is self.eng
        eng._upload_weights(a, W, b)
        st = eng.fold_data("rescale_fold", lambda i, ds, st, first: call(
            "pgl_rescale_fold", Psi=ptr(ds.Psi), ldn=eng.ldn, bias=ptr(eng.bias), Y=ptr(ds.Y), T=ds.T, nloc=eng.nloc, qpar=ptr(self.qpar),
            qpar0=self.qpar0, D=self.D, seed=self.seed & (2 ** 64 - 1), draw=(int(k) - 1) & 0xFFFFFFFF, neuron0=eng.n0, elem0=ds.elem0,
            hist=ptr(self.hist), zsum=ptr(self.zsum), accumulate=int(not first), work=ptr(self.work), hip_stream=st), only=only)
        call("pgl_rescale_ks", hist=ptr(self.hist), nloc=eng.nloc, D=self.D, coef=self.coef, ks=ptr(self.ks), ks_mean=ptr(self.ks_mean),
             ks_M2=ptr(self.ks_M2), exceed=ptr(self.exceed), hist_sum=ptr(self.hist_sum), k=int(k), hip_stream=st)

    @_on_device
    def read(self):
        """-> host dict: hist (nloc, D) and zsum (nloc, 2) of the last sample, ks of it, ks_mean, ks_M2, exceed over the samples, hist_sum"""
        host = lambda t: t.cpu().numpy()
        return dict(hist=host(self.hist).astype(np.int64), zsum=host(self.zsum), ks=host(self.ks), ks_mean=host(self.ks_mean),
                    ks_M2=host(self.ks_M2), exceed=host(self.exceed).astype(np.int64), hist_sum=host(self.hist_sum))


class TimeRescaling(object):
    """the time-rescaling test of a model's data under its chain (model.time_rescaling).  collect() folds the model's CURRENT state: sample k
    (1-based) uses Philox call k - 1 for the positions of the events inside their bins, so no two samples share a uniform.  Every data set
    of the model (or of datas=, held-out recordings) adds its intervals; none crosses data sets.  With several ranks every rank folds its own
    neurons; the read-outs are collective (one gather each, as PosteriorSummary's).  host=True folds in NumPy from engine.psi(...) whatever
    the engine -- what a model with an engine_factory always does."""

    def __init__(self, model, bins=64, seed=0, coef=1.36, datas=None, host=False, covariates=None):
        self.model, self.D, self.seed, self.coef = model, check_bins(bins), int(seed), float(coef)
        self.par = interval_par(model.regressions)[model.n0:model.n1]
        self._eng, Ys = model_data(model, datas, "time_rescaling()", covariates)
        self._nsets = len(Ys)
        if device_engine(self._eng) and not host:
            self._acc = _DeviceFold(self._eng, self.D, self.par, self.coef, self.seed)
        else:
            self._acc = _HostFold(self, Ys)
        self.count = 0

    def reset(self):
        self._acc.reset()
        self.count = 0

    def collect(self):
        """fold the model's current state: one histogram of z per neuron, its KS statistic into the running moments"""
        m = self.model
        if len(self._eng.datasets) != self._nsets:             # (the accumulators, host or device, are laid out for the data sets of then)
            raise RuntimeError("data was added to the model after time_rescaling(): the test covers %d data sets, the model holds %d "
                               "(build a new one)" % (self._nsets, len(self._eng.datasets)))
        if m._learns_xi():
            # the factor of log1p(exp(psi)) is the CURRENT xi: read again at every sample, and the device copy with it (a fixed xi keeps
            # the single read of the constructor)
            self.par = interval_par(m.regressions)[m.n0:m.n1]
            self._acc.set_par(self.par)
        a, W, b = m._local_state()
        if getattr(m, "K", 0):
            m._sync_covariates(self._eng)
        self._acc.fold(self._eng, a, W, b, self.count + 1)
        self.count += 1

    # ---- read-outs
    def _read(self, key):
        if self.count < 1:
            raise RuntimeError("no sample folded so far: call collect() first")
        return self.model._gather_rows(np.ascontiguousarray(self._acc.read()[key]))

    intervals = property(lambda self: self._read("hist").sum(axis=1), doc="(N,) M: rescaled intervals per neuron (the same in every sample)")
    hist = property(lambda self: self._read("hist_sum"), doc="(N, D) histogram of z, summed over the samples")
    hist_last = property(lambda self: self._read("hist"), doc="(N, D) histogram of z of the last sample")
    zsum_last = property(lambda self: self._read("zsum"), doc="(N, 2) (sum z, sum z^2) of the last sample")
    ks_last = property(lambda self: self._read("ks"), doc="(N,) binned KS statistic of the last sample; NaN without an interval")
    ks_mean = property(lambda self: self._read("ks_mean"), doc="(N,) its mean over the samples")
    ks_std = property(lambda self: np.sqrt(self._read("ks_M2") / self.count), doc="(N,) its population standard deviation")
    exceed_fraction = property(lambda self: self._read("exceed") / float(self.count), doc="(N,) share of the samples with ks > band")
    band = property(lambda self: band(self.coef, self.intervals), doc="(N,) coef / sqrt(M)")

    def failing(self, threshold=0.5):
        """the neurons the model does not describe: those whose KS statistic left the band in more than `threshold` of the samples"""
        return np.flatnonzero(self.exceed_fraction > threshold)
