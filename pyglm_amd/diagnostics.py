"""Chain diagnostics: how much chain is there?  Monte Carlo standard errors and effective sample sizes of every edge, effective weight and
bias by dyadic batch means, the multi-chain R-hat, and the Rao-Blackwell estimator of the edge probabilities.

    diag = model.diagnose(levels=8)
    for it in range(n_sweeps):
        model.resample_model()
        if it >= burn:
            diag.collect()
    diag.edge_prob_rb, diag.mcse("edge_rb"), diag.ess("weight"), diag.min_ess(), diag.rb_gain
    rhat([diag, other_chain], "edge")

This module states the definitions once, in NumPy; the kernels (pgl_diag.hip) and the tests are held to them.

Dyadic batch means (BatchMeans, batch_means_host).  x_1 .. x_k are the collected values of one entry and L levels are kept, 1 <= L <= 16;
level l has batch size 2^l.  Batch sums form by binary carry: s_0 = x_k; a level-(l+1) sum is pending_l + s_l -- the earlier half first,
one IEEE addition -- and forms whenever a second level-l sum completes, so sample k touches levels 0 .. min(tz(k), L - 1), tz = trailing
zero bits.  Per level and entry three doubles are kept: `pending`, the first half that awaits its sibling, and (mean, M2) of the level's
completed batch means s_l / 2^l, updated with the Welford step of the posterior summary (summary._welford); its count m_l = k >> l is
derived from k, never stored.  Read-outs after n samples:
    reporting level  l*(n) = min(L - 1, floor(log2(n) / 2)): a batch size of about sqrt(n)
    batch_var(l)     2^l M2_l / (m_l - 1)                    needs m_l >= 2
    mcse             sqrt(batch_var(l*) / (m_l* 2^l*))       the error of the mean over the samples the batches cover
    ess              n (M2_0 / (n - 1)) / batch_var(l*)      NaN where both variances are zero (a constant entry); not capped at n

Conditional edge probabilities (edge_conditional_host).  The sweep proposes every edge once, from its log-odds given everything else; the
average of sigma(log-odds) is the Rao-Blackwell estimator of the edge probability: the expectation of the 0/1 average in stationarity, a
smaller variance.  An edge that was not proposed (rho exactly 0 or 1, deterministic sparsity, a row the sweep did not run) has NaN log-odds
and contributes its current value.

R-hat (rhat).  For C >= 2 chains of equal n, from each chain's level-0 mean and variance (ddof = 1): Wv = mean of the variances, Bv = n x the
variance (ddof = 1) of the means, R-hat = sqrt(((n - 1) / n Wv + Bv / n) / Wv); NaN where Wv = 0.
"""
import numpy as np

from .summary import _welford

MAX_LEVELS = 16                                   # PGL_DIAG_MAX_LEVELS
SECTIONS = ("edge", "edge_rb", "weight", "bias")  # the device sections, in the order of the accumulators' entries (bit i of `what`)


def _check_levels(levels):
    if int(levels) != levels or not 1 <= int(levels) <= MAX_LEVELS:
        raise ValueError("levels = %r: an integer in 1 .. %d is required" % (levels, MAX_LEVELS))
    return int(levels)


def reporting_level(n, levels):
    """l*(n) = min(levels - 1, floor(log2(n) / 2))"""
    if n < 1:
        raise RuntimeError("no sample folded so far")
    return min(int(levels) - 1, (int(n).bit_length() - 1) // 2)


class BatchMeans(object):
    """dyadic batch means of an array of entries (the module's docstring states them).  pending, mean, M2: (levels,) + shape; n: samples
    pushed.  An instance read back from the device may hold only some of the levels (`held`): the read-outs need level 0 and one more."""

    def __init__(self, shape=(), levels=8):
        self.levels = _check_levels(levels)
        self.shape = tuple(int(v) for v in np.atleast_1d(shape))
        self.pending, self.mean_, self.M2 = (np.zeros((self.levels,) + self.shape) for _ in range(3))
        self.held = list(range(self.levels))
        self.n = 0

    @classmethod
    def from_arrays(cls, pending, mean, M2, n, levels, held=None):
        """the accumulators as they stand after n samples; held: the levels the arrays' planes are (default: all of them, in order)"""
        self = cls.__new__(cls)
        self.levels = _check_levels(levels)
        self.pending, self.mean_, self.M2 = (np.asarray(v, dtype=np.float64) for v in (pending, mean, M2))
        self.held = list(range(self.levels)) if held is None else [int(l) for l in held]
        assert self.pending.shape == self.mean_.shape == self.M2.shape and self.M2.shape[0] == len(self.held)
        self.shape = self.M2.shape[1:]
        self.n = int(n)
        return self

    def push(self, x):
        """sample n + 1"""
        assert self.held == list(range(self.levels))
        k = self.n + 1
        tz = (k & -k).bit_length() - 1
        top = min(tz, self.levels - 1)
        s = np.array(np.broadcast_to(np.asarray(x, dtype=np.float64), self.shape))
        for l in range(top + 1):
            _welford(self.mean_[l, ...], self.M2[l, ...], s / float(1 << l), float(k >> l))      # ([l, ...]: a view, for scalars too)
            if l < top:
                s = self.pending[l, ...] + s          # the earlier half first
            elif l == tz:
                self.pending[l, ...] = s
        self.n = k

    # ---- read-outs
    def level(self, n=None):
        return reporting_level(self.n if n is None else n, self.levels)

    def count(self, level):
        """m_l: the completed batches of level l"""
        return self.n >> int(level)

    def _plane(self, level):
        level = int(level)
        if not 0 <= level < self.levels:
            raise ValueError("level %d outside 0 .. %d" % (level, self.levels - 1))
        if level not in self.held:
            raise RuntimeError("level %d was not read back (held: %s)" % (level, self.held))
        return self.held.index(level)

    @property
    def mean(self):
        """the mean of the n samples (level 0)"""
        if self.n < 1:
            raise RuntimeError("no sample folded so far")
        return self.mean_[self._plane(0)].copy()

    def var(self):
        """the sample variance (ddof = 1) of the n samples"""
        return self.batch_var(0)

    def batch_var(self, level):
        """2^l M2_l / (m_l - 1): the variance of a single sample that the spread of the level's batch means implies"""
        m = self.count(level)
        if m < 2:
            raise RuntimeError("level %d holds %d completed batch%s after %d sample%s; this read-out needs at least 2"
                               % (level, m, "" if m == 1 else "es", self.n, "" if self.n == 1 else "s"))
        return float(1 << int(level)) * self.M2[self._plane(level)] / (m - 1)

    def mcse(self, level=None):
        l = self.level() if level is None else int(level)
        bv = self.batch_var(l)
        return np.sqrt(bv / float(self.count(l) << l))

    def ess(self, level=None):
        l = self.level() if level is None else int(level)
        bv, v0 = self.batch_var(l), self.batch_var(0)
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.n * v0 / bv


def batch_means_host(x, levels):
    """BatchMeans of the samples stacked along the first axis of x"""
    x = np.asarray(x, dtype=np.float64)
    bm = BatchMeans(x.shape[1:], levels)
    for row in x:
        bm.push(row)
    return bm


def edge_conditional_host(logodds, perm, a):
    """p (n, N): the conditional edge probabilities of one sweep.  p[n][m] = 1.0 if a[n][m] else 0.0; then for every proposal step kk whose
    logodds[n][kk] is not NaN, p[n][perm[n][kk]] = 1 / (1 + exp(-logodds[n][kk])).  A step whose perm[n][kk] lies outside [0, N) is skipped,
    never stored through."""
    logodds, perm, a = np.asarray(logodds, dtype=np.float64), np.asarray(perm), np.asarray(a)
    nl, N = a.shape
    p = np.where(a != 0, 1.0, 0.0)
    with np.errstate(over="ignore"):
        for n in range(nl):
            for kk in range(N):
                lo, m = logodds[n, kk], int(perm[n, kk])
                if lo == lo and 0 <= m < N:
                    p[n, m] = 1.0 / (1.0 + np.exp(-lo))
    return p


def rhat(chains, what=None):
    """the potential scale reduction of C >= 2 chains of equal length, per entry: ChainDiagnostics objects (what: one of their read-outs,
    "edge", "edge_rb", "weight", "bias", "ll", "xi") or BatchMeans objects.  NaN where the within-chain variance is zero."""
    bms = [c if isinstance(c, BatchMeans) else c._bm(what, (0,)) for c in chains]
    if len(bms) < 2:
        raise ValueError("rhat: at least two chains")
    n = bms[0].n
    if any(b.n != n for b in bms):
        raise ValueError("rhat: chains of different lengths: %s" % [b.n for b in bms])
    means, variances = np.stack([b.mean for b in bms]), np.stack([b.var() for b in bms])
    Wv = variances.mean(axis=0)
    Bv = n * means.var(axis=0, ddof=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.sqrt(((n - 1.0) / n * Wv + Bv / n) / Wv)
    return np.where(Wv == 0, np.nan, out)


class _HostDiag(object):
    """the accumulators in NumPy, for an engine without diag_alloc: one BatchMeans per section, the interface of _DeviceDiag"""

    def __init__(self, model, levels, sections):
        nl, N, B = model.n1 - model.n0, model.N, model.B
        shapes = dict(edge=(nl, N), weight=(nl, N, B), bias=(nl,))
        self.levels, self.shapes = levels, {s: shapes[s] for s in sections}
        self.reset()

    def reset(self):
        self.bm = {s: BatchMeans(shape, self.levels) for s, shape in self.shapes.items()}

    def fold(self, a, W, b, k):
        a = np.asarray(a) != 0
        values = dict(edge=np.where(a, 1.0, 0.0), weight=np.where(a[:, :, None], np.asarray(W, dtype=np.float64), 0.0),
                      bias=np.asarray(b, dtype=np.float64).reshape(-1))
        for s, bm in self.bm.items():
            assert bm.n == k - 1
            bm.push(values[s])

    def read(self, k, section, levels):
        bm = self.bm[section]
        return {key: v[list(levels)] for key, v in (("pending", bm.pending), ("mean", bm.mean_), ("M2", bm.M2))}


class _DeviceDiag(object):
    """the same interface on GibbsEngine's device accumulators (engine.diag_alloc / diag_fold / diag_read)"""

    def __init__(self, eng, levels, sections):
        self.eng = eng
        self.buf = eng.diag_alloc(levels, sections)

    def reset(self):
        self.eng.diag_reset(self.buf)

    def fold(self, a, W, b, k):
        self.eng.diag_fold(self.buf, a, W, b, k)

    def read(self, k, section, levels):
        return self.eng.diag_read(self.buf, k, sections=(section,), levels=levels)[section]


class ChainDiagnostics(object):
    """running diagnostics of a model's chain (model.diagnose).  collect() folds the model's CURRENT state, once per kept sweep, after
    resample_model(); the read-outs name a section: "edge" (the 0/1 adjacency), "edge_rb" (the conditional edge probabilities of the sweep),
    "weight" (the effective weights a * W), "bias", and the host traces "ll" (the log-likelihood) and "xi" (the negative-binomial
    dispersions; NaN for a neuron without one).  With several ranks every rank accumulates its own neurons; the per-neuron read-outs are
    collective (one gather each, like PosteriorSummary's)."""

    def __init__(self, model, levels=8, weights=True, rb=True):
        self.model, self.levels = model, _check_levels(levels)
        eng = model.engine
        sections = ["edge"] + (["edge_rb"] if rb else []) + (["weight"] if weights else []) + ["bias"]
        if hasattr(eng, "diag_alloc"):
            self._acc = _DeviceDiag(eng, self.levels, sections)
            if rb:
                eng.keep_logodds = True               # the sweeps from now on leave their log-odds (they are bit-equal either way)
        else:
            if rb:
                raise ValueError("diagnose(rb=True): the conditional edge probabilities come from the device sweep's log-odds, which %s does "
                                 "not keep; diagnose(rb=False) works" % type(eng).__name__)
            self._acc = _HostDiag(model, self.levels, sections)
        self.sections = tuple(sections)
        self._nloc = model.n1 - model.n0
        self.reset(_acc=False)

    def reset(self, _acc=True):
        if _acc:
            self._acc.reset()
        self.count = 0
        self._ll = BatchMeans((), self.levels)
        self._xi = BatchMeans((self._nloc,), self.levels)

    def collect(self, ll=None):
        """fold the model's current state -> the log-likelihood that joined the trace: `ll` where given (a caller that has it already, from
        PosteriorSummary.collect() for one), else model.log_likelihood()"""
        m = self.model
        a, W, b = m._local_state()
        self._acc.fold(a, W, b, self.count + 1)
        self.count += 1
        ll = float(m.log_likelihood() if ll is None else ll)
        self._ll.push(ll)
        with np.errstate(invalid="ignore"):
            self._xi.push(np.array([getattr(r, "xi", np.nan) for r in m.regressions[m.n0:m.n1]], dtype=np.float64))
        return ll

    # ---- read-outs
    def level(self, n=None):
        """the reporting level after n samples (default: those collected)"""
        return reporting_level(self.count if n is None else n, self.levels)

    def _bm(self, what, levels):
        """BatchMeans of read-out `what` over ALL neurons, holding the given levels"""
        if what == "ll":
            return self._ll
        if self.count < 1:
            raise RuntimeError("no sample folded so far")
        gather = self.model._gather_rows
        if what == "xi":
            src = self._xi
            parts = {key: v for key, v in (("pending", src.pending), ("mean", src.mean_), ("M2", src.M2))}
            levels = src.held
        elif what in self.sections:
            levels = sorted(set(int(l) for l in levels))
            parts = self._acc.read(self.count, what, levels)
        else:
            raise ValueError("no read-out %r: one of %s" % (what, list(self.sections) + ["ll", "xi"]))
        # rows = neurons: (3, levels, nloc, ...) -> (nloc, 3, levels, ...) for the gather, and back
        stack = np.stack([parts["pending"], parts["mean"], parts["M2"]])
        full = np.moveaxis(gather(np.ascontiguousarray(np.moveaxis(stack, 2, 0))), 0, 2)
        return BatchMeans.from_arrays(full[0], full[1], full[2], self.count, self.levels, held=levels)

    def mean(self, what):
        """the mean over the collected samples.  "edge": a mean of 0/1 values is a count over n -- n x the running mean is rounded to the
        nearest integer and divided by n, the correctly rounded quotient PosteriorSummary.edge_prob is"""
        out = self._bm(what, (0,)).mean
        if what == "edge":
            out = np.rint(out * self.count) / self.count
        return out if np.ndim(out) else float(out)

    def _levels_for(self, level):
        l = self.level() if level is None else int(level)
        if not 0 <= l < self.levels:
            raise ValueError("level %d outside 0 .. %d" % (l, self.levels - 1))
        return l

    def mcse(self, what, level=None):
        l = self._levels_for(level)
        return self._bm(what, (0, l)).mcse(l)

    def ess(self, what, level=None):
        l = self._levels_for(level)
        return self._bm(what, (0, l)).ess(l)

    def min_ess(self):
        """{read-out: (smallest ESS, its index)} over the sections, "ll" and (where a neuron has one) "xi"; entries whose ESS is NaN (constant
        ones) are passed over, and a read-out with no other entry gives (nan, None)"""
        out = {}
        for what in self.sections + ("ll", "xi"):
            e = np.asarray(self.ess(what), dtype=np.float64)
            if what == "xi" and np.all(np.isnan(e)):
                continue
            if np.all(np.isnan(e)):
                out[what] = (float("nan"), None)
            else:
                i = int(np.nanargmin(e))
                out[what] = (float(e.reshape(-1)[i]), tuple(int(j) for j in np.unravel_index(i, e.shape)))
        return out

    edge_prob = property(lambda self: self.mean("edge"), doc="(N, N) mean of the adjacency: PosteriorSummary.edge_prob")
    edge_prob_rb = property(lambda self: self.mean("edge_rb"), doc="(N, N) mean of the conditional edge probabilities (Rao-Blackwell)")

    @property
    def rb_gain(self):
        """(N, N): (mcse("edge") / mcse("edge_rb"))^2 -- how many plain samples one Rao-Blackwell sample is worth; NaN where both are zero"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return (self.mcse("edge") / self.mcse("edge_rb")) ** 2
