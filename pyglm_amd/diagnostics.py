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
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr
from .engine import I32, _on_device
from .summary import _welford, device_engine

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
    """the accumulators in NumPy, for an engine that is no device engine: one BatchMeans per section, the interface of _DeviceDiag"""

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
    """the same accumulators in the memory of a GibbsEngine's GPU: zeroed batch means of `levels` dyadic levels for the sections `what` (a bit
    mask, or names out of SECTIONS) -- the pending / mean / M2 planes, the copies of the state the fold reads (a, and where asked for W, b
    and the conditional edge probabilities p), and the serial number of the sweep p was last formed from.  Passes the engine's memory gate
    (reserve; an engine built with mem_budget_bytes stays inside that figure too) BEFORE anything is allocated: MemoryError otherwise."""

    @staticmethod
    def mask(what):
        """`what` as the bit mask of pgl_diag_fold: an int, or names out of SECTIONS"""
        if isinstance(what, (int, np.integer)):
            mask = int(what)
        else:
            mask = sum(1 << SECTIONS.index(w) for w in set(what))
        if mask < 1 or mask > _lib.PGL_DIAG_ALL:
            raise ValueError("diagnostics: no such sections: %r" % (what,))
        return mask

    @staticmethod
    def section_layout(eng, mask):
        """-> {section: (first entry, entries, shape)} of the sections in `mask`, and the number of entries"""
        nl, N, B = eng.nloc, eng.N, eng.B
        shapes = dict(edge=(nl, N), edge_rb=(nl, N), weight=(nl, N, B), bias=(nl,))
        out, off = {}, 0
        for i, name in enumerate(SECTIONS):
            if mask >> i & 1:
                cnt = int(np.prod(shapes[name]))
                out[name] = (off, cnt, shapes[name])
                off += cnt
        assert off == _lib.load().pgl_diag_entries(N, B, nl, mask)
        return out, off

    @classmethod
    def bytes(cls, eng, levels, what):
        """device bytes the accumulators take: three planes of `levels` doubles per entry (3 * levels * 8 * entries: at N = 1024, B = 5 and 8
        levels 1.4 GB for all four sections), and the copies of the state the fold reads: a, and where asked for W, b and the conditionals p"""
        mask = cls.mask(what)
        lib = _lib.load()
        if not 1 <= int(levels) <= _lib.PGL_DIAG_MAX_LEVELS:
            raise ValueError("diagnostics: levels = %r outside 1 .. %d" % (levels, _lib.PGL_DIAG_MAX_LEVELS))
        state = 4 * eng.nloc * eng.N + 8 * (eng.nloc * eng.N * bool(mask & _lib.PGL_DIAG_EDGE_RB) + eng.nloc * eng.D * bool(mask & _lib.PGL_DIAG_WEIGHT)
                                            + eng.nloc * bool(mask & _lib.PGL_DIAG_BIAS))
        return lib.pgl_diag_bytes(lib.pgl_diag_entries(eng.N, eng.B, eng.nloc, mask), int(levels)) + state

    def __init__(self, eng, levels, what):
        self.eng, self.dev = eng, eng.dev
        eng.reserve("chain diagnostics: the accumulators need", self.bytes(eng, levels, what), cap=eng._mem_budget)
        self.levels, self.what = int(levels), self.mask(what)
        self.layout, self.entries = self.section_layout(eng, self.what)
        self.pending, self.mean, self.M2 = (eng._z(self.levels, self.entries) for _ in range(3))
        self.a = eng._z(eng.nloc, eng.N, dtype=I32)
        self.W = eng._z(eng.nloc, eng.D) if self.what & _lib.PGL_DIAG_WEIGHT else None
        self.b = eng._z(eng.nloc) if self.what & _lib.PGL_DIAG_BIAS else None
        self.p = eng._z(eng.nloc, eng.N) if self.what & _lib.PGL_DIAG_EDGE_RB else None
        self.serial = eng._sweep_serial        # the conditionals of a sweep queued before the allocation are not this chain's

    @_on_device
    def reset(self):
        for t in (self.pending, self.mean, self.M2):
            t.zero_()
        self.serial = self.eng._sweep_serial

    @_on_device
    def fold(self, a, W, b, k):
        """sample k (1-based) of the state (a, W, b): one upload of the state, then pgl_diag_fold.  With edge_rb among the sections,
        pgl_diag_edge_conditional first forms p from the log-odds and the proposal order of the engine's LAST sweep (keep_logodds must
        have been on for it) and the given a: the conditionals belong to a sweep, so one fold per sweep is the rule -- RuntimeError where
        the log-odds are absent or no sweep was queued since the previous fold."""
        eng = self.eng
        st = eng._st()
        rb = bool(self.what & _lib.PGL_DIAG_EDGE_RB)
        if rb:
            if eng.logodds is None:
                raise RuntimeError("diagnostics: the conditional edge probabilities need the last sweep's log-odds, and there are none "
                                   "(engine.keep_logodds must be on before the sweep)")
            if eng._sweep_serial == self.serial:
                raise RuntimeError("diagnostics: no sweep since the previous fold -- the conditional edge probabilities belong to a sweep, "
                                   "one fold per sweep")
        self.a.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(a).reshape(eng.nloc, eng.N), dtype=np.int32)))
        if self.W is not None:
            self.W.copy_(torch.from_numpy(np.ascontiguousarray(W, dtype=np.float64).reshape(eng.nloc, eng.D)))
        if self.b is not None:
            self.b.copy_(torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64).reshape(eng.nloc)))
        if rb:
            call("pgl_diag_edge_conditional", logodds=ptr(eng.logodds), perm=ctypes.c_void_p(eng._din.data_ptr() + eng._perm_off), a=ptr(self.a),
                 p=ptr(self.p), nloc=eng.nloc, N=eng.N, hip_stream=st)
            self.serial = eng._sweep_serial
        h = eng._tic("diag_fold", float(self.entries))
        call("pgl_diag_fold", a=ptr(self.a), W=ptr(self.W), b=ptr(self.b), p=ptr(self.p), pending=ptr(self.pending), mean=ptr(self.mean),
             M2=ptr(self.M2), N=eng.N, B=eng.B, nloc=eng.nloc, levels=self.levels, k=int(k), what=self.what, hip_stream=st)
        eng._toc(h)

    @_on_device
    def read(self, k, section, levels=None):
        """-> host dict(pending, mean, M2) of one section after k samples, each array (number of levels read,) + the section's shape: edge and
        edge_rb (nloc, N), weight (nloc, N, B), bias (nloc,).  levels: the levels to read (default: all) -- a read-out needs two of them,
        and a plane of the weights is 42 MB at N = 1024."""
        lv = list(range(self.levels)) if levels is None else [int(l) for l in levels]
        idx = torch.tensor(lv, dtype=torch.int64, device=self.eng.dev)
        off, cnt, shape = self.layout[section]
        return {key: t[:, off:off + cnt].index_select(0, idx).cpu().numpy().reshape((len(lv),) + shape)
                for key, t in (("pending", self.pending), ("mean", self.mean), ("M2", self.M2))}


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
        if device_engine(eng):
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
