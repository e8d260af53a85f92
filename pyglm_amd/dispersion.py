"""Learning the negative-binomial dispersion xi: the CRT (Chinese restaurant table) augmentation of Zhou & Carin (2015).

With y ~ NB(xi, sigma(psi)) and xi ~ Gamma(e0, rate f0), the table counts

    L_t | y_t, xi = sum_{i = 0 .. y_t - 1} Bernoulli(xi / (xi + i))

make the conditional of xi conjugate:

    xi | L, psi ~ Gamma(e0 + sum_t L_t, rate f0 + sum_t log(1 + e^psi_t)).

omega is redrawn from the new xi at the start of the next sweep, so (xi, omega) are updated as a block given the weights and the chain's
target is the joint posterior.  A regression with xi_prior=(e0, f0) takes the step after every sweep (regression.py, models.py).

dispersion_host is THE DEFINITION of what pgl_dispersion_fold (csrc/pgl_dispersion.hip) computes on the device (_DeviceStep); a model with
an engine_factory folds through it on the host from engine.psi(...) (_HostStep).
"""
import numpy as np
import torch

from . import _lib, simulate as _sim
from ._lib import call, ptr
from .engine import _StepScratch, _on_device, make_gamma_draws

PURPOSE_DISPERSION = _lib.PGL_PURPOSE_DISPERSION          # 4
MAX_COUNT = _lib.PGL_DISPERSION_MAX_COUNT                 # a larger count is taken as this one: call j of a cell's stream sits in 24 bits
COOP_COUNT = _lib.PGL_DISPERSION_COOP                     # the device finishes a larger cell with a whole wave (the result is the same)
ROWS = _lib.PGL_DISPERSION_ROWS                           # rows of time one workgroup of the device fold owns
XI_LANE = 2                                               # counter lane of the gamma variate of xi (make_gamma_draws; eta's is lane 1)
_M32 = 0xFFFFFFFF
_CHUNK = 1 << 21                                          # Philox calls evaluated together


def cell_counts(Y):
    """m of every cell: floor(y) for y >= 1 (at most MAX_COUNT), otherwise 0 -- NaN and negative values count as none -> int64"""
    Y = np.asarray(Y, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(Y >= 1.0, np.minimum(np.floor(np.where(Y >= 1.0, Y, 0.0)), float(MAX_COUNT)), 0.0).astype(np.int64)


def table_uniforms(seed, sweep, neuron, elems, calls):
    """(u_{2j}, u_{2j+1}) of call j = `calls` of the streams of the cells at elements `elems` of global neuron `neuron`: purpose
    PURPOSE_DISPERSION, key = seed, stream = (sweep << 32) | neuron -- words 0, 1 and words 2, 3 through simulate._unit"""
    stream = ((int(sweep) & _M32) << 32) | (int(neuron) & _M32)
    elems = np.asarray(elems, dtype=np.uint64) & np.uint64(_M32)
    c0 = (np.asarray(calls, dtype=np.uint64) & np.uint64(0xFFFFFF)) | np.uint64(PURPOSE_DISPERSION << 24)
    w = _sim.philox4x32_10(c0, elems, stream & _M32, (stream >> 32) & _M32, seed)
    return _sim._unit(w[0], w[1]), _sim._unit(w[2], w[3])


def softplus(x):
    """log(1 + e^x) as max(x, 0) + log1p(exp(-|x|)): the form of pgl_generate.hip, which does not overflow"""
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def dispersion_host(psi, Y, xi, seed, sweep, neuron0, elem0):
    """THE DEFINITION.  psi, Y (T, N): the activation (bias added) and the observations of one data set, column j being global neuron
    neuron0 + j; xi a scalar or (N,); elem0 the data set's offset in the stream (the bins of the data sets in front of it).
    -> (L (N,) int64, S (N,) float64).
    Count of a cell: m = floor(y) for y >= 1, otherwise 0 (cell_counts).  Table count of a cell:
        l = 1[m >= 1] + sum_{i = 1 .. m - 1} 1[ u_{i-1} * (xi + i) < xi ]
    -- the first trial has probability 1 and draws nothing, so a column of zeros and ones makes no Philox call --, with u_k the k-th uniform
    of the cell's own stream (table_uniforms; element = elem0 + t): trial i is addressed by its index.  L = sum_t l, exact;
    S = sum_t softplus(psi)."""
    psi, Y = np.asarray(psi, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    if psi.ndim != 2 or psi.shape != Y.shape:
        raise ValueError("dispersion_host(): psi and Y (T, N) of one shape are required")
    T, N = psi.shape
    xi = np.broadcast_to(np.asarray(xi, dtype=np.float64), (N,))
    M = cell_counts(Y)
    L = (M >= 1).sum(axis=0).astype(np.int64)
    for j in range(N):
        rows = np.flatnonzero(M[:, j] >= 2)
        m = M[rows, j]
        ncalls = m // 2                                            # trials 1 .. m - 1 are uniforms 0 .. m - 2: calls 0 .. (m - 2) // 2
        ends = np.cumsum(ncalls)
        lo = 0
        while lo < rows.size:                                      # the column's calls, a chunk of whole cells at a time
            hi = max(lo + 1, int(np.searchsorted(ends, (ends[lo - 1] if lo else 0) + _CHUNK, side="right")))
            nc = ncalls[lo:hi]
            cell = np.repeat(np.arange(lo, hi), nc)
            call = np.arange(int(nc.sum()), dtype=np.int64) - np.repeat(np.cumsum(nc) - nc, nc)
            u0, u1 = table_uniforms(seed, sweep, int(neuron0) + j, int(elem0) + rows[cell], call)
            i0 = 2 * call + 1
            x = xi[j]
            L[j] += int(np.count_nonzero(u0 * (x + i0) < x)) + int(np.count_nonzero((i0 + 1 < m[cell]) & (u1 * (x + (i0 + 1)) < x)))
            lo = hi
    with np.errstate(over="ignore", invalid="ignore"):
        sp = softplus(psi)
        S = np.array([np.ascontiguousarray(sp[:, j]).sum() for j in range(N)], dtype=np.float64)     # column by column: the same whatever N
    return L, S


class _HostStep(object):
    """the statistics of xi | y, psi where the engine is no device engine: dispersion_host of engine.psi(...) and the model's data and xi"""

    def __init__(self, eng, model):
        self.eng, self.model = eng, model

    def stats(self, a, W, b, seed, sweep):
        m, nl, elem0 = self.model, self.model.n1 - self.model.n0, 0
        xi, L, S = np.array([r.xi for r in m.regressions[m.n0:m.n1]], dtype=np.float64), np.zeros(nl, dtype=np.int64), np.zeros(nl)
        for i, (_, Y) in enumerate(m.data_list):
            Yl = np.asarray(Y, dtype=np.float64)[:, m.n0:m.n1]
            Li, Si = dispersion_host(np.asarray(self.eng.psi(a, W, b, i), dtype=np.float64), Yl, xi, seed, sweep, m.n0, elem0)
            L, S, elem0 = L + Li, S + Si, elem0 + Yl.shape[0]
        return L, S


class _DeviceStep(_StepScratch):
    """the same on a GibbsEngine's GPU, with its scratch: the workgroups' partials of the longest data set, L and S (engine._StepScratch)"""

    def _alloc(self, T, eng):
        need = _lib.load().pgl_dispersion_work_bytes(eng.nloc, T)
        eng.reserve("dispersion: the scratch needs", need + 16 * eng.nloc)
        return dict(work=torch.empty(need, dtype=torch.uint8, device=eng.dev), L=eng._z(eng.nloc, dtype=torch.int64), S=eng._z(eng.nloc))

    @_on_device
    def stats(self, a, W, b, seed, sweep):
        """at the state (a, W, b) -> (L int64, S float64), host arrays (nloc,): the CRT table counts under the engine's CURRENT per-neuron
        xi (set_obs_param) and sum_t log(1 + e^psi_t), over every data set (the first fold, accumulate = 0, overwrites both)"""
        eng = self.eng
        if eng.obs != eng.OBS["negbin"] or eng.obs_param is None:
            raise ValueError("dispersion_stats(): an engine of the negative-binomial model with one xi per neuron is required")
        c = self._scratch()
        eng._upload_weights(a, W, b)
        eng.fold_data("dispersion_fold", lambda i, ds, st, first: call(
            "pgl_dispersion_fold", Psi=ptr(ds.Psi), ldn=eng.ldn, bias=ptr(eng.bias), Y=ptr(ds.Y), T=ds.T, nloc=eng.nloc,
            xi=ptr(eng.obs_param), seed=int(seed) & (2 ** 64 - 1), sweep=int(sweep) & (2 ** 64 - 1), neuron0=eng.n0, elem0=ds.elem0,
            L=ptr(c.L), S=ptr(c.S), accumulate=int(not first), work=ptr(c.work), hip_stream=st))
        return c.L.cpu().numpy(), c.S.cpu().numpy()


def table_mean(m, xi):
    """E[l] of a cell of count m: sum_{i < m} xi / (xi + i)"""
    i = np.arange(int(m), dtype=np.float64)
    return float(np.sum(xi / (xi + i)))


def draw_xi(reg, L, S, seed, sweep, neuron):
    """xi ~ Gamma(e0 + L, rate f0 + S) of regression `reg` (its xi_posterior): the standard gamma variate from the host, as eta's is, on
    counter lane XI_LANE of (seed, sweep, GLOBAL neuron)"""
    alpha, rate = reg.xi_posterior(L, S)
    return float(make_gamma_draws(seed, sweep, [neuron], alpha, lane=XI_LANE)[0] / rate)
