"""Forward simulation of a population model: the device path of `NetworkGLM.generate()` (reference pyglm/models.py:98-151), and -- second half
of this file -- posterior predictive simulation, `model.simulate()` / `model.predictive_check()`: its law, the NumPy path and the driver of
pgl_simulate; and -- last part -- conditional simulation, `model.conditional_simulate()` / `model.conditional_check()`: some neurons are drawn
while the others are clamped to a recording (its law: conditional_host; the driver of pgl_conditional_simulate).

generate():

The bins are simulated by pgl_generate (pyglm_amd/csrc/pgl_generate.hip), a chunk of bins per launch, serial in t inside the launch.
The random numbers are NumPy's, drawn on the host in the reference's order: the reference draws `npr.rand(N)` (Bernoulli) or
`npr.randn(N)` (Gaussian) once per bin, and one `rand(Tc, N)` / `randn(Tc, N)` call gives the same values, and leaves the global
generator in the same state, as Tc calls of `rand(N)` / `randn(N)` (legacy RandomState; the cached second Gaussian included).  The draws
of chunk k+1 are made while chunk k runs.  Y stays on the device until the end; X is then formed once from it by pgl_design_matrix
(the convolution add_data uses) and read back.
"""
import ctypes

import numpy as np
import numpy.random as npr

from . import _lib
from . import regression as _reg
from ._lib import PglError, call, ptr

OBS_BERNOULLI, OBS_GAUSSIAN = _reg.MODELS["bernoulli"].generate, _reg.MODELS["gaussian"].generate      # obs of pgl_generate
MAX_CHUNK_BINS = 16384          # bins per launch at most
CHUNK_DRAWS = 1 << 22           # host draws per chunk (N * bins): 32 MiB of U
CHUNK_MACS = 1 << 33            # multiply-adds per launch (N * N * B * bins): no single launch runs for long
X_BLOCK_BYTES = 1 << 30         # device scratch of the design matrix, formed in blocks of rows


def chunk_bins(N, B, R=1):
    """bins per launch for an N-neuron, B-basis model, R replicates sharing the launch"""
    return int(max(1, min(MAX_CHUNK_BINS, CHUNK_DRAWS // (N * R), CHUNK_MACS // (N * N * B * R))))


def _device(what, device):
    """what both device paths start with: the GPU check, the library, the device -> (dev, handle of its current stream)"""
    import torch
    if not torch.cuda.is_available():
        raise PglError("the device path of %s() needs a ROCm GPU (torch.cuda.is_available() is False)" % what)
    _lib.load()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    return dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _upload(dev, Wm, bias, basis):
    """the model on the device, float64 and contiguous -> (Wm_d (N, N*B), bias_d (N,), basis_d (L, B))"""
    import torch
    Wm_d, bias_d, basis_d = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev) for v in (Wm, bias, basis))
    return Wm_d, bias_d.reshape(Wm_d.shape[0]), basis_d


def _finish_launch(entry, dev, status, status_h, first_bin, last_bin, meanwhile=None):
    """after the launch of bins first_bin..last_bin: run `meanwhile` (host work, -> its result) while it runs, wait, raise what its status reports"""
    import torch
    status_h.copy_(status, non_blocking=True)
    result = meanwhile() if meanwhile else None
    torch.cuda.current_stream(dev).synchronize()
    code = int(status_h[0])
    if code == 2:
        _raise_cap(*(int(v) for v in status_h[1:4]))
    if code:
        raise PglError("%s: a grid barrier timed out at bin %d (chunk of bins %d..%d)" % (entry, int(status_h[1]), first_bin, last_bin))
    return result


def generate(Wm, bias, basis, T, obs, noise_scale=0.0, device=None, verbose=False, intvl=10, chunk=None):
    """(X (T, N, B), Y (T, N)) of the host loop at pyglm_amd/models.py (generate), from the current state of NumPy's global generator,
    which is left where that loop leaves it.  Wm (N, N*B), bias (N,), basis (L, B) as the model holds them (basis row 0 = previous bin);
    obs OBS_BERNOULLI or OBS_GAUSSIAN (noise_scale = sqrt(eta) of the regression whose rvs the loop calls)."""
    import torch
    dev, st = _device("generate", device)
    N = np.shape(Wm)[0]
    L, B = np.shape(basis)
    assert np.shape(Wm) == (N, N * B) and obs in (OBS_BERNOULLI, OBS_GAUSSIAN)
    Tc = int(chunk) if chunk else chunk_bins(N, B)
    draw = npr.rand if obs == OBS_BERNOULLI else npr.randn
    with torch.cuda.device(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        Wm_d, bias_d, basis_d = _upload(dev, Wm, bias, basis)
        ring = torch.zeros((L, N), **f64)
        Y_d = torch.empty((T, N), **f64)
        work = torch.zeros(_lib.load().pgl_generate_work_bytes(N, B), dtype=torch.uint8, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        status_h = torch.zeros(2, dtype=torch.int32).pin_memory()
        U_h = torch.empty((min(Tc, T), N), dtype=torch.float64).pin_memory()
        U_d = torch.empty((min(Tc, T), N), **f64)
        U = draw(min(Tc, T), N)
        for t0 in range(0, T, Tc):
            n = min(Tc, T - t0)
            U_h[:n].numpy()[...] = U
            U_d[:n].copy_(U_h[:n], non_blocking=True)
            call("pgl_generate", Wm=ptr(Wm_d), bias=ptr(bias_d), basis=ptr(basis_d), N=N, B=B, L=L, obs=obs, noise_scale=float(noise_scale),
                 U=ptr(U_d), ring=ptr(ring), Y=ptr(Y_d[t0:t0 + n]), t0=t0, Tc=n, work=ptr(work), status=ptr(status), hip_stream=st)
            more = min(Tc, T - t0 - n)                     # the next chunk's draws, while this one runs
            U = _finish_launch("pgl_generate", dev, status, status_h, t0, t0 + n - 1, (lambda: draw(more, N)) if more > 0 else None)
            if verbose:
                for t in range(L + t0, L + t0 + n):
                    if t % intvl == 0:
                        print("Generate t={}".format(t))
        Y = Y_d.cpu().numpy()
        # X = the basis convolution of Y (bins before 0 are zero), in blocks of rows: pgl_design_matrix writes D = N*B columns and the bias
        # column; each block is computed from the L rows before it as well, whose outputs are dropped
        D = N * B
        X = np.empty((T, N, B))
        X2 = torch.from_numpy(X.reshape(T, D))
        rows = max(1, min(T, X_BLOCK_BYTES // (8 * (D + 1)) - L))
        Xs = torch.empty((rows + L, D + 1), **f64)
        for r0 in range(0, T, rows):
            r1 = min(T, r0 + rows)
            h = min(L, r0)
            call("pgl_design_matrix", S=ptr(Y_d[r0 - h:]), lds=N, basis=ptr(basis_d), X=ptr(Xs), ldx=D + 1, Xt=None, ldxt=0, T=r1 - r0 + h,
                 N=N, B=B, R=L, clip=0, hip_stream=st)
            X2[r0:r1].copy_(Xs[h:h + r1 - r0, :D])
    return X, Y


# =====================================================================================================================================
# Posterior predictive simulation: model.simulate() / model.predictive_check().
#
# THE LAW (the header comment of pgl_simulate in pyglm_amd/csrc/pgl_generate.hip states the same; the kernel and the NumPy path below are
# two separately written implementations of it and are tested against each other):
#   activation   psi_t[r, n] = (a*W)[n, :] . x_t[r] + b[n]  -- the activation of `means` and log_likelihood(), not generate()'s stored W --
#                x_t[r][m, :] = sum_l Y_r[t-1-l, m] basis[l, :]
#   model        per neuron, from its own regression: kind[n] in KINDS, par[n] = (unused, sqrt(eta_n), xi_n, n_n)
#   stream       Philox4x32-10: key = seed, counter = (j | PURPOSE_SIM << 24, t, global neuron, replicate), j = 0, 1, ...; a call gives two
#                uniforms ((x >> 11) + 0.5) / 2^53 from its low and high 64 bits; u1, u2 = those of call j = 0.  Path r depends on (seed, r,
#                the parameters, its initial history) and on nothing else.
#   Bernoulli    y = u1 < 1 / (1 + exp(-psi))
#   Gaussian     y = psi + par * (sqrt(-2 log u1) * cos(2 pi u2))
#   binomial     n = par <= BINOMIAL_MAX_N (a larger n is refused: f = q^n is formed by n multiplications).  pp = 1 / (1 + exp(|psi|)),
#                q = 1 - pp, s = pp / q, f = q^n; c = f, k = 0; while u1 >= c and k < n: f = f * (n - k) / (k + 1) * s, k += 1, c = c + f.
#                y = k, or n - k when psi > 0
#   neg. binom.  xi = par, p = 1 / (1 + exp(-psi)), softplus = max(psi, 0) + log1p(exp(-|psi|)), f = exp(-xi * softplus); c = f, k = 0;
#                while u1 >= c and k < NEGBIN_CAP: f = f * p * (k + xi) / (k + 1), k += 1, c = c + f.  y = k; k = NEGBIN_CAP is an error that
#                names bin, replicate and neuron (an exploding count model)
#   Every fp64 operation of the walks is evaluated left to right as written.
#   offset       a model with covariates or latent common input (covariates.py, latents.py):
#                psi_t[r, n] = ((a*W)[n, :] . x_t[r] + b[n]) + o_r[t, n] -- the offset added last, as one rounded sum --,
#                o_r = covariates.offset_host([S_obs | X_r], beta), beta = [covariate weights | latent loadings] (N, K): from 0.0, columns
#                ascending, a rounded product then a rounded sum (simulate_offset_host).  X_r (T, Q): given, or the prior's path of
#                replicate r (latent_prior_host).
PURPOSE_SIM = 2
PURPOSE_SIM_LATENT = _lib.PGL_PURPOSE_SIM_LATENT     # the normals of the latents' prior paths: stream = replicate, element = time bin, call = factor
KINDS = tuple(sorted(_reg.MODELS, key=lambda name: _reg.MODELS[name].sim_kind))          # KINDS[kind[n]]: the model's name
KIND_BERNOULLI, KIND_GAUSSIAN, KIND_NEGBIN, KIND_BINOMIAL = (_reg.MODELS[name].sim_kind for name in KINDS)
NEGBIN_CAP = 65535
BINOMIAL_MAX_N = _lib.PGL_SIM_BINOMIAL_MAX_N
HOST_BLOCK_BINS = 4096          # bins the host path keeps in its rolling buffer when the paths are not kept
PGL_LAG_MAX = _lib.PGL_LAG_MAX  # lags of the cross-correlogram at most
LAG_I8, LAG_F64 = _lib.PGL_LAG_I8, _lib.PGL_LAG_F64     # modes of pgl_lagged_products: the counts on the int8 matrix cores (exact), any real Y through the fp64 contraction
LAG_REDOS = 0                   # folds of simulate_device that the int8 mode refused (a count beyond 127) and the fp64 mode redid, since import
PGL_ISI_MAX_BINS = _lib.PGL_ISI_MAX_BINS    # bins of the inter-spike-interval histogram at most

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, seed):
    """Philox4x32-10 on arrays of counter words (broadcast against each other), key = (seed lo, seed hi) -> four uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & _M32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & _M32, (p0 >> s32) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return [v.astype(np.uint32) for v in c]


def philox_words(seed, purpose, j, elem0, stream, n):
    """(n, 4) uint32: the words of call j for elements elem0 .. elem0 + n - 1 of `stream` (what pgl_philox_words gives on the device)"""
    elem = (int(elem0) + np.arange(n, dtype=np.uint64)) & _M32
    w = philox4x32_10((int(j) & 0xFFFFFF) | (int(purpose) << 24), elem, int(stream) & 0xFFFFFFFF, (int(stream) >> 32) & 0xFFFFFFFF, seed)
    return np.stack(w, axis=-1)


def _unit(lo, hi):
    x = lo.astype(np.uint64) | (hi.astype(np.uint64) << np.uint64(32))
    return ((x >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def sim_uniforms(seed, t, neurons, replicates):
    """(u1, u2), each (len(replicates), len(neurons)): the two uniforms of call 0 of every (replicate, neuron) stream at time bin t"""
    o = philox4x32_10(PURPOSE_SIM << 24, int(t), np.asarray(neurons, dtype=np.uint64)[None, :], np.asarray(replicates, dtype=np.uint64)[:, None], seed)
    return _unit(o[0], o[1]), _unit(o[2], o[3])


def observation_models(regressions):
    """-> [regression.ObsModel] of the regressions, each from its own model; ValueError for a regression whose rvs is not one of the four
    built-in ones (an override in a class, an attribute of the instance, a subclass that changes the hooks but not rvs)"""
    models = []
    for i, r in enumerate(regressions):
        try:
            model = _reg.MODELS.get(_reg._kind(r))
        except TypeError:
            model = None
        if model is None or not _reg.is_builtin(r, model, "rvs"):
            raise ValueError("simulate(): regression %d (%s) does not draw from one of the built-in observation models (%s); a user-defined rvs "
                             "or observation model cannot be simulated" % (i, type(r).__name__, ", ".join(KINDS)))
        if model.sim_kind == KIND_BINOMIAL and r.n > BINOMIAL_MAX_N:
            raise ValueError("simulate(): regression %d is Binomial with n = %d; the sampler supports n <= %d" % (i, r.n, BINOMIAL_MAX_N))
        models.append(model)
    return models


def observation_kinds(regressions):
    """-> (kind (N,) int32, par (N,) float64) of pgl_simulate, of observation_models(regressions)"""
    models = observation_models(regressions)
    return (np.array([m.sim_kind for m in models], dtype=np.int32),
            np.array([m.sim_par(r) for m, r in zip(models, regressions)], dtype=np.float64))


def first_without_events(models):
    """index of the first of `models` that has no events (Gaussian: no inter-spike or rescaled intervals), or None"""
    return next((i for i, m in enumerate(models) if not m.events), None)


def host_draw(kind, par, psi, u1, u2):
    """y (R, N) of THE LAW from psi, u1, u2 (R, N) and the per-neuron kind / par (N,); and the (replicate row, neuron) of the first
    negative-binomial walk that reached NEGBIN_CAP, or None"""
    y = np.empty_like(psi)
    capped = None
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = np.flatnonzero(kind == KIND_BERNOULLI)
        if m.size:
            y[:, m] = u1[:, m] < 1.0 / (1.0 + np.exp(-psi[:, m]))
        m = np.flatnonzero(kind == KIND_GAUSSIAN)
        if m.size:
            y[:, m] = psi[:, m] + par[m] * (np.sqrt(-2.0 * np.log(u1[:, m])) * np.cos(2.0 * np.pi * u2[:, m]))
        m = np.flatnonzero(kind == KIND_BINOMIAL)
        if m.size:
            ps, u = psi[:, m], u1[:, m]
            n = np.broadcast_to(par[m].astype(np.int64), ps.shape)
            pp = 1.0 / (1.0 + np.exp(np.abs(ps)))
            q = 1.0 - pp
            s = pp / q
            f = np.ones_like(ps)
            for i in range(int(n.max()) if n.size else 0):
                f = np.where(i < n, f * q, f)
            c = f.copy()
            k = np.zeros(ps.shape, dtype=np.int64)
            while True:
                act = (u >= c) & (k < n)
                if not act.any():
                    break
                f = np.where(act, f * (n - k).astype(np.float64) / (k + 1).astype(np.float64) * s, f)
                k = k + act
                c = np.where(act, c + f, c)
            y[:, m] = np.where(ps > 0.0, n - k, k)
        m = np.flatnonzero(kind == KIND_NEGBIN)
        if m.size:
            ps, u = psi[:, m].ravel(), u1[:, m].ravel()
            xi = np.broadcast_to(par[m], psi[:, m].shape).ravel()
            p = 1.0 / (1.0 + np.exp(-ps))
            softplus = np.where(ps > 0.0, ps, 0.0) + np.log1p(np.exp(-np.abs(ps)))
            f = np.exp(-xi * softplus)
            c = f.copy()
            k = np.zeros(ps.shape, dtype=np.int64)
            idx = np.flatnonzero(u >= c)                    # the walks still going (all at the same k: they all started at 0)
            step = 0
            while idx.size and step < NEGBIN_CAP:
                fi = f[idx] * p[idx] * (step + xi[idx]) / float(step + 1)
                step += 1
                f[idx] = fi
                k[idx] = step
                ci = c[idx] + fi
                c[idx] = ci
                idx = idx[u[idx] >= ci]
            hit = np.flatnonzero(k >= NEGBIN_CAP)
            if hit.size:
                capped = (int(hit[0] // m.size), int(m[hit[0] % m.size]))
            y[:, m] = k.reshape(-1, m.size)
    return y, capped


class Simulation(object):
    """what model.simulate() returns: Y (R, T, N) float64 or None (keep_paths=False); sum and sumsq (R, N), the sums of y and y^2 over the T
    bins, added in time order; history (R, L, N), the last L bins of every replicate in time order; t0 / t1, the first bin simulated and the
    first bin not simulated; seed and first_replicate.  Passed as `history=` of the next call it continues the same trajectories.
    With lags = K > 0: lagged (R, K, N, N), the lagged products of the T bins of this call (lagged_products_host states them; a device tensor
    if the caller asked for that), and lag_redos, the folds that the int8 kernel refused and the fp64 one redid.
    With isi = D > 0: isi (R, N, D) and isi_moments (R, N, 3), int64, the inter-spike-interval histogram and (M, sum d, sum d^2) of every
    replicate (isi_host states them) over the events of the T bins of THIS call only: a call that continues a `history=` does not count the
    interval from the history's last event to its own first one.
    Of a model with latent factors: latents (R, T, Q), or (1, T, Q) where the replicates share them -- kept with keep_paths=True, else None
    --, and latent_last (R, Q), every replicate's factors at the last bin: the carry from which `history=` this Simulation continues the
    prior's AR(1) paths.  Both None without latents."""

    def __init__(self, Y, sum, sumsq, history, t0, t1, seed, first_replicate, lagged=None, lag_redos=0, isi=None, isi_moments=None,
                 latents=None, latent_last=None):
        self.Y, self.sum, self.sumsq, self.history = Y, sum, sumsq, history
        self.latents, self.latent_last = latents, latent_last
        self.t0, self.t1, self.seed, self.first_replicate = int(t0), int(t1), int(seed), int(first_replicate)
        self.lagged, self.lag_redos = lagged, int(lag_redos)
        self.isi, self.isi_moments = isi, isi_moments

    def _isi(self):
        if self.isi is None:
            raise ValueError("the interval statistics need simulate(..., isi=D) with D >= 2")
        return self.isi, self.isi_moments

    def isi_density(self):
        """the interval histogram over the number of intervals, (R, N, D); NaN where a train has no interval"""
        return isi_density(*self._isi())

    def isi_mean(self):
        """mean interval in bins, (R, N); NaN where a train has no interval"""
        return isi_mean(self._isi()[1])

    def isi_cv(self):
        """coefficient of variation of the intervals, (R, N); NaN where a train has fewer than two"""
        return isi_cv(self._isi()[1])

    def correlogram(self):
        """the lagged cross-correlogram of every replicate, (R, K, N, N): correlogram() of `lagged`"""
        if self.lagged is None:
            raise ValueError("correlogram(): simulate(..., lags=K) with K > 0 collects the lagged products")
        return correlogram(self.lagged, self.sum, self.sumsq, self.T)

    @property
    def T(self):
        return self.t1 - self.t0

    def rate(self):
        """mean of y per bin, (R, N)"""
        return self.sum / self.T

    def fano(self):
        """variance / mean of y over the bins, (R, N); NaN where the mean is zero"""
        return fano_factor(self.sum, self.sumsq, self.T)

    def __iter__(self):                       # (Y, sum, sumsq, history) = model.simulate(...)
        return iter((self.Y, self.sum, self.sumsq, self.history))


def fano_factor(s, ss, T):
    mean = np.asarray(s, dtype=np.float64) / T
    var = np.asarray(ss, dtype=np.float64) / T - mean * mean
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(mean != 0.0, var / mean, np.nan)


def check_isi_bins(bins):
    """D = int(bins) of an inter-spike-interval histogram: 0 (none), or 2 <= D <= PGL_ISI_MAX_BINS, else ValueError"""
    D = int(bins)
    if D != 0 and not 2 <= D <= PGL_ISI_MAX_BINS:
        raise ValueError("isi = %d: 0, or 2 <= isi <= PGL_ISI_MAX_BINS = %d bins, is required" % (D, PGL_ISI_MAX_BINS))
    return D


def isi_host(Y, bins):
    """THE DEFINITION of the inter-spike-interval statistics of a series Y (T, N) -> (hist (N, D), moments (N, 3)), int64.  An event of neuron
    n is a bin with Y[t, n] > 0 (a count above 1 is one event; NaN and negative values are none); an interval is the difference of the bin
    indices of two consecutive events of a neuron -- the time before its first and after its last event is censored.  hist[n, d - 1] counts
    the intervals of length d < D, hist[n, D - 1] those of length >= D; moments[n] = (M, sum d, sum d^2) over all of them, unclipped"""
    Y = np.asarray(Y, dtype=np.float64)
    D = check_isi_bins(bins)
    if D == 0 or Y.ndim != 2:
        raise ValueError("isi_host(): a series (T, N) and 2 <= bins <= %d are required" % PGL_ISI_MAX_BINS)
    N = Y.shape[1]
    hist, moments = np.zeros((N, D), dtype=np.int64), np.zeros((N, 3), dtype=np.int64)
    for n in range(N):
        d = np.diff(np.flatnonzero(Y[:, n] > 0)).astype(np.int64)
        hist[n] = np.bincount(np.minimum(d, D) - 1, minlength=D)
        moments[n] = d.size, d.sum(), (d * d).sum()
    return hist, moments


def _isi_fold_host(hist, moments, since, block):
    """the running statistics hist (R, N, D), moments (R, N, 3), since (R, N) += the new rows block (R, rows, N).  since: bins from the train's
    last event to the end of the rows folded so far, -1 before its first event: the first event of the block, at row u, closes an interval of
    u + 1 + since bins"""
    R, rows, N = block.shape
    D = hist.shape[2]
    for r in range(R):
        for n in range(N):
            ev = np.flatnonzero(block[r, :, n] > 0).astype(np.int64)
            if ev.size == 0:
                if since[r, n] >= 0:
                    since[r, n] += rows
                continue
            d = np.diff(ev)
            if since[r, n] >= 0:
                d = np.concatenate(([ev[0] + 1 + since[r, n]], d))
            hist[r, n] += np.bincount(np.minimum(d, D) - 1, minlength=D)
            moments[r, n] += (d.size, d.sum(), (d * d).sum())
            since[r, n] = rows - 1 - ev[-1]


def isi_density(hist, moments):
    """hist / M; NaN where M = 0"""
    M = np.asarray(moments)[..., 0:1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(M > 0, np.asarray(hist, dtype=np.float64) / M, np.nan)


def isi_mean(moments):
    m = np.asarray(moments, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(m[..., 0] > 0, m[..., 1] / m[..., 0], np.nan)


def isi_cv(moments):
    """sqrt(sum d^2 / M - mean^2) / mean; NaN where M < 2"""
    m = np.asarray(moments, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = m[..., 1] / m[..., 0]
        return np.where(m[..., 0] > 1, np.sqrt(np.maximum(m[..., 2] / m[..., 0] - mean * mean, 0.0)) / mean, np.nan)


class _IsiFold(object):
    """the running interval statistics on the device: hist (R, N, D) int32, moments (R, N, 3) int64, since (R, N) int32, folded chunk by chunk
    through pgl_isi_fold"""

    def __init__(self, dev, st, N, D, R, max_rows):
        import torch
        self.st, self.N, self.D, self.R = st, N, D, R
        self.hist = torch.empty((R, N, D), dtype=torch.int32, device=dev)
        self.moments = torch.empty((R, N, 3), dtype=torch.int64, device=dev)
        self.since = torch.empty((R, N), dtype=torch.int32, device=dev)
        self.work = torch.empty(_lib.load().pgl_isi_work_bytes(N, R, max_rows), dtype=torch.uint8, device=dev)
        self.first = True

    def fold(self, Y, ldy, strideY, rows):
        """Y: the tensor that starts at the first new row of replicate 0"""
        call("pgl_isi_fold", Y=ptr(Y), ldy=ldy, strideY=strideY, rows=rows, N=self.N, R=self.R, D=self.D, hist=ptr(self.hist),
             moments=ptr(self.moments), since=ptr(self.since), accumulate=0 if self.first else 1, work=ptr(self.work), hip_stream=self.st)
        self.first = False

    def finish(self):
        return self.hist.cpu().numpy().astype(np.int64), self.moments.cpu().numpy()


def isi_device(Y, bins, device=None):
    """isi_host(Y, bins) of Y (T, N) through one pgl_isi_fold call"""
    import torch
    dev, st = _device("isi_histogram", device)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    D = check_isi_bins(bins)
    if D == 0 or Y.ndim != 2:
        raise ValueError("isi_device(): a series (T, N) and 2 <= bins <= %d are required" % PGL_ISI_MAX_BINS)
    T, N = Y.shape
    with torch.cuda.device(dev):
        fold = _IsiFold(dev, st, N, D, 1, T)
        fold.fold(torch.from_numpy(Y).to(dev), N, T * N, T)
        hist, moments = fold.finish()
    return hist[0], moments[0]


def check_lags(lags, T):
    """K = int(lags) of a series of T bins: 0 <= K <= PGL_LAG_MAX and K - 1 < T, else ValueError"""
    K = int(lags)
    if K < 0 or K > PGL_LAG_MAX:
        raise ValueError("lags = %d: 0 <= lags <= PGL_LAG_MAX = %d is required" % (K, PGL_LAG_MAX))
    if K > 0 and K - 1 >= T:
        raise ValueError("lags = %d needs more than %d bins, got T = %d" % (K, K - 1, T))
    return K


def lagged_products_host(Y, lags):
    """THE DEFINITION of the lagged products of a series Y (T, N): S (K, N, N), S[l, i, j] = sum_{t = 0}^{T-1-l} Y[t, i] Y[t+l, j] -- neuron i
    leads neuron j by l bins --, one matrix product per lag"""
    Y = np.asarray(Y, dtype=np.float64)
    T, N = Y.shape
    K = check_lags(lags, T)
    S = np.empty((K, N, N))
    for l in range(K):
        S[l] = Y[:T - l].T @ Y[l:]
    return S


def correlogram(S, sum, sumsq, T):
    """the lagged cross-correlogram from the lagged products S (..., K, N, N) and the whole-series sums of y and y^2 (..., N) over T bins:
    c[l, i, j] = (S[l, i, j] / (T - l) - m_i m_j) / sqrt(v_i v_j), m = sum / T, v = sumsq / T - m^2; NaN where v_i v_j <= 0.  NumPy arrays,
    or torch tensors (every operand on the device of S): the same operations in the same order"""
    K = S.shape[-3]
    if isinstance(S, np.ndarray):
        mean = np.asarray(sum, dtype=np.float64) / T
        var = np.asarray(sumsq, dtype=np.float64) / T - mean * mean
        cnt = (T - np.arange(K, dtype=np.float64))[:, None, None]
        den = var[..., None, :, None] * var[..., None, None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            c = (S / cnt - mean[..., None, :, None] * mean[..., None, None, :]) / np.sqrt(den)
        return np.where(den > 0.0, c, np.nan)
    import torch
    mean = sum / T
    var = sumsq / T - mean * mean
    cnt = (T - torch.arange(K, dtype=torch.float64, device=S.device))[:, None, None]
    den = var[..., None, :, None] * var[..., None, None, :]
    c = (S / cnt - mean[..., None, :, None] * mean[..., None, None, :]) / torch.sqrt(den)
    return torch.where(den > 0.0, c, torch.full_like(c, float("nan")))


def _fold_host(S, buf, a, b, prev):
    """S (R, K, N, N) += the lagged products of the new rows buf[:, a:b] with themselves and with the `prev` rows before them"""
    for l in range(S.shape[1]):
        u0 = max(0, l - prev)
        if u0 < b - a:
            S[:, l] += np.matmul(buf[:, a + u0 - l:b - l].transpose(0, 2, 1), buf[:, a + u0:b])


def lag_mode_of(Y):
    """LAG_I8 if every value of the array is an integer of [-127, 127] (the int8 kernel takes it), else LAG_F64"""
    Y = np.asarray(Y)
    return LAG_I8 if Y.size == 0 or (np.all(np.abs(Y) <= 127.0) and np.all(Y == np.rint(Y))) else LAG_F64


def lagged_products_device(Y, lags, mode=None, device=None):
    """lagged_products_host(Y, lags) of Y (T, N) through pgl_lagged_products, as one chunk; mode None: LAG_I8 where lag_mode_of(Y) allows it"""
    import torch
    dev, st = _device("cross_correlogram", device)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    T, N = Y.shape
    K = check_lags(lags, T)
    mode = lag_mode_of(Y) if mode is None else mode
    with torch.cuda.device(dev):
        Y_d = torch.from_numpy(Y).to(dev)
        S = torch.empty((K, N, N), dtype=torch.float64, device=dev)
        work = torch.empty(_lib.load().pgl_lagged_work_bytes(N, K, 1, T), dtype=torch.uint8, device=dev)
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        call("pgl_lagged_products", Y=ptr(Y_d), ldy=N, strideY=T * N, rows=T, prev=0, N=N, K=K, R=1, S=ptr(S), strideS=K * N * N, accumulate=0,
             mode=mode, work=ptr(work), status=ptr(status), hip_stream=st)
        code = status.cpu().numpy()
        if code[0]:
            raise PglError("pgl_lagged_products: the value of neuron %d at row %d is no integer of [-127, 127]" % (code[3], code[1]))
        return S.cpu().numpy()


class _LagFold(object):
    """the running lagged products of simulate_device: S (R, K, N, N) on the device, folded chunk by chunk through pgl_lagged_products.  The mode
    is fp64 if a neuron is Gaussian, else int8; where counts can pass 127 (negative-binomial neurons) the status of every int8 fold is read,
    and a refused fold -- S untouched, the chunk still in the buffer -- is redone in fp64."""

    def __init__(self, dev, st, N, K, R, max_rows, kind):
        import torch
        self.dev, self.st, self.N, self.K, self.R = dev, st, N, K, R
        self.S = torch.empty((R, K, N, N), dtype=torch.float64, device=dev)
        self.work = torch.empty(_lib.load().pgl_lagged_work_bytes(N, K, R, max_rows), dtype=torch.uint8, device=dev)
        self.status = torch.zeros(4, dtype=torch.int32, device=dev)
        self.mode = LAG_F64 if np.any(kind == KIND_GAUSSIAN) else LAG_I8
        self.unbounded = bool(np.any(kind == KIND_NEGBIN))
        self.first, self.redos = True, 0

    def _call(self, Y, strideY, rows, prev, mode):
        call("pgl_lagged_products", Y=ptr(Y), ldy=self.N, strideY=strideY, rows=rows, prev=prev, N=self.N, K=self.K, R=self.R, S=ptr(self.S),
             strideS=self.K * self.N * self.N, accumulate=0 if self.first else 1, mode=mode, work=ptr(self.work), status=ptr(self.status),
             hip_stream=self.st)

    def fold(self, Y, strideY, rows, prev):
        """Y: the tensor that starts at the first new row of replicate 0"""
        global LAG_REDOS
        self._call(Y, strideY, rows, prev, self.mode)
        if self.mode == LAG_I8 and self.unbounded and int(self.status[0]) == 3:      # (reading the status waits for the fold)
            self.status.zero_()
            self._call(Y, strideY, rows, prev, LAG_F64)
            self.redos += 1
            LAG_REDOS += 1
        self.first = False

    def finish(self):
        code = self.status.cpu().numpy()
        if code[0]:
            raise PglError("pgl_lagged_products: neuron %d of replicate %d at row %d of its chunk is no integer of [-127, 127]"
                           % (code[3], code[2], code[1]))
        return self.S


def _initial_history(history, R, L, N, t0):
    """-> (hist (R, L, N) in time order, t0).  history: None (silence), a Simulation (continue it), (rows, N) -- the last rows of a data set,
    the same for every replicate; fewer than L rows are preceded by silence, of more only the last L are used -- or (R, rows, N)"""
    if isinstance(history, Simulation):
        if t0 is None:
            t0 = history.t1
        history = history.history
    t0 = 0 if t0 is None else int(t0)
    hist = np.zeros((R, L, N))
    if history is not None:
        h = np.asarray(history, dtype=np.float64)
        if h.ndim == 2:
            h = np.broadcast_to(h[None], (R,) + h.shape)
        if h.ndim != 3 or h.shape[0] != R or h.shape[2] != N:
            raise ValueError("history must be (rows, N = %d) or (replicates = %d, rows, N), got %r" % (N, R, np.shape(history)))
        h = h[:, -L:]
        hist[:, L - h.shape[1]:] = h
    if t0 < 0:
        raise ValueError("t0 must be >= 0")
    return hist, t0


def _raise_cap(t, rep, n):
    raise PglError("simulate(): the negative-binomial draw of neuron %d in replicate %d at bin %d reached the cap of %d: the count model "
                   "explodes at this state (the rate grows without bound)" % (n, rep, t, NEGBIN_CAP))


def latent_normals_sim_host(seed, reps, t0, T, Q):
    """z (len(reps), T, Q): the standard normals of the latents' prior paths as the device draws them -- Philox4x32-10, key = seed, counter =
    (q | PURPOSE_SIM_LATENT << 24, t0 + k, replicate lo, replicate hi); words (0, 1) of call q make u0, words (2, 3) u1,
    z = sqrt(-2 log u0) cos(2 pi u1) (latents.latent_normals_host on another purpose and stream)"""
    reps = np.atleast_1d(np.asarray(reps, dtype=np.int64))
    z = np.empty((reps.size, T, Q))
    for i, r in enumerate(reps):
        for q in range(Q):
            w = philox_words(seed, PURPOSE_SIM_LATENT, q, t0, int(r), T)
            u0, u1 = _unit(w[:, 0], w[:, 1]), _unit(w[:, 2], w[:, 3])
            z[i, :, q] = np.sqrt(-2.0 * np.log(u0)) * np.cos(2.0 * np.pi * u1)
    return z


def latent_recurrence_host(z, phi, carry=None):
    """x (R, T, Q) from the normals z (R, T, Q): x[0] = z[0] without a carry -- the stationary start --, else x_t = fl(fl(phi x_{t-1}) +
    fl(s z_t)), s = sqrt(1 - phi^2), x_{-1} = carry (R, Q).  No fused multiply-add; phi = 0 gives z itself"""
    z = np.asarray(z, dtype=np.float64)
    phi = np.asarray(phi, dtype=np.float64).reshape(z.shape[2])
    s = np.sqrt(1.0 - phi * phi)
    x = np.empty_like(z)
    prev = None if carry is None else np.asarray(carry, dtype=np.float64).reshape(z.shape[0], z.shape[2])
    for k in range(z.shape[1]):
        if prev is None:
            cur = z[:, k].copy()
        else:
            a, b = phi * prev, s * z[:, k]            # two rounded products, then one rounded sum
            cur = a + b
        x[:, k] = cur
        prev = cur
    return x


def latent_prior_host(seed, reps, t0, T, phi, carry=None):
    """THE LAW of the latents' prior paths -> X (len(reps), T, Q): per factor q a stationary AR(1) process with coefficient phi[q] and
    marginal variance 1 (N(0, I) per bin at phi = 0), on the normals of latent_normals_sim_host.  reps: the absolute replicate indices; t0: the
    first bin; carry (R, Q): the factors at bin t0 - 1 of a trajectory that is continued, None: bin t0 starts it.  A path depends on (seed,
    replicate, q, the bin the trajectory started at, phi) alone"""
    phi = np.atleast_1d(np.asarray(phi, dtype=np.float64))
    return latent_recurrence_host(latent_normals_sim_host(seed, reps, t0, int(T), phi.size), phi, carry)


def simulate_offset_host(S_obs, X, beta):
    """o (R' , T, N) of THE LAW: covariates.offset_host([S_obs | X_r], beta) per replicate of X.  S_obs (T, K_obs) or None; X (R', T, Q) or None
    (then R' = 1); beta (N, K_obs + Q)"""
    from .covariates import offset_host
    parts = []
    for r in range(1 if X is None else np.shape(X)[0]):
        cols = [v for v in (S_obs, None if X is None else np.asarray(X)[r]) if v is not None]
        parts.append(offset_host(np.concatenate(cols, axis=1), beta))
    return np.stack(parts)


class Drive(object):
    """what a model with covariates or latents adds to the activation of a simulation of T bins: beta (N, K) = [covariate weights | latent
    loadings]; S_obs (T, K_obs) or None, row k for the k-th simulated bin; and the latents -- "prior" (with phi (Q,)) or an array (1, T, Q),
    shared by the replicates, or (R, T, Q) -- or None where Q = 0.  What model.simulate() hands to simulate()"""

    def __init__(self, beta, S_obs=None, latents=None, phi=None):
        self.beta = np.ascontiguousarray(beta, dtype=np.float64)
        self.S_obs = None if S_obs is None else np.ascontiguousarray(S_obs, dtype=np.float64)
        self.K_obs = 0 if self.S_obs is None else self.S_obs.shape[1]
        self.Q = self.beta.shape[1] - self.K_obs
        self.prior = isinstance(latents, str) and latents == "prior"
        self.X = None if self.prior or latents is None else np.ascontiguousarray(latents, dtype=np.float64)
        self.phi = np.zeros(self.Q) if phi is None else np.ascontiguousarray(phi, dtype=np.float64)
        if (self.Q > 0) != (self.prior or self.X is not None) or (self.X is not None and (self.X.ndim != 3 or self.X.shape[2] != self.Q)):
            raise ValueError("Drive: beta has %d columns for %d observed covariates, and the latents do not have the other %d" %
                             (self.beta.shape[1], self.K_obs, self.Q))

    def host(self, seed, R, rep0, t0, T, carry):
        """-> (offset (R or 1, T, N), X (R or 1, T, Q) or None, latent_last (R, Q) or None) by the host law"""
        X = latent_prior_host(seed, rep0 + np.arange(R), t0, T, self.phi, carry) if self.prior else self.X
        return simulate_offset_host(self.S_obs, X, self.beta), X, self.last(X, R)

    def last(self, X, R):
        return None if X is None else np.ascontiguousarray(np.broadcast_to(X[:, -1], (R, self.Q)))


def simulate_host(Wm, bias, basis, kind, par, T, R, seed, rep0, hist, t0, keep_paths, lags=0, isi=0, offset=None):
    """THE LAW in NumPy, vectorised over (R, N) per bin -> Simulation.  lags = K > 0: the lagged products of the T bins as well, folded block by
    block from the rolling buffer, which then keeps max(L, K - 1) rows in front.  isi = D > 0: the interval statistics, folded from the same
    blocks with the `since` carry.  offset (R or 1, T, N): added to the activation last, as one rounded sum; None: no such term"""
    Wm = np.ascontiguousarray(Wm, dtype=np.float64)
    N = Wm.shape[0]
    L, B = basis.shape
    WmT = np.ascontiguousarray(Wm.T)
    bias = np.asarray(bias, dtype=np.float64).reshape(N)
    C = T if keep_paths else min(T, HOST_BLOCK_BINS)
    K = int(lags)
    H = max(L, K - 1)                                # rows in front of the block: the history, and the partners of the first K - 1 new bins
    buf = np.zeros((R, H + C, N))
    buf[:, H - L:H] = hist
    s, ss = np.zeros((R, N)), np.zeros((R, N))
    S = np.zeros((R, K, N, N)) if K else None
    D = int(isi)
    ih, im, since = (np.zeros((R, N, D), dtype=np.int64), np.zeros((R, N, 3), dtype=np.int64), np.full((R, N), -1, dtype=np.int64)) if D else (None,) * 3
    neurons, reps = np.arange(N), rep0 + np.arange(R)
    pos = H                                          # buf[:, pos] receives bin t
    for t in range(t0, t0 + T):
        if pos == H + C:
            if K:
                _fold_host(S, buf, H, pos, min(K - 1, t - t0 - C))
            if D:
                _isi_fold_host(ih, im, since, buf[:, H:pos])
            buf[:, :H] = buf[:, C:].copy()
            pos = H
        x = np.einsum("rlm,lb->rmb", buf[:, pos - L:pos][:, ::-1], basis)
        psi = x.reshape(R, N * B).dot(WmT) + bias
        if offset is not None:
            psi = psi + offset[:, t - t0]
        u1, u2 = sim_uniforms(seed, t, neurons, reps)
        y, capped = host_draw(kind, par, psi, u1, u2)
        if capped is not None:
            _raise_cap(t, rep0 + capped[0], capped[1])
        buf[:, pos] = y
        s += y
        ss += y * y
        pos += 1
    if K:
        _fold_host(S, buf, H, pos, min(K - 1, T - (pos - H)))
    if D:
        _isi_fold_host(ih, im, since, buf[:, H:pos])
    return Simulation(buf[:, H:H + T].copy() if keep_paths else None, s, ss, buf[:, pos - L:pos].copy(), t0, t0 + T, seed, rep0, lagged=S,
                      isi=ih, isi_moments=im)


class _DriveDevice(object):
    """a Drive on the device: S_obs and the k-major beta uploaded once; per chunk the prior's paths (pgl_latent_prior_paths, where the latents
    are the prior's), the offset (pgl_simulate_offset_build) and the arguments of pgl_simulate_offset -- all on the one stream"""

    def __init__(self, drive, dev, st, N, R, T, Tcap, seed, rep0, t0, carry, keep_paths):
        import torch
        self.d, self.st, self.N, self.R, self.T, self.seed, self.rep0, self.t0 = drive, st, N, R, T, seed, rep0, t0
        Q = drive.Q
        self.Rx = R if Q and (drive.prior or drive.X.shape[0] > 1) else 1      # replicates of the offset: 1 where they share it
        keep = keep_paths and drive.prior
        self.Tx = T if keep or not drive.prior else Tcap                        # rows of a replicate in the latents' buffer
        need = 8 * self.Rx * Tcap * N + (8 * self.Rx * self.Tx * Q if Q else 0)
        free = torch.cuda.mem_get_info(dev)[0]
        if need > free:
            raise PglError("simulate(covariates / latents): the offset of a chunk (%d replicates x %d bins x %d neurons) and the latents need "
                           "%d bytes of device memory, %d are free: simulate fewer replicates per call" % (self.Rx, Tcap, N, need, free))
        f64 = dict(dtype=torch.float64, device=dev)
        self.S = torch.from_numpy(drive.S_obs).to(dev) if drive.K_obs else None
        self.beta = torch.from_numpy(np.ascontiguousarray(drive.beta.T)).to(dev)        # [K][N]
        self.Off = torch.empty((self.Rx, Tcap, N), **f64)
        self.ldo_r = Tcap * N if self.Rx > 1 else 0
        self.X = self.carry = None
        if drive.prior:
            self.X = torch.empty((R, self.Tx, Q), **f64)
            self.has_carry = carry is not None
            self.carry = torch.from_numpy(np.ascontiguousarray(carry, dtype=np.float64).reshape(R, Q)).to(dev) if self.has_carry else torch.zeros((R, Q), **f64)
            self.phi = (ctypes.c_double * Q)(*drive.phi)
            self.s = (ctypes.c_double * Q)(*np.sqrt(1.0 - drive.phi * drive.phi))
        elif Q:
            self.X = torch.from_numpy(drive.X).to(dev)

    def chunk(self, k0, n):
        """queue what the launch of bins k0 .. k0 + n - 1 of the call needs -> the keywords Off, ldo_t, ldo_r of pgl_simulate_offset"""
        d, Q = self.d, self.d.Q
        X = None
        if d.prior:
            X = self.X[0, k0:] if self.Tx == self.T else self.X
            call("pgl_latent_prior_paths", X=ptr(X), ldx_r=self.Tx * Q, R=self.R, rep0=self.rep0, t0=self.t0 + k0, Tc=n, Q=Q,
                 phi=ctypes.cast(self.phi, ctypes.c_void_p), s=ctypes.cast(self.s, ctypes.c_void_p), carry=ptr(self.carry),
                 has_carry=1 if self.has_carry or k0 > 0 else 0, z_override=None, seed=self.seed & (2 ** 64 - 1), hip_stream=self.st)
        elif Q:
            X = self.X[0, k0:]
        call("pgl_simulate_offset_build", S=ptr(self.S[k0:]) if d.K_obs else None, lds=d.K_obs, X=ptr(X), ldx_r=self.Tx * Q if self.Rx > 1 else 0,
             Beta=ptr(self.beta), ldn=self.N, Off=ptr(self.Off), ldo_t=self.N, ldo_r=self.ldo_r, Tc=n, N=self.N, K_obs=d.K_obs, Q=Q, R=self.Rx,
             hip_stream=self.st)
        return dict(Off=ptr(self.Off), ldo_t=self.N, ldo_r=self.ldo_r)

    def finish(self, keep_paths):
        """-> (latents or None, latent_last or None) of the Simulation"""
        d = self.d
        if not d.Q:
            return None, None
        if d.prior:
            return (self.X.cpu().numpy() if keep_paths else None), self.carry.cpu().numpy()
        return (d.X if keep_paths else None), d.last(d.X, self.R)


def simulate_device(Wm, bias, basis, kind, par, T, R, seed, rep0, hist, t0, keep_paths, device=None, lags=0, lagged_on_device=False, isi=0,
                    drive=None, carry=None):
    """THE LAW through pgl_simulate, a chunk of bins per launch -> Simulation.  lags = K > 0: every launch writes its bins behind the K - 1 bins
    before them -- into the paths if they are kept, else into a buffer of K - 1 + chunk rows per replicate -- and pgl_lagged_products folds
    them into the running sums (_LagFold); the sums come back as a device tensor if lagged_on_device.  isi = D > 0: pgl_isi_fold folds the rows
    of every launch as well (_IsiFold) -- from the paths, else from the lag buffer, else from a buffer of one chunk kept for this alone"""
    import torch
    dev, st = _device("simulate", device)
    N = np.shape(Wm)[0]
    L, B = np.shape(basis)
    Tc = chunk_bins(N, B, R)
    K, D = int(lags), int(isi)
    with torch.cuda.device(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        if K:
            Tb = K - 1 + min(Tc, T)                                  # rows of the path buffer
            need = 8 * R * K * N * N + _lib.load().pgl_lagged_work_bytes(N, K, R, min(Tc, T)) + 8 * R * (T if keep_paths else Tb) * N
            free = torch.cuda.mem_get_info(dev)[0]
            if need > free:
                raise PglError("simulate(lags=%d, replicates=%d): the lagged products of %d replicates x %d lags x %d x %d neuron pairs, their "
                               "scratch and the paths need %d bytes of device memory, %d are free: ask for fewer lags or fewer replicates per "
                               "call" % (K, R, R, K, N, N, need, free))
        if keep_paths:
            need = 8 * R * T * N
            free = torch.cuda.mem_get_info(dev)[0]
            if need > free:
                raise PglError("simulate(keep_paths=True): the paths of %d replicates x %d bins x %d neurons need %d bytes of device memory, %d "
                               "are free: simulate fewer replicates or bins per call, or pass keep_paths=False" % (R, T, N, need, free))
        Wm_d, bias_d, basis_d = _upload(dev, Wm, bias, basis)
        kind_d = torch.from_numpy(np.ascontiguousarray(kind, dtype=np.int32)).to(dev)
        par_d = torch.from_numpy(np.ascontiguousarray(par, dtype=np.float64)).to(dev)
        rows = (t0 - L + np.arange(L)) % L               # ring row t mod L = Y[t]
        ring_h = np.empty((R, L, N))
        ring_h[:, rows] = hist
        ring = torch.from_numpy(ring_h).to(dev)
        Y_d = torch.empty((R, T, N), **f64) if keep_paths else None
        fold = _LagFold(dev, st, N, K, R, min(Tc, T), kind) if K else None
        buf = torch.empty((R, Tb, N), **f64) if K and not keep_paths else None
        ifold = _IsiFold(dev, st, N, D, R, min(Tc, T)) if D else None
        ibuf = torch.empty((R, min(Tc, T), N), **f64) if D and not K and not keep_paths else None
        sum_d, sq_d = torch.zeros((R, N), **f64), torch.zeros((R, N), **f64)
        work = torch.zeros(_lib.load().pgl_simulate_work_bytes(N, B, R), dtype=torch.uint8, device=dev)
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        status_h = torch.zeros(4, dtype=torch.int32).pin_memory()
        ddev = _DriveDevice(drive, dev, st, N, R, T, min(Tc, T), seed, rep0, t0, carry, keep_paths) if drive is not None else None
        entry = "pgl_simulate_offset" if ddev else "pgl_simulate"
        for k0 in range(0, T, Tc):
            n = min(Tc, T - k0)
            out, ldr = ((Y_d[0, k0:], T * N) if keep_paths else (buf[0, K - 1:], Tb * N) if K else (ibuf, min(Tc, T) * N) if D
                        else (None, T * N))
            okw = ddev.chunk(k0, n) if ddev else {}
            call(entry, Wm=ptr(Wm_d), bias=ptr(bias_d), basis=ptr(basis_d), N=N, B=B, L=L, kind=ptr(kind_d), par=ptr(par_d), R=R, rep0=rep0,
                 seed=seed & (2 ** 64 - 1), ring=ptr(ring), Y=ptr(out), ldr=ldr, sum=ptr(sum_d), sumsq=ptr(sq_d), t0=t0 + k0, Tc=n, work=ptr(work),
                 status=ptr(status), hip_stream=st, **okw)
            _finish_launch(entry, dev, status, status_h, t0 + k0, t0 + k0 + n - 1)
            if D:
                ifold.fold(out, N, ldr, n)
            if K:
                fold.fold(out, ldr, n, min(K - 1, k0))
                if not keep_paths and K > 1 and k0 + n < T:
                    buf[:, :K - 1] = buf[:, n:n + K - 1].clone()     # the last K - 1 bins move to the front (the ranges overlap when n < K - 1)
        rows = (t0 + T - L + np.arange(L)) % L
        lagged = fold.finish() if K else None
        if K and not lagged_on_device:
            lagged = lagged.cpu().numpy()
        ih, im = ifold.finish() if D else (None, None)
        X, last = ddev.finish(keep_paths) if ddev else (None, None)
        return Simulation(Y_d.cpu().numpy() if keep_paths else None, sum_d.cpu().numpy(), sq_d.cpu().numpy(), ring.cpu().numpy()[:, rows],
                          t0, t0 + T, seed, rep0, lagged=lagged, lag_redos=fold.redos if K else 0, isi=ih, isi_moments=im, latents=X,
                          latent_last=last)


def simulate(Wm, bias, basis, kind, par, T, replicates=1, seed=0, first_replicate=0, history=None, keep_paths=True, t0=None, on_device=False,
             device=None, lags=0, lagged_on_device=False, isi=0, drive=None):
    """R = `replicates` trajectories of T bins of the model (Wm = a*W as (N, N*B), bias, basis (L, B), per-neuron kind / par) -> Simulation;
    on the device (pgl_simulate) or in NumPy.  What model.simulate() calls once it has read the model.  lags = K > 0 (K - 1 < T): the
    Simulation carries the lagged products of its T bins (lagged_products_host) as well; lagged_on_device leaves them on the device.
    isi = D >= 2: it carries the interval histogram and moments of its T bins (isi_host) -- of the events of these bins alone, also when the
    call continues a history.
    drive: a Drive -- the covariates and latents of THE LAW's offset; where its latents are the prior's and `history` is a Simulation, their
    paths continue from its latent_last."""
    N = np.shape(Wm)[0]
    L = basis.shape[0]
    T, R, rep0, seed = int(T), int(replicates), int(first_replicate), int(seed)
    if T < 0 or R < 1 or rep0 < 0 or not 0 <= seed < 2 ** 64:
        raise ValueError("simulate(): T >= 0, replicates >= 1, first_replicate >= 0 and 0 <= seed < 2^64 are required")
    carry = history.latent_last if isinstance(history, Simulation) and drive is not None and drive.prior else None
    if carry is not None and np.shape(carry) != (R, drive.Q):
        raise ValueError("simulate(): the Simulation to continue carries latents of shape %r; (replicates = %d, n_latents = %d) is required"
                         % (np.shape(carry), R, drive.Q))
    if drive is not None:
        for name, v, want in (("covariates", drive.S_obs, (T, drive.K_obs)), ("latents", drive.X, (T, drive.Q))):
            if v is not None and (v.shape[-2:] != want or (v.ndim == 3 and v.shape[0] not in (1, R))):
                raise ValueError("simulate(): %s of shape %r; (T = %d, %d)%s is required" %
                                 (name, v.shape, want[0], want[1], " or (replicates = %d, T, %d)" % (R, want[1]) if v.ndim == 3 else ""))
    hist, t0 = _initial_history(history, R, L, N, t0)
    if t0 + T >= 2 ** 31 or rep0 + R >= 2 ** 31:
        raise ValueError("simulate(): time bins and replicate indices must stay below 2^31")
    kind, par = np.asarray(kind, dtype=np.int32), np.asarray(par, dtype=np.float64)
    K = check_lags(lags, T)
    D = check_isi_bins(isi)
    if T == 0:
        return Simulation(np.zeros((R, 0, N)) if keep_paths else None, np.zeros((R, N)), np.zeros((R, N)), hist, t0, t0, seed, rep0,
                          isi=np.zeros((R, N, D), dtype=np.int64) if D else None, isi_moments=np.zeros((R, N, 3), dtype=np.int64) if D else None,
                          latent_last=carry)
    run = simulate_device if on_device else simulate_host
    kw = dict(device=device) if on_device else {}
    host_latents = None
    if drive is not None and on_device:
        kw.update(drive=drive, carry=carry)
    elif drive is not None:
        kw["offset"], X, last = drive.host(seed, R, rep0, t0, T, carry)
        host_latents = (X if keep_paths else None), last
    if K:
        kw.update(dict(lags=K, lagged_on_device=lagged_on_device) if on_device else dict(lags=K))
    if D:
        kw["isi"] = D
    sim = run(Wm, bias, basis, kind, par, T, R, seed, rep0, hist, t0, keep_paths, **kw)
    if host_latents is not None:
        sim.latents, sim.latent_last = host_latents
    return sim


class PredictiveCheck(object):
    """Posterior predictive check of the per-neuron firing rates and Fano factors of one data set (model.predictive_check()).

        ppc = model.predictive_check(replicates=8, seed=0)
        for it in range(n_sweeps):
            model.resample_model()
            if it >= burn:
                ppc.collect()
        ppc.pvalue("rate"), ppc.rate_quantiles([0.05, 0.5, 0.95])

    collect() simulates `replicates` fresh trajectories of the data set's length from the model's current state (from silence, paths not
    kept; the k-th call uses replicate indices k R ... k R + R - 1, so no two calls share a stream) and keeps their per-neuron rates and
    Fano factors -- (S R, N) after S calls -- on the host.

    lags = K > 0 adds the pairwise statistic "xcorr", the lagged cross-correlogram (K, N, N) -- the one that sees the coupling: observed["xcorr"]
    is the data's (model.cross_correlogram), and collect() folds every replicate's correlogram, cell by cell, into #{rep >= obs}, #{rep <= obs},
    the number of replicates in which the cell is defined, and a Welford mean and M2 -- where the simulation ran (torch on the device, else
    NumPy); the replicated correlograms themselves are never stacked.  pvalue("xcorr"), xcorr_mean and xcorr_std read them.

    isi = D >= 2 adds the statistics of the single spike train, the ones that see refractoriness and bursting: "isi", the inter-spike-interval
    density (N, D) (isi_host; the last bin holds the intervals of D bins or more), and "cv", the coefficient of variation of the intervals
    (N,).  observed["isi"] and observed["cv"] are the data's (model.isi_histogram); collect() keeps the cv per replicate, as the Fano factor,
    and streams the density per cell by the rule of the correlogram, on the host ((N, D) is small).  pvalue("isi"), pvalue("cv"), isi_mean,
    isi_std, cvs and cv_quantiles(q) read them."""

    def __init__(self, model, replicates=8, seed=0, data=0, gpu=None, lags=0, isi=0, covariates=None, latents=None):
        self.model, self.R, self.seed, self.gpu = model, int(replicates), int(seed), gpu
        # a model with covariates or latents (model.predictive_check checks them): what every collect() hands to model.simulate()
        self._drive_kw = {} if covariates is None and latents is None else dict(covariates=covariates, latents=latents, data=data)
        self.D = check_isi_bins(isi)
        Y = np.asarray(model.data_list[data][1], dtype=np.float64)
        self.T = Y.shape[0]
        self.K = check_lags(lags, self.T)
        self.observed = {"rate": Y.mean(axis=0), "fano": fano_factor(Y.sum(axis=0), (Y * Y).sum(axis=0), self.T)}
        if self.K:
            self.observed["xcorr"] = model.cross_correlogram(data=data, lags=self.K, gpu=gpu)
        if self.D:
            hist, moments = model.isi_histogram(data=data, bins=self.D, gpu=gpu)
            self.observed["isi"], self.observed["cv"] = isi_density(hist, moments), isi_cv(moments)
        self.calls = 0
        self._rate, self._fano, self._cv = [], [], []
        self._isi = None                         # [ge, le, n, mean, M2], each (N, D), NumPy
        self._xc = None                          # [obs, ge, le, n, mean, M2], each (K, N, N), on the device of the simulations or in NumPy

    def collect(self):
        sim = self.model.simulate(self.T, replicates=self.R, seed=self.seed, first_replicate=self.calls * self.R, keep_paths=False, gpu=self.gpu,
                                  lags=self.K, lagged_on_device=True, isi=self.D, **self._drive_kw)
        self.calls += 1
        self._rate.append(sim.rate())
        self._fano.append(sim.fano())
        if self.K:
            self._collect_xcorr(sim)
        if self.D:
            self._cv.append(sim.isi_cv())
            self._collect_isi(sim)

    def _collect_isi(self, sim):
        obs = self.observed["isi"]
        if self._isi is None:
            self._isi = [np.zeros(obs.shape, dtype=np.int64) for _ in range(3)] + [np.zeros(obs.shape) for _ in range(2)]
        ge, le, n, mean, M2 = self._isi
        dens = sim.isi_density()
        with np.errstate(invalid="ignore"):
            for r in range(dens.shape[0]):       # the rule of _collect_xcorr: one replicate at a time, Welford's order
                c = dens[r]
                ok = ~np.isnan(c)
                ge += ok & (c >= obs)
                le += ok & (c <= obs)
                n += ok
                d = np.where(ok, c - mean, 0.0)
                mean += d / np.maximum(n, 1)
                M2 += d * np.where(ok, c - mean, 0.0)

    def _isi_state(self):
        if not self.D or self._isi is None:
            raise ValueError("the interval statistics need predictive_check(isi=D) with D >= 2 and at least one collect()")
        return self._isi

    @property
    def isi_mean(self):
        """mean of the replicated interval density over the replicates in which it is defined, (N, D); NaN where it never is"""
        _, _, n, mean, _ = self._isi_state()
        return np.where(n > 0, mean, np.nan)

    @property
    def isi_std(self):
        """its standard deviation (n - 1 in the denominator); NaN with fewer than two defined replicates"""
        _, _, n, _, M2 = self._isi_state()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 1, np.sqrt(M2 / (n - 1.0)), np.nan)

    @property
    def cvs(self):
        """(S R, N)"""
        self._isi_state()
        return np.concatenate(self._cv, axis=0)

    def cv_quantiles(self, q):
        """quantiles over the replicates whose coefficient of variation is defined (at least two intervals)"""
        return np.nanquantile(self.cvs, q, axis=0)

    def _collect_xcorr(self, sim):
        S = sim.lagged
        if isinstance(S, np.ndarray):
            xp, s, ss = np, sim.sum, sim.sumsq
            zeros = lambda dtype: np.zeros(S.shape[1:], dtype=dtype)
            obs = self.observed["xcorr"]
            i64, f64 = np.int64, np.float64
        else:
            import torch
            xp = torch
            s, ss = torch.from_numpy(sim.sum).to(S.device), torch.from_numpy(sim.sumsq).to(S.device)
            zeros = lambda dtype: torch.zeros(S.shape[1:], dtype=dtype, device=S.device)
            obs = torch.from_numpy(self.observed["xcorr"]).to(S.device)
            i64, f64 = torch.int64, torch.float64
        if self._xc is None:
            self._xc = [obs, zeros(i64), zeros(i64), zeros(i64), zeros(f64), zeros(f64)]
        obs, ge, le, n, mean, M2 = self._xc
        for r in range(S.shape[0]):              # one replicate at a time: (K, N, N) temporaries, and Welford's order
            c = correlogram(S[r], s[r], ss[r], self.T)
            ok = ~xp.isnan(c)
            ge += ok & (c >= obs)
            le += ok & (c <= obs)
            n += ok
            d = xp.where(ok, c - mean, xp.zeros_like(c))
            mean += d / xp.maximum(n, xp.ones_like(n))
            M2 += d * xp.where(ok, c - mean, xp.zeros_like(c))

    def _xcorr_state(self):
        if not self.K or self._xc is None:
            raise ValueError("the cross-correlogram needs predictive_check(lags=K) with K > 0 and at least one collect()")
        return [v if isinstance(v, np.ndarray) else v.cpu().numpy() for v in self._xc]

    @property
    def xcorr_mean(self):
        """mean of the replicated correlogram over the replicates in which the cell is defined, (K, N, N); NaN where it never is"""
        _, _, _, n, mean, _ = self._xcorr_state()
        return np.where(n > 0, mean, np.nan)

    @property
    def xcorr_std(self):
        """its standard deviation (n - 1 in the denominator); NaN with fewer than two defined replicates"""
        _, _, _, n, _, M2 = self._xcorr_state()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 1, np.sqrt(M2 / (n - 1.0)), np.nan)

    @property
    def rates(self):
        """(S R, N)"""
        return np.concatenate(self._rate, axis=0)

    @property
    def fanos(self):
        return np.concatenate(self._fano, axis=0)

    def rate_quantiles(self, q):
        return np.quantile(self.rates, q, axis=0)

    def fano_quantiles(self, q):
        """quantiles over the replicates whose Fano factor is defined (a silent replicate has none)"""
        return np.nanquantile(self.fanos, q, axis=0)

    def pvalue(self, stat="rate"):
        """two-sided posterior predictive p-value of the observed statistic per neuron, (N,): with M replicated values (those that are
        defined), p = min(1, 2 min(1 + #{rep >= obs}, 1 + #{rep <= obs}) / (M + 1)) -- the smallest attainable value is 2 / (M + 1).
        NaN where the observed statistic is undefined."""
        if stat == "xcorr":                      # the same rule per cell (K, N, N), from the streamed counts
            obs, ge, le, M, _, _ = self._xcorr_state()
            p = np.minimum(1.0, 2.0 * np.minimum(1 + ge, 1 + le) / (M + 1.0))
            return np.where(np.isnan(obs), np.nan, p)
        if stat == "isi":                        # and per cell (N, D)
            ge, le, M, _, _ = self._isi_state()
            p = np.minimum(1.0, 2.0 * np.minimum(1 + ge, 1 + le) / (M + 1.0))
            return np.where(np.isnan(self.observed["isi"]), np.nan, p)
        if stat not in ("rate", "fano", "cv"):
            raise ValueError("pvalue(): stat is 'rate', 'fano', 'xcorr', 'isi' or 'cv'")
        rep = self.rates if stat == "rate" else self.fanos if stat == "fano" else self.cvs
        obs = self.observed[stat]
        ok = ~np.isnan(rep)
        M = ok.sum(axis=0)
        with np.errstate(invalid="ignore"):
            ge = (ok & (rep >= obs)).sum(axis=0)
            le = (ok & (rep <= obs)).sum(axis=0)
        p = np.minimum(1.0, 2.0 * np.minimum(1 + ge, 1 + le) / (M + 1.0))
        return np.where(np.isnan(obs), np.nan, p)


# =====================================================================================================================================
# Conditional simulation: model.conditional_simulate() / model.conditional_check().  Some neurons are data, the others are drawn.
PGL_COND_MAX_FREE = _lib.PGL_COND_MAX_FREE  # free neurons at most
COND_MAX_X = 8192               # F * B at most on the device: x_t of a replicate lives in LDS


def check_free(free, N):
    """-> the free neurons as a sorted int64 array; ValueError, naming the offender, for an empty list, more than PGL_COND_MAX_FREE, a
    duplicate or an index outside [0, N)"""
    f = np.asarray(free)
    if f.ndim != 1 or f.size == 0:
        raise ValueError("conditional simulation: `free` is empty; a list of at least one neuron index is required")
    if not np.issubdtype(f.dtype, np.integer):
        raise ValueError("conditional simulation: `free` must hold integer neuron indices, got dtype %s" % f.dtype)
    f = f.astype(np.int64)
    if f.size > PGL_COND_MAX_FREE:
        raise ValueError("conditional simulation: %d free neurons; at most PGL_COND_MAX_FREE = %d can be free" % (f.size, PGL_COND_MAX_FREE))
    bad = f[(f < 0) | (f >= N)]
    if bad.size:
        raise ValueError("conditional simulation: free neuron index %d is outside [0, N = %d)" % (bad[0], N))
    f = np.sort(f)
    dup = f[1:][f[1:] == f[:-1]]
    if dup.size:
        raise ValueError("conditional simulation: neuron %d is listed more than once in `free`" % dup[0])
    return f


def check_window(start, stop, T):
    """-> (start, stop) of a window of a recording of T bins (stop None: T); ValueError unless 0 <= start <= stop <= T"""
    start, stop = int(start), T if stop is None else int(stop)
    if not 0 <= start <= stop <= T:
        raise ValueError("conditional simulation: the window [%d, %d) is not within the recording's bins [0, %d)" % (start, stop, T))
    return start, stop


class ConditionalSimulation(object):
    """what model.conditional_simulate() returns: free (F,), the global indices of the free neurons; Y (R, T', F) float64, the free neurons'
    paths over the window, or None (keep_paths=False); sum and sumsq (R, F), added in time order; history (R, L, F), the last L bins of every
    replicate; base (T', F), the input of the serial law; t0 / t1, the window in the recording's bins; seed and first_replicate; psi (R, T', F)
    where it was asked for."""

    def __init__(self, free, Y, sum, sumsq, history, base, t0, t1, seed, first_replicate, psi=None, recording=None):
        self.free, self.Y, self.sum, self.sumsq, self.history, self.base = np.asarray(free), Y, sum, sumsq, history, base
        self.t0, self.t1, self.seed, self.first_replicate = int(t0), int(t1), int(seed), int(first_replicate)
        self.psi, self._recording = psi, recording

    @property
    def T(self):
        return self.t1 - self.t0

    def rate(self):
        """mean of y per bin, (R, F)"""
        return self.sum / self.T

    def fano(self):
        """variance / mean of y over the bins, (R, F); NaN where the mean is zero"""
        return fano_factor(self.sum, self.sumsq, self.T)

    def paths(self, r):
        """(T', N): the recording's window with the free columns replaced by replicate r"""
        if self.Y is None or self._recording is None:
            raise ValueError("paths(): the paths were not kept (keep_paths=False) or no recording is attached")
        out = np.array(self._recording[self.t0:self.t1], dtype=np.float64)
        out[:, self.free] = self.Y[r]
        return out


def cond_chunk_bins(F, R):
    """bins per launch of pgl_conditional_simulate for F free neurons and R replicates"""
    return int(max(1, min(MAX_CHUNK_BINS, CHUNK_DRAWS // (F * R))))


def conditional_host(Wff, base, basis, kind, par, neuron, R, seed, rep0, hist, t0, keep_paths, want_psi=False):
    """THE CONDITIONAL LAW in NumPy (the header comment of pgl_conditional_simulate in pyglm_amd/csrc/pgl_generate.hip refers to this; the
    kernel and this function are two separately written implementations and are tested against each other).

    Inputs: data set i of a model with recording Y (T, N) and regressors X (T, N, B) as add_data stored them; the model's current state; a
    sorted list `free` of F distinct neuron indices n_0 < ... < n_{F-1}, every other neuron being clamped to the recording; a window
    [start, stop) of the recording's bins.
      Wm          = (a*W).reshape(N, N*B), the activation of `means` and simulate()
      base[t, j]  = bias[n_j] + sum_{m clamped} sum_b Wm[n_j, m*B + b] X[t, m, b]   for t in the window: engine.psi on the current state with the
                    free COLUMNS of the adjacency set to zero, columns `free` of the result (gathered as `means` gathers on a sharded model).
                    base is an INPUT of the serial law: this function and the kernel receive the same array (T', F), row 0 = bin t0 = start
      Wff[j, k*B + b] = Wm[n_j, n_k*B + b]                                            the free block, (F, F*B)
      x_r[t][k, b]    = sum_l y_r[t-1-l, n_k] basis[l, b]
      psi_r[t, j]     = base[t, j] + Wff[j, :] . x_r[t]
      y_r[t, n_j]     ~ neuron n_j's own model at psi_r[t, j], by host_draw / sim_draw exactly as in THE LAW of simulate: kind / par (F,) are
                    those of the free neurons
      history     the free neurons' bins before `start` are the recording's own rows Y[start-L:start, free], silence before bin 0 (the
                    convention of convolve_with_basis): hist (R, L, F) in time order
      stream      that of simulate: PURPOSE_SIM, stream = (replicate << 32) | n_j with the GLOBAL neuron index, element = the bin's index in the
                    recording, call 0.  A free neuron sees the uniforms it sees in simulate(seed, replicate); path r depends on (seed, r, state,
                    recording, free, window) and not on R or on the chunking
    With every neuron free and start = 0, base is the bias and this is simulate_host from silence: the array expressions below are that
    function's, so the bits are too.
    -> ConditionalSimulation (free = `neuron`); want_psi: True keeps psi (R, T', F); a callable f(psi_block (R, n, F), k0) is fed the
    activations of bins k0 .. k0 + n - 1 of the window block by block instead"""
    Wff = np.ascontiguousarray(Wff, dtype=np.float64)
    F = Wff.shape[0]
    L, B = basis.shape
    WffT = np.ascontiguousarray(Wff.T)
    base = np.asarray(base, dtype=np.float64)
    T = base.shape[0]
    C = T if keep_paths else min(T, HOST_BLOCK_BINS)
    buf = np.zeros((R, L + C, F))
    buf[:, :L] = hist
    s, ss = np.zeros((R, F)), np.zeros((R, F))
    fold = want_psi if callable(want_psi) else None
    P = np.empty((R, T if want_psi is True else C, F)) if want_psi else None
    neurons, reps = np.asarray(neuron, dtype=np.int64), rep0 + np.arange(R)
    pos, k0 = L, 0                                   # buf[:, pos] receives bin t; k0: the window row of buf[:, L]
    for t in range(t0, t0 + T):
        if pos == L + C:
            if fold:
                fold(P, k0)
            buf[:, :L] = buf[:, C:].copy()
            pos, k0 = L, t - t0
        x = np.einsum("rlm,lb->rmb", buf[:, pos - L:pos][:, ::-1], basis)
        psi = x.reshape(R, F * B).dot(WffT) + base[t - t0]
        u1, u2 = sim_uniforms(seed, t, neurons, reps)
        y, capped = host_draw(kind, par, psi, u1, u2)
        if capped is not None:
            _raise_cap(t, rep0 + capped[0], int(neurons[capped[1]]))
        buf[:, pos] = y
        if want_psi:
            P[:, t - t0 if want_psi is True else pos - L] = psi
        s += y
        ss += y * y
        pos += 1
    if fold and pos > L:
        fold(P[:, :pos - L], k0)
    return ConditionalSimulation(neurons, buf[:, L:L + T].copy() if keep_paths else None, s, ss, buf[:, pos - L:pos].copy(), base, t0, t0 + T,
                                 seed, rep0, psi=P if want_psi is True else None)


def conditional_device(Wff, base, basis, kind, par, neuron, R, seed, rep0, hist, t0, keep_paths, device=None, chunk=None, want_psi=False):
    """THE CONDITIONAL LAW through pgl_conditional_simulate, a chunk of bins per launch (chunk: its length, default cond_chunk_bins)
    -> ConditionalSimulation.  A callable want_psi is fed device tensors."""
    import torch
    dev, st = _device("conditional_simulate", device)
    F = np.shape(Wff)[0]
    L, B = np.shape(basis)
    T = np.shape(base)[0]
    if F * B > COND_MAX_X:
        raise ValueError("conditional_simulate(): %d free neurons x %d basis functions = %d; the device path holds at most %d" % (F, B, F * B, COND_MAX_X))
    Tc = min(T, int(chunk) if chunk else cond_chunk_bins(F, R))
    fold = want_psi if callable(want_psi) else None
    with torch.cuda.device(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        need = 8 * F * (T + R * T * bool(keep_paths) + R * (T if want_psi is True else Tc if want_psi else 0))
        free = torch.cuda.mem_get_info(dev)[0]
        if need > free:
            raise PglError("conditional_simulate(): base, the paths and the activations of %d replicates x %d bins x %d free neurons need %d bytes "
                           "of device memory, %d are free: simulate fewer replicates or bins per call, or pass keep_paths=False" % (R, T, F, need, free))
        Wff_d, base_d, basis_d = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev) for v in (Wff, base, basis))
        kind_d = torch.from_numpy(np.ascontiguousarray(kind, dtype=np.int32)).to(dev)
        par_d = torch.from_numpy(np.ascontiguousarray(par, dtype=np.float64)).to(dev)
        neuron_d = torch.from_numpy(np.ascontiguousarray(neuron, dtype=np.int32)).to(dev)
        rows = (t0 - L + np.arange(L)) % L               # ring row t mod L = Y[t]
        ring_h = np.empty((R, L, F))
        ring_h[:, rows] = hist
        ring = torch.from_numpy(ring_h).to(dev)
        Y_d = torch.empty((R, T, F), **f64) if keep_paths else None
        P_d = torch.empty((R, T if want_psi is True else Tc, F), **f64) if want_psi else None
        sum_d, sq_d = torch.zeros((R, F), **f64), torch.zeros((R, F), **f64)
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        status_h = torch.zeros(4, dtype=torch.int32).pin_memory()
        for k0 in range(0, T, Tc):
            n = min(Tc, T - k0)
            yout, ldr = (Y_d[0, k0:], T * F) if keep_paths else (None, 0)
            pout, ldp = (P_d[0, k0:], T * F) if want_psi is True else (P_d, Tc * F) if want_psi else (None, 0)
            call("pgl_conditional_simulate", Wff=ptr(Wff_d), base=ptr(base_d[k0:]), ldb=F, basis=ptr(basis_d), F=F, B=B, L=L, kind=ptr(kind_d),
                 par=ptr(par_d), neuron=ptr(neuron_d), R=R, rep0=rep0, seed=seed & (2 ** 64 - 1), ring=ptr(ring), Y=ptr(yout), ldr=ldr,
                 Psi=ptr(pout), ldp=ldp, sum=ptr(sum_d), sumsq=ptr(sq_d), t0=t0 + k0, Tc=n, status=ptr(status), hip_stream=st)
            _finish_launch("pgl_conditional_simulate", dev, status, status_h, t0 + k0, t0 + k0 + n - 1)
            if fold:
                fold(P_d[:, :n], k0)
        rows = (t0 + T - L + np.arange(L)) % L
        return ConditionalSimulation(np.asarray(neuron, dtype=np.int64), Y_d.cpu().numpy() if keep_paths else None, sum_d.cpu().numpy(),
                                     sq_d.cpu().numpy(), ring.cpu().numpy()[:, rows], np.asarray(base, dtype=np.float64), t0, t0 + T, seed, rep0,
                                     psi=P_d.cpu().numpy() if want_psi is True else None)


def conditional_simulate(Wff, base, basis, kind, par, neuron, R, seed, rep0, hist, t0, keep_paths, on_device, device, chunk=None, want_psi=False):
    """R replicates of the free neurons `neuron` (F,) over the T' = len(base) bins from t0 under THE CONDITIONAL LAW (conditional_host states
    it) -> ConditionalSimulation; on the device (pgl_conditional_simulate) or in NumPy.  What model.conditional_simulate() calls once it has
    read the model: Wff (F, F*B), base (T', F), basis (L, B), kind / par (F,) of the free neurons, hist (R, L, F) or (L, F), their L bins
    before t0 in time order."""
    Wff, base, basis = (np.asarray(v, dtype=np.float64) for v in (Wff, base, basis))
    neuron = np.asarray(neuron, dtype=np.int64)
    F, (L, B) = neuron.size, basis.shape
    R, rep0, seed, t0 = int(R), int(rep0), int(seed), int(t0)
    if not 1 <= F <= PGL_COND_MAX_FREE or Wff.shape != (F, F * B) or base.ndim != 2 or base.shape[1] != F:
        raise ValueError("conditional_simulate(): 1 <= F <= %d free neurons, Wff (F, F*B) and base (T', F) are required, got F = %d, Wff %r, base %r"
                         % (PGL_COND_MAX_FREE, F, Wff.shape, base.shape))
    if R < 1 or rep0 < 0 or t0 < 0 or not 0 <= seed < 2 ** 64:
        raise ValueError("conditional_simulate(): replicates >= 1, first_replicate >= 0, t0 >= 0 and 0 <= seed < 2^64 are required")
    T = base.shape[0]
    if t0 + T >= 2 ** 31 or rep0 + R >= 2 ** 31 or (neuron.size and neuron.max() >= 2 ** 31):
        raise ValueError("conditional_simulate(): time bins, replicate and neuron indices must stay below 2^31")
    kind, par = np.asarray(kind, dtype=np.int32), np.asarray(par, dtype=np.float64)
    hist = np.array(np.broadcast_to(np.asarray(hist, dtype=np.float64), (R, L, F)))
    if T == 0:
        return ConditionalSimulation(neuron, np.zeros((R, 0, F)) if keep_paths else None, np.zeros((R, F)), np.zeros((R, F)), hist, base, t0, t0,
                                     seed, rep0, psi=np.zeros((R, 0, F)) if want_psi is True else None)
    if on_device:
        return conditional_device(Wff, base, basis, kind, par, neuron, R, seed, rep0, hist, t0, keep_paths, device=device, chunk=chunk, want_psi=want_psi)
    return conditional_host(Wff, base, basis, kind, par, neuron, R, seed, rep0, hist, t0, keep_paths, want_psi=want_psi)


class ConditionalPrediction(object):
    """Population-conditioned prediction of the free neurons of one data set (model.conditional_check()), in the pattern of PredictiveCheck:

        cp = model.conditional_check(free=[3, 7], replicates=8, seed=0)
        for it in range(n_sweeps):
            model.resample_model()
            if it >= burn:
                cp.collect()
        cp.rate_mean, cp.rate_std, cp.log_score()

    collect() simulates `replicates` fresh conditional replicates over the window from the model's current state (the k-th call uses replicate
    indices k R ... k R + R - 1) and folds, per cell (t, j) of the window and one replicate after the other, a Welford mean / M2 of the rate
    E[y | psi_r[t, j]] -- by the neuron's own link, as regression.means_of_psi -- and a streaming log-sum-exp (m, s), as in summary.py, of
    l_r = log p(Y[t, n_j] | psi_r[t, j]): logC + a psi - b log1p(e^psi) with the terms of regression.obs_terms for the Polya-gamma models,
    -1/2 log(2 pi eta) - (y - psi)^2 / (2 eta) for Gaussian neurons.  The accumulators live where the simulation ran: torch tensors on the
    device, folded elementwise from every launch's activations, else NumPy.  It changes nothing in the chain."""

    def __init__(self, model, free, replicates=8, seed=0, data=0, start=0, stop=None, gpu=None):
        self.model, self.R, self.seed, self.gpu = model, int(replicates), int(seed), gpu
        self.data = range(len(model.data_list))[data]
        Y = np.asarray(model.data_list[self.data][1], dtype=np.float64)
        self.free = check_free(free, model.N)
        self.t0, self.t1 = check_window(start, stop, Y.shape[0])
        if self.R < 1:
            raise ValueError("conditional_check(): replicates >= 1 is required")
        self._Yw = Y[self.t0:self.t1][:, self.free]
        self._read_par()
        self.calls = self.count = 0
        self._acc = None                         # [rate mean, rate M2, lse m, lse s], each (T', F), where the simulations run
        self._consts = None                      # link masks, parameters and the terms of l, on the accumulators' side

    def _read_par(self):
        """the links' parameters and the terms of l from the free neurons' regressions as they are now: once, in the constructor -- and again
        before every sample of a model that learns xi, whose b(y) = y + xi and log c(y) move with the chain"""
        regs = [self.model.regressions[n] for n in self.free]
        models = observation_models(regs)
        self._link = np.array([m.link for m in models], dtype=np.int64)
        self._link_par = np.array([m.par(r) for m, r in zip(models, regs)], dtype=np.float64)
        self._gauss = models[0].sim_kind == KIND_GAUSSIAN
        if self._gauss:
            self._terms = (self._Yw, np.array([float(r.eta) for r in regs]))
        else:
            self._terms = _reg.obs_terms(regs, self._Yw)

    def _setup(self, like):
        shape = (self.t1 - self.t0, self.free.size)
        if isinstance(like, np.ndarray):
            conv, zeros = (lambda v: np.asarray(v)), (lambda: np.zeros(shape))
        else:
            import torch
            conv, zeros = (lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(like.device)), (lambda: torch.zeros(shape, dtype=torch.float64, device=like.device))
        self._conv = conv
        self._acc = [zeros() for _ in range(4)]
        self._put_consts()

    def _put_consts(self):
        conv = self._conv
        self._consts = dict(link=[conv(self._link == c) for c in range(4)], par=conv(self._link_par), terms=tuple(conv(v) for v in self._terms))

    def _fold(self, psi, k0):
        """psi (R, n, F): the activations of window rows k0 .. k0 + n - 1 of this call's R replicates"""
        xp = np
        if not isinstance(psi, np.ndarray):
            import torch
            xp = torch
        if self._acc is None:
            self._setup(psi)
        n = psi.shape[1]
        mean, M2, lm, ls = (v[k0:k0 + n] for v in self._acc)
        link, par = self._consts["link"], self._consts["par"]
        terms = tuple(v[k0:k0 + n] if v.ndim == 2 else v for v in self._consts["terms"])
        for r in range(psi.shape[0]):            # one replicate at a time: Welford's order
            p = psi[r]
            k = self.count + r + 1
            lg = 1.0 / (1.0 + xp.exp(-p))
            rate = xp.where(link[0], lg, xp.where(link[1], p, xp.where(link[2], par * xp.exp(p), par * lg)))
            d = rate - mean
            mean += d / k
            M2 += d * (rate - mean)
            if self._gauss:
                y, eta = terms
                l = -0.5 * xp.log(2 * np.pi * eta) - (y - p) ** 2 / (2 * eta)
            else:
                A, Bv, logC = terms
                l = logC + A * p - Bv * xp.log1p(xp.exp(p))
            if k == 1:
                lm[...] = l
                ls[...] = 1.0
            else:
                m1 = xp.maximum(lm, l)
                ls[...] = ls * xp.exp(lm - m1) + xp.exp(l - m1)
                lm[...] = m1

    def collect(self):
        if self.model._learns_xi():
            self._read_par()
            if self._acc is not None:
                self._put_consts()
        inp = self.model._conditional_inputs(self.free, self.data, self.t0, self.t1)
        conditional_simulate(inp["Wff"], inp["base"], inp["basis"], inp["kind"], inp["par"], self.free, self.R, self.seed, self.calls * self.R,
                             inp["hist"], self.t0, False, self.model._on_gpu(self.gpu, "conditional_check"), self.model._device, want_psi=self._fold)
        self.calls += 1
        self.count += self.R

    def _state(self):
        if self._acc is None:
            raise ValueError("conditional_check(): the read-outs need at least one collect()")
        return [v if isinstance(v, np.ndarray) else v.cpu().numpy() for v in self._acc]

    @property
    def rate_mean(self):
        """mean over the S R replicates folded so far of E[y | psi_r], (T', F)"""
        return self._state()[0].copy()

    @property
    def rate_std(self):
        """its standard deviation, sqrt(M2 / (S R)), (T', F)"""
        return np.sqrt(self._state()[1] / self.count)

    def log_score(self):
        """the conditional log predictive score of the recording: dict(total, per_neuron (F,), per_bin (T', F)), per_bin = logsumexp_r l_r -
        log(S R)"""
        _, _, lm, ls = self._state()
        per_bin = lm + np.log(ls) - np.log(self.count)
        return dict(total=float(per_bin.sum()), per_neuron=per_bin.sum(axis=0), per_bin=per_bin)
