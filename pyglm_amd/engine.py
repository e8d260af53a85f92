"""Device-side state and sweep orchestration for one shard of postsynaptic neurons on one MI355X.

The reference runs `for n in range(N): regressions[n].resample(...)` in Python (pyglm/models.py:169-171); here the
shard's neurons go through the HIP kernels in batches: one activation contraction + one PG/log-likelihood pass for
the whole shard, then per batch the omega-weighted Gram, posterior assembly, tableau flips and the Gaussian draw.
PyTorch is used for device memory and streams only; all arithmetic is in libpyglm_hip.so (include/pyglm_hip.h).
"""
import ctypes
import functools
import time
import types
import typing

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr
from .regression import MODELS, OBS_NEGBIN, OBS_GAUSSIAN, OBS_BINOMIAL, OBS_HOOKS

F64 = torch.float64
I32 = torch.int32


def _r(x, m):
    return (x + m - 1) // m * m


def _on_device(fn):
    """run a GibbsEngine method with the engine's GPU as the current device and put the caller's device back afterwards: the library's
    launches act on the current HIP device, and an engine must not move its process onto its own device behind the caller's back (a
    temporary engine on another GPU, several engines in one process)"""
    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        with torch.cuda.device(self.dev):
            return fn(self, *args, **kwargs)
    return wrapped


class _StepScratch(object):
    """THE rule of the scratch of the Gibbs steps beside the sweep (dispersion, covariates, latents): owned by the step object, allocated at
    its first call behind the memory gate (_alloc(T, eng) -> dict, after eng.reserve), kept, allocated again when the longest data set grew"""

    def __init__(self, eng):
        self.eng, self.dev, self.scratch, self.T = eng, eng.dev, None, -1

    def _scratch(self):
        T = max([ds.T for ds in self.eng.datasets] or [0])
        if self.scratch is None or self.T < T:
            self.scratch = None                       # (released first; a refusal at the gate leaves none, and the next call asks again)
            self.scratch, self.T = types.SimpleNamespace(**self._alloc(T, self.eng)), T
        return self.scratch


def make_draws(seed, sweep, neuron_ids, N, D):
    """Host random inputs of the non-PG steps, keyed by (seed, sweep, GLOBAL neuron) so that results do not depend on
    how neurons are sharded: perm = permutation(N) (regression.py:286), u = N uniforms (:315), z = D+1 normals (:334,
    the first sum(a)*B+1 are used)."""
    nloc = len(neuron_ids)
    perm = np.empty((nloc, N), dtype=np.int32)
    u = np.empty((nloc, N))
    z = np.empty((nloc, D + 1))
    for i, n in enumerate(neuron_ids):
        rng = np.random.Generator(np.random.Philox(key=int(seed) & (2 ** 64 - 1), counter=[int(sweep), int(n), 0, 0]))
        perm[i] = rng.permutation(N)
        u[i] = rng.random(N)
        z[i] = rng.standard_normal(D + 1)
    return perm, u, z


def make_gamma_draws(seed, sweep, neuron_ids, alpha, lane=1):
    """standard Gamma(alpha, 1) variates for the noise-variance update of the Gaussian model (regression.py:433-445), keyed like
    make_draws by (seed, sweep, GLOBAL neuron) on a separate counter lane: 1, the noise variance eta; 2, the negative-binomial dispersion
    xi (dispersion.XI_LANE)"""
    g = np.empty(len(neuron_ids))
    for i, n in enumerate(neuron_ids):
        rng = np.random.Generator(np.random.Philox(key=int(seed) & (2 ** 64 - 1), counter=[int(sweep), int(n), int(lane), 0]))
        g[i] = rng.standard_gamma(alpha)
    return g


def prior_terms(S_w, mu_w, S_b, mu_b):
    """natural parameters (regression.py:138-151) + the per-block prior constant of the collapsed flips.
    S_w (n,N,B,B), mu_w (n,N,B), S_b (n,), mu_b (n,)  ->  Jw, hw, Jb, hb, c0 (n,N)."""
    Jw = np.linalg.inv(S_w)
    hw = np.einsum("nmij,nmj->nmi", Jw, mu_w)
    Jb = 1.0 / S_b
    hb = Jb * mu_b
    _, logdet = np.linalg.slogdet(Jw)
    c0 = 0.5 * logdet - 0.5 * np.einsum("nmi,nmi->nm", mu_w, hw)
    return Jw, hw, Jb, hb, c0


class BlockPrior(object):
    """block-diagonal weight prior of a shard in table form: the K distinct (J_w, h_w, c0) blocks and, per (local neuron, presynaptic
    neuron), the index of its block.  A network prior pushes two or three distinct blocks for N^2 pairs; the tables travel to the
    GPU instead of the expanded (nloc, N, B, B) array.  Accepted by GibbsEngine.sweep in place of the dense Jw (hw and c0 = None)."""

    def __init__(self, Jw_u, hw_u, c0_u, label):
        self.Jw_u = np.ascontiguousarray(Jw_u, dtype=np.float64)
        self.hw_u = np.ascontiguousarray(hw_u, dtype=np.float64)
        self.c0_u = np.ascontiguousarray(c0_u, dtype=np.float64)
        self.label = np.ascontiguousarray(label, dtype=np.int32)

    def dense(self):
        return self.Jw_u[self.label], self.hw_u[self.label], self.c0_u[self.label]


class _Dataset(object):
    # what add_data leaves unset on a data set without the integer Gram, without hooks or without covariates
    int8, planes, sA, PA, xmax, hooks, S, Off = False, 0, None, None, None, None, None, None


class _I8Scratch(typing.NamedTuple):
    """the integer Gram's scratch (GibbsEngine._i8_reserve)"""
    bytes: int                           # held by the buffers below
    T: int                               # the longest data set it is sized for
    G: int                               # neurons per product launch (pgl_sweep_t.i8_group)
    PB: torch.Tensor                     # planes of omega_g X (of one time slice)
    R: torch.Tensor                      # residues of a group
    stat: torch.Tensor                   # (3, G, D) per group: column maxima, sums of squares, scales of omega_g X
    slice: int                           # time bins per slice (pgl_sweep_t.i8_slice; 0: the whole data set at once)
    PAs: typing.Optional[torch.Tensor]   # planes of one slice of X where X's own are not resident
    Rx: typing.Optional[torch.Tensor]    # the three extra residue slots per neuron of the K-quarter split of the last plane (groups that
    #                                      fill the per-XCD lists: multiples of 8)


class GibbsEngine(object):
    # observation models (include/pyglm_hip.h, pgl_pg_loglik_ex): the built-in Bernoulli, negative-binomial, Gaussian and binomial regressions,
    # and "hooks" -- any other Polya-gamma model, its a(y), b(y), log c(y) evaluated on the host and kept next to the data (add_data obs_terms)
    OBS = dict([(m.name, m.device) for m in MODELS.values()] + [("hooks", OBS_HOOKS)])
    _LINK = dict([(m.device, m.link) for m in MODELS.values()] + [(OBS_HOOKS, 0)])     # link0 of pgl_summary_fold (hooks: per neuron, summary.py)

    def __init__(self, N, B, n0=0, n1=None, device=None, obs="bernoulli", xi=1.0, batch=None, mem_budget_bytes=None,
                 design_only=False, visit_order=True, gram=None, likelihood_only=False, planes=None, i8_group=None, i8_slice=None,
                 i8_resident=None, device_share=1, n_covariates=0, covariate_prior=None, n_latents=0, latent_ar=None):
        """device: torch device of this shard (default: the process's current GPU).  design_only: only the design matrix is kept (basis
        convolution).  likelihood_only: activation / log-likelihood / means only -- no sweep buffers, no residue planes (a held-out data
        set costs X', Y and Psi, nothing else).  i8_group / i8_slice / i8_resident: override the integer Gram's plan (_i8_plan) -- neurons
        per product launch, time bins per slice, X's planes kept (True) or converted per slice (False); tests and probes.  device_share: number of
        engines (ranks) that share this GPU -- each then stays inside an equal share of its memory (bench.py's one-GPU dry run of N ranks).
        xi: the negative-binomial xi (obs "negbin") or the binomial number of trials n (obs "binomial"): a scalar, or one value per neuron
        of the model (N) or of this shard (n1 - n0).  n_covariates = K > 0: every data set carries covariates S (T, K) and an offset
        Off = S beta' on the device (pyglm_amd/covariates.py); covariate_prior = (mu0, Sigma0) of beta_n, default (0, I).  n_latents = Q > 0
        (pyglm_amd/latents.py): Q further columns of S whose values are sampled (latents._DeviceStep) -- K becomes n_covariates + Q, S
        is [S_obs | X] with X zero at add_data, and covariate_prior is the prior of all K weights (latents.joint_prior).  latent_ar =
        phi (a scalar or Q values in [0, 1)): the latents' AR(1) prior -- where some phi_q > 0 the latent step draws a data set's X
        jointly (pgl_latent_ar_draw); None or all zeros: the independent bins of pgl_latent_draw, launch for launch."""
        from . import covariates as _cov
        from . import latents as _lat
        self.K_obs = _cov.check_count(n_covariates)
        self.Q = _lat.check_count(n_latents, self.K_obs)
        self.K = self.K_obs + self.Q
        self.latent_ar = _lat.check_ar(latent_ar, self.Q)
        self.cov_prior = _cov.prior_terms(self.K, covariate_prior) if self.K else None
        if not torch.cuda.is_available():
            raise _lib.PglError("pyglm_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        _lib.load()
        self.N, self.B, self.D = int(N), int(B), int(N) * int(B)
        self.n0, self.n1 = int(n0), int(N if n1 is None else n1)
        self.nloc = self.n1 - self.n0
        assert 0 <= self.n0 < self.n1 <= self.N
        self.dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(self.dev):
            self._i8_over = dict(group=i8_group, slice=i8_slice, resident=i8_resident)
            self._device_share = max(1, int(device_share))
            self._init(N, B, obs, xi, batch, mem_budget_bytes, design_only, visit_order, gram, likelihood_only, planes)

    def _init(self, N, B, obs, xi, batch, mem_budget_bytes, design_only, visit_order, gram, likelihood_only, planes):
        self.obs = self.OBS[obs]
        self.xi, self.obs_param = self._obs_param(xi)
        self.Dp = _r(self.D + 1, 16)
        self.ldn = _r(self.nloc, 2)
        self.ldj = _r(self.D + 2, 16)
        self.kmax = _lib.load().pgl_flip_kmax()
        self.R = _lib.load().pgl_flip_window_blocks(self.B)
        if self.R < 1:
            raise ValueError("B=%d too large for the proposal window" % self.B)
        self.datasets = []
        # the likelihood Gram X'OX: "fp64" = the fp64-MFMA kernel; "int8" = exact integer arithmetic on the int8 MFMA (residue planes +
        # CRT, pgl_i8_*; operands rounded to integers scaled from their column norms -- measured error several times below the fp64
        # kernel's own); "auto" (default) takes the integer path per data set where it is the faster one and its
        # planes -- whole or in time slices -- fit in memory (_i8_plan)
        self.gram = gram or "auto"
        assert self.gram in ("auto", "fp64", "int8")
        # number of residue planes (moduli) of the integer path: an int, or None = pgl_i8_min_planes (13: integer column norms of 2^50,
        # measured error several times below the fp64 kernel's own); every further plane buys 4 more bits
        self.planes = int(planes) if planes else None
        assert self.planes is None or 1 <= self.planes <= _lib.load().pgl_i8_max_planes()
        self._i8_scratch = None
        # sweep tableau kept in proposal order (updates after a window touch only the rows not yet proposed); False keeps J's order and
        # full-tableau updates -- same decisions, and the final tableau is then the complete sweep(A, S) (used by a full-size test)
        self.visit_order = bool(visit_order)
        # the compacted active block of the weight draw overlays the tableau, which is dead once a batch's flips are done (kept apart
        # with visit_order=False, where tests read the final tableau): two (D+2)^2 buffers per neuron instead of three
        self.share_tableau = self.visit_order
        # neurons per batch: given, or chosen when the first data set is in place (_ensure_batch) -- what is left of the GPU then has to hold
        # the batch's posterior systems AND, on the integer Gram path, the residue planes
        self._batch_arg, self._mem_budget = batch, mem_budget_bytes
        self.nb = None
        self.design_only = design_only
        self.likelihood_only = bool(likelihood_only)
        if likelihood_only:
            self._alloc_shard()
        elif not design_only:
            self._alloc_shard()
            if batch is not None:
                self._ensure_batch()
        self.flip_single_pass = False   # True: one pass over the trailing tableau per proposal window instead of per pair (same bits; tests)
        self.keep_logodds = False       # True: sweep() leaves the flip log-odds in self.logodds (parity tests)
        self.logodds = None
        self.profile = False            # True: every stage of pgl_sweep is timed with HIP events; a collection of stage names: only those
        self._times = None              # pgl_stage_times_t filled by pgl_sweep while `profile` is on
        self._i8_norm = None            # integer Gram: per-batch sums of squares of the columns of omega_n X + the largest omega per neuron
        self._ev = []
        # host-side accounting of sweep(): seconds blocked waiting for the GPU (pgl_get_state) and seconds of host work done while the GPU was
        # busy (host_overlap) -- what a rank's wall time has to be cleared of to see its exposed host share (bench.py: host_busy_ms_per_step)
        self.wait_seconds = 0.0
        self.overlap_seconds = 0.0
        self.launch_seconds = 0.0      # inside the pgl_sweep call itself: ~3 000 launches at the headline size (and, when the queue is full, waiting)
        self._sweep_serial = 0         # sweeps queued so far, and where the last one's perm lies in _din (the chain diagnostics form the
        self._perm_off = None          # conditional edge probabilities from the last sweep's log-odds and proposal order)

    def _obs_param(self, xi):
        """-> (scalar xi, None) or (1.0, [nloc] device array of the shard's per-neuron values), checked: > 0 (negative binomial), >= 0 (binomial)"""
        v = np.asarray(xi, dtype=np.float64)
        if v.ndim == 0:
            vals, out = v.reshape(1), (float(v), None)
        else:
            v = v.reshape(-1)
            if v.size == self.N:
                v = v[self.n0:self.n1]
            elif v.size != self.nloc:
                raise ValueError("xi: %d values for a model of %d neurons (shard of %d)" % (v.size, self.N, self.nloc))
            vals, out = v, (1.0, torch.from_numpy(np.ascontiguousarray(v)).to(self.dev))
        if self.obs == OBS_NEGBIN and not np.all(vals > 0):
            raise ValueError("negative binomial: xi must be > 0")
        if self.obs == OBS_BINOMIAL and not np.all((vals >= 0) & (vals == np.floor(vals))):
            raise ValueError("binomial: the number of trials n must be an integer >= 0")
        return out

    @_on_device
    def set_obs_param(self, xi):
        """overwrite the per-neuron parameter of the observation model (xi, negative binomial; n, binomial) IN PLACE: the device array's
        pointer sits in the once-built pgl_sweep_t and in the accumulators that share it, so it is never reallocated.  xi: one value per
        neuron of the model (N) or of this shard (n1 - n0), checked as at construction.  An engine built from a scalar has no such array
        and raises."""
        if self.obs_param is None:
            raise ValueError("this engine was built with the scalar parameter %r, which its kernels read from their argument blocks: build "
                             "the engine with one value per neuron to change it afterwards" % (self.xi,))
        v = np.asarray(xi, dtype=np.float64)
        if v.ndim == 0:
            v = np.full(self.nloc, float(v))
        _, new = self._obs_param(v)
        self.obs_param.copy_(new)

    # ------------------------------------------------------------------ stage timing (HIP events on the launch stream)
    def _tic(self, name, work=0.0):
        if not self.profile:
            return None
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(self.dev))
        return (name, e0, e1, work)

    def _toc(self, h):
        if h is not None:
            h[2].record(torch.cuda.current_stream(self.dev))
            self._ev.append(h)

    @_on_device
    def collect_timings(self):
        """-> {stage: dict(ms=total, calls=n, work=sum)} since the last call"""
        torch.cuda.synchronize(self.dev)
        out = {}
        for name, e0, e1, work in self._ev:
            d = out.setdefault(name, dict(ms=0.0, calls=0, work=0.0))
            d["ms"] += e0.elapsed_time(e1)
            d["calls"] += 1
            d["work"] += work
        self._ev = []
        if self._times is not None:            # the stages of pgl_sweep (HIP events recorded on the launch stream by the library)
            call("pgl_stage_times_collect", ctypes.byref(self._times))
            lib = _lib.load()
            for i in range(_lib.NSTAGES):
                if self._times.calls[i]:
                    d = out.setdefault(lib.pgl_stage_name(i).decode(), dict(ms=0.0, calls=0, work=0.0))
                    d["ms"] += self._times.ms[i]
                    d["calls"] += self._times.calls[i]
                    d["work"] += self._times.work[i]
            self._times = None
        return out

    # ------------------------------------------------------------------ buffers
    def _z(self, *shape, dtype=F64):
        return torch.zeros(*shape, dtype=dtype, device=self.dev)

    def _free_bytes(self):
        """memory this engine may still take on its GPU.  Ranks that share one device (device_share = their number) each stay inside an
        equal share of it, whatever the others have allocated so far."""
        free, total = torch.cuda.mem_get_info(self.dev)
        share = self._device_share
        if share > 1:
            free = min(free, int(total * 0.94) // share - torch.cuda.memory_reserved(self.dev))
        return max(0, free)

    def _ensure_batch(self):
        if self.nb is not None or self.design_only or self.likelihood_only:
            return
        batch = self._batch_arg
        per_neuron = (2 if self.share_tableau else 3) * self.ldj * self.ldj * 8 + 2 * self.kmax * self.ldj * 8 + 2 * (self.kmax + 1) ** 2 * 8
        if batch is None:
            budget = self._mem_budget if self._mem_budget is not None else int(self._free_bytes() * 0.45)
            batch = max(2, min(self.nloc, budget // per_neuron))
            # equal batches: every batch pays the same latency-bound steps (one workgroup per neuron in the proposal and solve kernels,
            # ~100 panel launches of the Cholesky), so 1024 neurons go as 4 x 256, not as 3 x 295 + 139 -- or, before the overlay, 5 x 204 + 4
            batch = -(-self.nloc // -(-self.nloc // batch))
        self.nb = int(min(batch, self.nloc))
        self._alloc_batch()

    def _alloc_batch(self):
        nb, ldj, N, D, kmax = self.nb, self.ldj, self.N, self.D, self.kmax
        self.Jbuf = self._z(nb, ldj, ldj)
        self.Mtab = self._z(nb, ldj, ldj)
        self.Ac = self.Mtab if self.share_tableau else self._z(nb, ldj, ldj)
        self.hc = self._z(2, nb, ldj)
        self.Tinv = self._z(nb, 64, 64)
        self.G = self._z(nb, kmax, kmax)
        self.Lws = self._z(nb, (kmax + 1) * (kmax + 1))
        self.Ut = self._z(nb, kmax, ldj)
        self.Wt_ws = self._z(nb, kmax, ldj)
        self.d_idx = self._z(nb, kmax, dtype=I32)
        self.d_sign = self._z(nb, kmax)
        self.d_cnt = self._z(nb, dtype=I32)
        self.batch_k = self._z(nb, dtype=I32)
        self.act = self._z(nb, D + 1, dtype=I32)
        self.na = self._z(nb, dtype=I32)

    def _alloc_shard(self):
        """whole-shard state (all a likelihood-only engine needs besides its data)"""
        N, D, nl = self.N, self.D, self.nloc
        # chain state and per-neuron results live at the head of ONE device buffer, the sweep's inputs behind them (_io_reserve): a sweep
        # is one host-to-device copy from a pinned staging buffer instead of a dozen small ones
        self._din = self._hin = self._hout = None
        self._io_reserve(0)
        self.skip = self._z(nl, dtype=I32)
        self._c0_dense = None
        self.Wt = self._z(self.Dp, self.ldn)          # k-major weights for the activation contraction
        self.bias = self._z(nl)
        self.border = self._z(2 * self.ldn, self.Dp)
        if self.K:
            # covariate weights: k-major on the device like the activation's (pgl_covariate_offset), and the host's copy of what is there
            self.beta_dev = self._z(self.K, self.ldn)
            self.beta = np.zeros((nl, self.K))
        if self.obs == OBS_GAUSSIAN:
            # Gaussian observations: omega = 1/eta is constant in t, so X'X is formed once per dataset (add_data) and scaled per sweep
            self.G0 = self._z(self.ldj, self.ldj)
            self.inv_eta = torch.ones(nl, dtype=F64, device=self.dev)
            self.eta = np.ones(nl)

    def _st(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    # ------------------------------------------------------------------ the sweep's I/O block
    def _io_state_layout(self):
        """byte offsets of the state block at the head of the I/O buffer: a (nloc x N int32) | W (nloc x D f64) | b | ll (nloc f64) | status
        (nloc int32) -> (off_a, off_W, off_b, off_ll, off_status, state_bytes), every piece 16-byte aligned"""
        nl, N, D = self.nloc, self.N, self.D
        al = lambda x: (x + 15) // 16 * 16
        off_a = 0
        off_W = al(off_a + 4 * nl * N)
        off_b = al(off_W + 8 * nl * D)
        off_ll = al(off_b + 8 * nl)
        off_st = al(off_ll + 8 * nl)
        return off_a, off_W, off_b, off_ll, off_st, al(off_st + 4 * nl)

    def _io_reserve(self, in_bytes):
        """make the I/O buffer (device) and its pinned staging twin hold the state block + in_bytes of inputs; a_dev / W_dev / b_dev / ll / status
        are views of the device buffer's head (kept across a growth: the state is copied over)"""
        off_a, off_W, off_b, off_ll, off_st, sb = self._io_state_layout()
        need = sb + int(in_bytes)
        if self._din is not None and self._din.numel() >= need:
            return
        cap = max(need, sb + 4096)
        cap = cap + cap // 8                                    # head-room: a prior that changes form between sweeps does not reallocate
        new = torch.zeros(cap, dtype=torch.uint8, device=self.dev)
        if self._din is not None:
            new[:sb].copy_(self._din[:sb])
        self._din = new
        self._stats_dev = None
        self._hin = torch.zeros(cap, dtype=torch.uint8).pin_memory()
        self._hin_np = self._hin.numpy()
        if self._hout is None:
            self._hout = torch.zeros(sb, dtype=torch.uint8).pin_memory()
            self._hout_np = self._hout.numpy()
        nl, N, D = self.nloc, self.N, self.D
        self.a_dev = new[off_a:off_a + 4 * nl * N].view(I32).view(nl, N)
        self.W_dev = new[off_W:off_W + 8 * nl * D].view(F64).view(nl, D)
        self.b_dev = new[off_b:off_b + 8 * nl].view(F64)
        self.ll = new[off_ll:off_ll + 8 * nl].view(F64)
        self.status = new[off_st:off_st + 4 * nl].view(I32)
        self._sweep_cache = None

    # ------------------------------------------------------------------ data
    @_on_device
    def add_data(self, Y, X=None, basis=None, obs_terms=None, covariates=None):
        """models.py:66-80: Y is (T, N) counts; X (T, N, B) optional, else built on the device from `basis` (L, B)
        by pgl_design_matrix (utils/basis.py:5-34).  obs_terms (obs "hooks" only, and required there): (A, Bv, logC), the host arrays
        a(y), b(y), log c(y) of the LOCAL neurons, each (T, n1 - n0) -- kept on the device next to the data set (3 T ldn doubles).
        covariates (an engine with n_covariates = K > 0 only, and required there): S (T, K), kept on the device with the offset
        Off = S beta' (T, ldn), which is formed here from the engine's current beta.  An engine with latents appends their Q zero columns."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        T = Y.shape[0]
        assert Y.shape == (T, self.N)
        from .covariates import check_covariates
        S_cov = check_covariates(covariates, T, 0 if self.design_only else self.K_obs, "add_data")
        if (obs_terms is not None) != (self.obs == OBS_HOOKS) and not self.design_only:
            raise ValueError("obs_terms are the data of the hooks observation model: required with obs='hooks', and only there")
        if obs_terms is not None:
            terms = [np.broadcast_to(np.asarray(v, dtype=np.float64), (T, self.nloc)) for v in obs_terms]
            if len(terms) != 3 or not all(np.all(np.isfinite(v)) for v in terms) or not np.all(terms[1] >= 0):
                raise ValueError("obs_terms: a(y), b(y), log c(y) must be finite, with b(y) >= 0")
        ds = _Dataset()
        ds.T, ds.Tp = T, _r(T, 16)
        ds.X = self._z(ds.Tp, self.Dp)
        ds.Xt = self._z(self.Dp, ds.Tp)
        st = self._st()
        if X is None:
            assert basis is not None
            basis = np.ascontiguousarray(basis, dtype=np.float64)
            R, B = basis.shape
            assert B == self.B
            clip = int(basis.min() >= 0 and Y.min() >= 0)
            S_dev = torch.from_numpy(Y).to(self.dev)
            b_dev = torch.from_numpy(basis).to(self.dev)
            call("pgl_design_matrix", S=ptr(S_dev), lds=self.N, basis=ptr(b_dev), X=ptr(ds.X), ldx=self.Dp, Xt=ptr(ds.Xt), ldxt=ds.Tp, T=T,
                 N=self.N, B=self.B, R=R, clip=clip, hip_stream=st)
            torch.cuda.synchronize(self.dev)
        else:
            X = np.ascontiguousarray(X, dtype=np.float64).reshape(T, self.D)
            ds.X[:T, :self.D] = torch.from_numpy(X).to(self.dev)
            ds.X[:T, self.D] = 1.0
            call("pgl_transpose", ptr(ds.X), self.Dp, ptr(ds.Xt), ds.Tp, T, self.D + 1, st)
        ds.elem0 = sum(d.T for d in self.datasets)
        self.datasets.append(ds)
        if self.design_only:
            return ds
        ds.Y = self._z(T, self.ldn)
        ds.Y[:, :self.nloc] = torch.from_numpy(np.ascontiguousarray(Y[:, self.n0:self.n1])).to(self.dev)
        if obs_terms is not None:
            # [T][3 ldn] = a | b | log c (pgl_pg_loglik_ex), allocated before the batch size and the integer Gram's plan are chosen from the
            # memory left: 2.5 GB per data set at N = 1024, T = 1e5
            ds.hooks = self._z(T, 3, self.ldn)
            for k in range(3):
                ds.hooks[:, k, :self.nloc] = torch.from_numpy(np.require(terms[k], requirements=["C", "W"])).to(self.dev)
        if self.K:
            # like the hooks' terms, before the batch size and the integer Gram's plan are chosen from the memory left
            self.reserve("covariates: S and the offset of a data set need", 8 * T * (self.K + self.ldn))
            if self.Q:                                # [S_obs | X]: the latent columns start at zero (the first step draws them from the prior)
                ds.S = self._z(T, self.K)
                if self.K_obs:
                    ds.S[:, :self.K_obs] = torch.from_numpy(S_cov).to(self.dev)
            else:
                ds.S = torch.from_numpy(S_cov).to(self.dev)
            ds.Off = self._z(T, self.ldn)
            self._offset(ds, self._st())
        self._ensure_batch()
        ds.Psi = self._z(T, self.ldn)
        if not self.likelihood_only:
            ds.OK = self._z(ds.Tp, 2 * self.ldn)      # [Omega | Kappa], rows >= T stay zero
        ds.llpart = self._z(_lib.load().pgl_pg_loglik_partials(T), self.nloc)
        if self.likelihood_only:
            torch.cuda.synchronize(self.dev)
            ds.X = ds.OK = None                   # the activation contraction reads X' only
            return ds
        plan = self._i8_plan(T)
        ds.int8 = plan is not None
        if ds.int8:
            # residue planes of X, scaled column by column from the columns' norms and maxima: kept for the life of the data set where
            # they fit (plan["resident"]), else converted slice by slice inside the sweep
            lib = _lib.load()
            ds.planes = plan["planes"]
            stat = self._z(2, self.D)
            ds.sA = self._z(self.D)
            call("pgl_i8_colstats", X=ptr(ds.X), ldx=self.Dp, Om=None, ldo=0, T=T, D=self.D, G=1, amax=ptr(stat[0]), sumsq=ptr(stat[1]),
                 hip_stream=st)
            call("pgl_i8_scales", ptr(stat[0]), ptr(stat[1]), self.D, T, ds.planes, ptr(ds.sA), st)
            ds.xmax = stat[0]               # column maxima of X: with _i8_norm, the sweep takes the norms of omega_n X per batch (pgl_sweep_t.i8_norm)
            if self._i8_norm is None:
                self._i8_norm = self._z((self.nb + 2) * self.Dp + self.nloc + 2)
            ds.PA = None
            if plan["resident"]:
                ds.PA = torch.empty(lib.pgl_i8_plane_bytes(self.D, T) // lib.pgl_i8_max_planes() * ds.planes, dtype=torch.int8, device=self.dev)
                call("pgl_i8_planes_t", Xt=ptr(ds.Xt), ldt=ds.Tp, Om=None, ldo=0, scale=ptr(ds.sA), planes=ptr(ds.PA), T=T, D=self.D, G=1,
                     nplanes=ds.planes, t0=0, hip_stream=st)
            self._i8_reserve(T, plan)
            torch.cuda.synchronize(self.dev)
        if self.obs == OBS_GAUSSIAN:
            ones = self._z(ds.Tp, 2)
            ones[:T, 0] = 1.0
            call("pgl_weighted_gram", X=ptr(ds.X), ldx=self.Dp, x_cols=self.Dp, W=ptr(ones), ldw=2, Tp=ds.Tp, D=self.D, nz=1, J=ptr(self.G0),
                 ldj=self.ldj, strideJ=self.ldj * self.ldj, accumulate=int(len(self.datasets) > 1), hip_stream=st)
            torch.cuda.synchronize(self.dev)
        return ds

    # ------------------------------------------------------------------ integer-MFMA Gram: when, and its scratch
    I8_GROUPS = (64, 32, 16, 8, 4, 2, 1)     # neurons converted and multiplied per launch (their planes are `planes` T D bytes each)
    I8_MIN_D, I8_MIN_T = 1024, 2048
    I8_SMALL_T = 16384                       # below I8_MIN_D columns: only for long data sets, and only where a cost model says so (_i8_pays)

    def _i8_pays(self, T, planes=13):
        """gram='auto' below I8_MIN_D columns: the integer path only if a cost model says it wins by 10 %.  Per neuron and time bin, from rates
        measured on MI355X at T = 50 000 (profiles/archive/r04_small_D_crossover.md): the fp64 kernel takes 2.9e-14 s per multiply-add slot of its
        lower 128-tiles; an item of the integer product (one 320-tile of one plane) 1.9e-8 s on its CU, a launch _i8_rounds item-times for
        its group of neurons; the plane conversion 1.95e-13 s per byte.  Measured, ms per sweep int8 / fp64: D = 320 12.8 / 17.7, D = 500
        (padded to 640) 33.6 / 33.7, D = 640 41.5 / 56, D = 650 (padded to 960) 64.3 / 79.6, D = 900 95.2 / 165.6.
        The group size the model is priced at comes from the WHOLE model (min(64, N) neurons per launch), not from how many neurons this
        shard or batch holds: the two Gram paths differ in the last bits, so the choice must be the same on 1 GPU and on 8 (a shard of 2
        neurons of a 128-neuron model takes the integer path like the whole model does, at a launch it does not fill)."""
        if T < self.I8_SMALL_T:
            return False
        nt, nq = -(-self.D // 128), -(-self.D // 320)
        t64 = nt * (nt + 1) // 2 * 128 * 128 * 2.9e-14
        G = max(g for g in self.I8_GROUPS if g <= max(1, min(self.I8_GROUPS[0], self.N)))
        t8 = self._i8_rounds(G, nq * (nq + 1) // 2, planes) / G * 1.9e-8 + planes * nq * 320 * 1.95e-13
        return t8 < 0.9 * t64

    @staticmethod
    def _i8_rounds(G, ntiles, planes, cus=256):
        """item-times one product launch over G neurons takes (pgl_i8gram.hip): G a multiple of 8 -> per-XCD lists (cus / 8 workgroups each)
        of (planes - 1) x G/8 x ntiles whole items, then the last plane's items in K quarters; otherwise one flat list.  What the choice of
        the group size goes by: 8 neurons of a small model (BASELINE configs[1]: 3 tiles per plane, 312 items for 256 CUs) leave the chip
        half idle in their second round, 64 run 9.75 full rounds."""
        if G % 8:
            return float(-(-ntiles * planes * G // cus))
        per = cus // 8
        npx = G // 8
        full, quarters = ntiles * npx * (planes - 1), 4 * ntiles * npx
        t, rf = divmod(full, per)
        if rf:
            t += 1
            quarters = max(0, quarters - 4 * (per - rf))
        return t + -(-quarters // per) / 4.0

    def _i8_plan(self, T):
        """-> None (this data set's Gram runs on the fp64 kernel) or how it goes through the int8 MFMA: dict(planes, resident, G, slice).
        The integer path is taken if asked for, or (auto) at shapes where it is the faster one (320 x 320 tiles, 13 planes: not for small D
        or short T).  Memory decides the rest: X's planes stay resident if they are a small part of what is free; the planes of omega_g X
        for a group of G neurons and the group's residues must fit -- G = 8 (one neuron per XCD) at large D, more where a plane has only
        a few tiles (_i8_rounds); if a whole data set's planes do not fit (BASELINE configs[4]: 86 GB of planes per neuron), the product
        runs in time slices that add up in the residues (pgl_sweep_t.i8_slice), and only if not even a short slice fits does the data set
        fall back to the fp64 kernel (with a warning)."""
        if self.obs == OBS_GAUSSIAN or self.design_only or self.likelihood_only or self.gram == "fp64":
            return None
        if self.gram != "int8" and (T < self.I8_MIN_T or (self.D < self.I8_MIN_D and not self._i8_pays(T, self.planes or 13))):
            return None
        lib = _lib.load()
        planes = self.planes or lib.pgl_i8_min_planes(T)
        if lib.pgl_i8_norm_bits(planes, T) < 8:
            raise ValueError("%d residue planes cannot hold T = %d time bins" % (planes, T))
        over = self._i8_over
        mp = lib.pgl_i8_max_planes()
        Dq = lib.pgl_i8_padded_rows(self.D)
        pa_full = lib.pgl_i8_plane_bytes(self.D, T) // mp * planes
        kp_full = max(256, -(-T // 64) * 64)                     # bytes per plane row: the bins, padded to the 64-byte K tile
        per_bin = planes * Dq                                    # bytes of one time bin in one set of planes
        r1 = lib.pgl_i8_residue_bytes(self.D) // mp * planes
        free = self._free_bytes()
        have = self._i8_scratch.bytes if self._i8_scratch else 0
        budget = int(0.85 * free) + have
        gmax = int(max(1, min(over["group"] or self.I8_GROUPS[0], self.nb or self.nloc)))
        groups = [G for G in self.I8_GROUPS if G <= gmax] or [1]
        if over["group"]:
            groups = [G for G in groups if G == min(over["group"], gmax)] or [min(over["group"], gmax)]
        keep = pa_full <= 0.3 * free if over["resident"] is None else bool(over["resident"])
        ntiles = (Dq // 320) * (Dq // 320 + 1) // 2
        cus = torch.cuda.get_device_properties(self.dev).multi_processor_count

        def fit(resident, G):      # time bins per slice that fit with this choice
            fixed = (pa_full if resident else 0) + G * r1 + (3 * G * Dq * Dq if G % 8 == 0 else 0)
            return int((budget - fixed) // (per_bin * (G + (0 if resident else 1))))
        if over["slice"]:
            S = max(64, int(over["slice"]) // 64 * 64)
            return dict(planes=planes, resident=keep, G=groups[0] if over["group"] else min(gmax, 8), slice=S if S < T else 0)
        for resident in ((True, False) if keep else (False,)):
            ok = [G for G in groups if fit(resident, G) >= kp_full]
            if ok:
                # the largest group up to 8 that fits (one neuron per XCD), more only where the per-neuron cost of a launch (item-times) falls
                # by 1.5 % or more with it (memory is better spent elsewhere)
                cost = {G: self._i8_rounds(G, ntiles, planes, cus) / G for G in ok}
                small = [G for G in ok if G <= 8]
                pick = max(small) if small else min(ok)
                for G in sorted(G for G in ok if G > 8 and G > pick):
                    if cost[G] < 0.985 * cost[pick]:
                        pick = G
                return dict(planes=planes, resident=resident, G=pick, slice=0)
        cands = [(resident, G, fit(resident, G)) for resident in ((True, False) if keep else (False,)) for G in groups if G <= 8]
        cands = [c for c in cands if c[2] >= 16384]
        if not cands:
            if self.gram == "int8":
                raise _lib.PglError("gram='int8': the residue planes do not fit")
            import warnings
            warnings.warn("gram='auto': not even a 16384-bin slice of the residue planes of this data set (D = %d, T = %d) fits in the %.0f GB free "
                          "on %s; its likelihood Gram runs on the fp64 MFMA kernel" % (self.D, T, free / 1e9, self.dev), RuntimeWarning, stacklevel=3)
            return None
        resident, G, S = max(cands, key=lambda c: (min(c[2], kp_full // 2), c[1]))       # long slices first (at least two are needed anyway), then large groups
        nsl = -(-T // (S // 1024 * 1024))
        S = -(-(-(-T // nsl)) // 1024) * 1024                                             # equal slices, multiples of 1024 bins
        return dict(planes=planes, resident=resident, G=G, slice=int(S))

    def _i8_reserve(self, T, plan):
        """scratch for the planes of omega_g X (one time slice of them) and the residues of a group of G neurons -- and for a slice of X's own
        planes where those are not resident -- sized for the largest need seen so far.  One slice length per engine (pgl_sweep_t.i8_slice): the
        shortest any of its data sets needs; a data set no longer than that runs unsliced, and slices of any length add up to the same bits,
        so data sets planned with different slicing simply share the shorter one."""
        lib = _lib.load()
        mp, planes = lib.pgl_i8_max_planes(), plan["planes"]
        S, G, T0 = plan["slice"], plan["G"], 0
        old = self._i8_scratch
        if old and old.slice and (not S or old.slice < S):
            S = old.slice
        Ts = min(S, T) if S else T
        pb1, r1 = lib.pgl_i8_plane_bytes(self.D, Ts) // mp * planes, lib.pgl_i8_residue_bytes(self.D) // mp * planes
        pas = 0 if plan["resident"] else pb1
        if old:
            old_pas = old.PAs.numel() if old.PAs is not None else 0
            if old.G == G and old.slice == S and old.T >= T and old.PB.numel() >= G * pb1 and old.R.numel() >= G * r1 and old_pas >= pas:
                return
            pb1, r1 = max(pb1, old.PB.numel() // old.G), max(r1, old.R.numel() // old.G)      # keep what earlier data sets need
            pas = max(pas, old_pas)
            G, T0 = min(G, old.G), old.T
        self._i8_scratch = old = None
        torch.cuda.empty_cache()
        Dq = lib.pgl_i8_padded_rows(self.D)
        self._i8_scratch = _I8Scratch(bytes=G * (pb1 + r1) + pas, T=max(T, T0), G=G, PB=torch.empty(G * pb1, dtype=torch.int8, device=self.dev),
                                      R=torch.empty(G * r1, dtype=torch.int8, device=self.dev), stat=self._z(3, G, self.D), slice=S,
                                      PAs=torch.empty(pas, dtype=torch.int8, device=self.dev) if pas else None,
                                      Rx=torch.empty(3 * G * Dq * Dq, dtype=torch.int8, device=self.dev) if G % 8 == 0 else None)

    @_on_device
    def drop_int8(self, i):
        """put data set i on the fp64 Gram kernel and release its residue planes (the population model does this on every rank when ANY
        rank could not take the integer path, so that the choice never depends on the rank)"""
        ds = self.datasets[i]
        if ds.int8:
            ds.int8 = False
            ds.PA = ds.sA = ds.xmax = None
            if not any(d.int8 for d in self.datasets):
                self._i8_norm = None
                self._i8_scratch = None             # nobody multiplies planes any more: the group buffers (56 GB at cfg3) go back too
            torch.cuda.empty_cache()

    @_on_device
    def set_noise(self, eta):
        """noise variances eta (nloc,) of the Gaussian observation model (regression.py:380-398)"""
        assert self.obs == OBS_GAUSSIAN
        self.eta = np.asarray(eta, dtype=np.float64).reshape(self.nloc).copy()
        self.inv_eta.copy_(torch.from_numpy(1.0 / self.eta))

    @_on_device
    def design_matrix(self, i=0):
        ds = self.datasets[i]
        if ds.X is None:                          # likelihood-only engines keep the transposed copy only
            return ds.Xt[:self.D, :ds.T].t().contiguous().cpu().numpy().reshape(ds.T, self.N, self.B)
        return ds.X[:ds.T, :self.D].cpu().numpy().reshape(ds.T, self.N, self.B)

    # ------------------------------------------------------------------ activation / PG / log-likelihood
    def _upload_weights(self, a, W, b):
        aw = (np.asarray(a, dtype=np.float64)[:, :, None] * np.asarray(W, dtype=np.float64)).reshape(self.nloc, self.D)
        Wt = np.zeros((self.Dp, self.ldn))
        Wt[:self.D, :self.nloc] = aw.T
        self.Wt.copy_(torch.from_numpy(Wt))
        self.bias.copy_(torch.from_numpy(np.asarray(b, dtype=np.float64).reshape(self.nloc)))

    def fold_data(self, stage, launch, only=None, offset=True, activate=True):
        """THE walk over the data sets, behind weights the caller has uploaded (_upload_weights): per data set ONE activation -- Psi =
        X (a * W)' for the whole shard (regression.py:195-201; bias not added), a stage of its own --, then launch(i, ds, st, first) as
        the timed stage `stage` (work: T * nloc cells; None: the launch times its stages itself) on the engine's stream st.  first: the
        first data set visited -- the launch overwrites its sums there and adds to them behind it.  only = i: data set i alone.  Returns
        st.  Having this method is what makes an engine a device engine (summary.device_engine).  An engine with covariates adds each
        data set's offset to Psi right behind the activation: the read-outs follow beta without knowing of it; offset=False leaves Psi
        the net activation (the covariate and latent folds), activate=False as a walk just before left it."""
        st, first = self._st(), True
        for i, ds in enumerate(self.datasets):
            if only is not None and i != only:
                continue
            if activate:
                h = self._tic("activation", 2.0 * ds.T * self.D * self.nloc)
                call("pgl_activation", Xt=ptr(ds.Xt), ldxt=ds.Tp, Wt=ptr(self.Wt), ldw=self.ldn, Psi=ptr(ds.Psi), ldpsi=self.ldn, T=ds.T,
                     Dk=self.Dp, nloc=self.nloc, hip_stream=st)
                self._toc(h)
                if offset and self.K:
                    call("pgl_covariate_add_offset", Psi=ptr(ds.Psi), ldpsi=self.ldn, Off=ptr(ds.Off), ldo=self.ldn, T=ds.T, nloc=self.nloc,
                         hip_stream=st)
            h = self._tic(stage, float(ds.T) * self.nloc) if stage else None
            launch(i, ds, st, first)
            self._toc(h)
            first = False
        return st

    def reserve(self, what, nbytes, cap=None):
        """THE memory gate, passed BEFORE anything is allocated: MemoryError where the nbytes that `what` ("<feature>: the ... need")
        asks for exceed what this engine may still take on its GPU (_free_bytes) -- or cap, where that is less (the chain diagnostics
        pass the engine's mem_budget_bytes; nobody else does)"""
        free = self._free_bytes()
        if cap is not None:
            free = min(free, int(cap))
        if nbytes > free:
            raise MemoryError("%s %d bytes, %d are free on %s" % (what, nbytes, free, self.dev))

    def _psi_pass(self, draw, seed, sweep):
        """activation (regression.py:195-201) for the whole shard + PG/kappa/log-lik (:491-511). Returns ll (nloc,) device."""
        def launch(i, ds, st, first):
            om = ds.OK if draw else None
            kp = ctypes.c_void_p(ds.OK.data_ptr() + 8 * self.ldn) if draw else None
            if self.obs == OBS_GAUSSIAN:      # self.ll then holds the sums of squared residuals
                call("pgl_gaussian_stats", Psi=ptr(ds.Psi), ldpsi=self.ldn, bias=ptr(self.bias), Y=ptr(ds.Y), ldy=self.ldn, inv_eta=ptr(self.inv_eta),
                     Omega=ptr(om), ldo=2 * self.ldn, Kappa=kp, ldk=2 * self.ldn, part=ptr(ds.llpart), sse_out=ptr(self.ll),
                     accumulate=int(not first), T=ds.T, nloc=self.nloc, hip_stream=st)
            else:
                call("pgl_pg_loglik_ex", Psi=ptr(ds.Psi), ldpsi=self.ldn, bias=ptr(self.bias), Y=ptr(ds.Y), ldy=self.ldn, Omega=ptr(om),
                     ldo=2 * self.ldn, Kappa=kp, ldk=2 * self.ldn, llpart=ptr(ds.llpart), ll_out=ptr(self.ll), accumulate=int(not first),
                     T=ds.T, nloc=self.nloc, obs=self.obs, xi=self.xi, param=ptr(self.obs_param), hooks=ptr(ds.hooks), ldh=self.ldn,
                     seed=int(seed), sweep=int(sweep), neuron0=self.n0, elem0=ds.elem0, hip_stream=st)
        self.fold_data("pg_loglik", launch)
        return self.ll

    @_on_device
    def log_likelihood(self, a, W, b):
        """per-neuron sum_t log p(y_t | psi_t) (regression.py:491-494 summed as at models.py:93-94)."""
        self._upload_weights(a, W, b)
        return self._ll_host(self._psi_pass(False, 0, 0))

    def _ll_host(self, ll_dev):
        return self._ll_host_np(ll_dev.cpu().numpy().copy())

    def _ll_host_np(self, ll):
        if self.obs == OBS_GAUSSIAN:          # regression.py:399-403 summed over t: -T/2 log(2 pi eta) - sse / (2 eta)
            T = sum(ds.T for ds in self.datasets)
            ll = -0.5 * T * np.log(2 * np.pi * self.eta) - 0.5 * ll / self.eta
        return ll

    @_on_device
    def sse(self, a, W, b):
        """sum_t (y - mean)^2 per local neuron, the statistic of _resample_eta (regression.py:433-445)"""
        assert self.obs == OBS_GAUSSIAN
        self._upload_weights(a, W, b)
        return self._psi_pass(False, 0, 0).cpu().numpy().copy()

    @_on_device
    def psi(self, a, W, b, i=0):
        self._upload_weights(a, W, b)
        self._psi_pass(False, 0, 0)
        ds = self.datasets[i]
        return ds.Psi[:, :self.nloc].cpu().numpy()

    @_on_device
    def psi_columns(self, a, W, b, i, cols, start, stop):
        """rows [start, stop) and the local columns `cols` of psi(a, W, b, i) -> host (stop - start, len(cols)): the slice is taken on the
        device, so only it crosses to the host (conditional simulation reads a few neurons' columns of a long recording)"""
        self._upload_weights(a, W, b)
        self._psi_pass(False, 0, 0)
        idx = torch.from_numpy(np.ascontiguousarray(cols, dtype=np.int64)).to(self.dev)
        return self.datasets[i].Psi[start:stop].index_select(1, idx).cpu().numpy()

    # ------------------------------------------------------------------ external covariates (pyglm_amd/covariates.py)
    def _offset(self, ds, st):
        """queues Off = S beta' of data set ds from the weights on the device"""
        call("pgl_covariate_offset", S=ptr(ds.S), lds=self.K, Beta=ptr(self.beta_dev), Off=ptr(ds.Off), ldn=self.ldn, T=ds.T, nloc=self.nloc,
             K=self.K, hip_stream=st)

    @_on_device
    def set_covariate_weights(self, beta):
        """beta (nloc, K) of this shard's neurons onto the device, and every data set's offset rebuilt from it"""
        if not self.K:
            raise ValueError("set_covariate_weights(): this engine was built with n_covariates=0")
        beta = np.asarray(beta, dtype=np.float64).reshape(self.nloc, self.K)
        bt = np.zeros((self.K, self.ldn))
        bt[:, :self.nloc] = beta.T
        self.beta_dev.copy_(torch.from_numpy(bt))
        self.beta = beta.copy()
        st = self._st()
        for ds in self.datasets:
            self._offset(ds, st)

    # ------------------------------------------------------------------ latent common input (pyglm_amd/latents.py)
    def _need_latents(self, what):
        if not self.Q:
            raise ValueError("%s: this engine was built with n_latents=0" % what)

    @_on_device
    def latents(self, i=0):
        """X (T_i, Q) of data set i: a host copy of the latent columns of its S"""
        self._need_latents("latents()")
        return self.datasets[i].S[:, self.K_obs:].cpu().numpy().copy()

    @_on_device
    def set_latents(self, i, X):
        """X (T_i, Q) into the latent columns of data set i's S, and that data set's offset rebuilt from it"""
        from .latents import check_latents
        self._need_latents("set_latents()")
        ds = self.datasets[i]
        ds.S[:, self.K_obs:] = torch.from_numpy(check_latents(X, ds.T, self.Q)).to(self.dev)
        self._offset(ds, self._st())

    # ------------------------------------------------------------------ one Gibbs sweep of the shard's regressions
    def _sweep_args(self, ovs=None):
        """the argument block of pgl_sweep and pgl_sweep_gram.  Every buffer is persistent, so the struct is built once -- again when the I/O
        buffer, the data sets, the batch or the integer Gram's scratch change, and for a call with omega overrides (ovs: one (T, nloc) device
        array per data set, kept alive by the caller) -- and the caller assigns what changes from sweep to sweep (the inputs, the hints, the
        optional outputs)"""
        i8 = self._i8_scratch
        sig = (self._din.data_ptr(), len(self.datasets), id(i8), self.nb, tuple(ds.int8 for ds in self.datasets))
        if ovs or self._sweep_cache is None or self._sweep_cache[0] != sig:
            dsets = (_lib.Dataset * len(self.datasets))()
            for i, ds in enumerate(self.datasets):
                dsets[i] = _lib.Dataset(T=ds.T, Tp=ds.Tp, X=ptr(ds.X), Xt=ptr(ds.Xt), Y=ptr(ds.Y), Psi=ptr(ds.Psi), OK=ptr(ds.OK), llpart=ptr(ds.llpart),
                                        elem0=ds.elem0, int8=int(ds.int8), planes=ds.planes, sA=ptr(ds.sA), PA=ptr(ds.PA),
                                        omega_override=ptr(ovs[i]) if ovs else None, xmax=ptr(ds.xmax), hooks=ptr(ds.hooks))
            i8_args = dict(i8_group=i8.G, i8_PB=ptr(i8.PB), i8_R=ptr(i8.R), i8_stat=ptr(i8.stat), i8_slice=i8.slice, i8_PAs=ptr(i8.PAs),
                           i8_Rx=ptr(i8.Rx)) if i8 else {}
            sw = _lib.Sweep(N=self.N, B=self.B, n0=self.n0, nloc=self.nloc, nb=self.nb, obs=self.obs, xi=self.xi, visit_order=int(self.visit_order),
                            planes=self.planes or 0, datasets=dsets, ndatasets=len(self.datasets), a=ptr(self.a_dev), W=ptr(self.W_dev),
                            b=ptr(self.b_dev), inv_eta=ptr(getattr(self, "inv_eta", None)), G0=ptr(getattr(self, "G0", None)), ll=ptr(self.ll),
                            status=ptr(self.status), Wt=ptr(self.Wt), bias=ptr(self.bias), border=ptr(self.border), skip=ptr(self.skip),
                            Jbuf=ptr(self.Jbuf), Mtab=ptr(self.Mtab), Ac=ptr(self.Ac), hc=ptr(self.hc), Tinv=ptr(self.Tinv), G=ptr(self.G),
                            Lws=ptr(self.Lws), Ut=ptr(self.Ut), Wt_ws=ptr(self.Wt_ws), d_idx=ptr(self.d_idx), d_sign=ptr(self.d_sign),
                            d_cnt=ptr(self.d_cnt), batch_k=ptr(self.batch_k), act=ptr(self.act), na=ptr(self.na), obs_param=ptr(self.obs_param),
                            **i8_args)
            self._sweep_cache = None if ovs else (sig, sw, dsets)       # (the override tensors die with the caller's call)
        else:
            sw = self._sweep_cache[1]
        sw.i8_norm = ptr(self._i8_norm) if i8 else None
        if self.profile and self._times is None:
            self._times = _lib.StageTimes()
            if self.profile is not True:
                names = [_lib.load().pgl_stage_name(i).decode() for i in range(_lib.NSTAGES)]
                self._times.mask = sum(1 << names.index(n) for n in self.profile)
        sw.times = ctypes.pointer(self._times) if self.profile else None
        return sw

    @_on_device
    def sweep(self, a, W, b, rho, Jw, hw, Jb, hb, c0, perm, u, z, seed, sweep, omega_override=None, host_overlap=None, nrun=0,
              after_queue=None, readback=True, nfirst=0, copy=True, want_stats=False):
        """regression.py:265-280 for every local neuron, as ONE call of pgl_sweep (include/pyglm_hip.h): the whole sweep is queued on the
        stream without a host synchronisation.  a (nloc,N) bool, W (nloc,N,B), b (nloc,), hyper-parameters in natural form
        (prior_terms), random inputs from make_draws.  Returns (a, W, b, ll_before) as host arrays.
        omega_override: list of (T, nloc) arrays replacing the PG draws (test hook: the reference fixtures inject omega).
        host_overlap: optional callable run on the host while the GPU works through the queue (seconds at full size), e.g. to draw the
        next sweep's permutations.
        nrun, nfirst: sweep only local neurons [nfirst, nfirst + nrun) (what one rank of a larger job would do, timed on this GPU -- bench.py's
        scaling_proxy times every shard of a G-rank job this way); the returned rows of the others are their input.
        after_queue: optional callable(engine) run right after the sweep has been queued, with the engine's device current -- the
        population model packs the new rows (packed_state) and starts its all_gather there, behind the sweep on the same stream.
        readback=False: the new (a, W, b) stay on the device (a_dev / W_dev / b_dev, packed_state); only ll and the status flags come
        back: returns (None, None, None, ll); flags of a non-positive-definite system do not raise here (self.last_status; they travel in
        the packed rows and the population model raises on every rank).
        want_stats: the rows' sufficient statistics for the network prior (row_stats) are taken behind the sweep and come back with the
        state in the same wait: self.last_row_stats (nloc, 1 + B + B^2), a view of a pinned buffer valid until the next sweep.
        copy=False: the returned a (int32), W, b are VIEWS of the engine's pinned read-back buffer, valid until its next sweep -- for a
        caller that stores them into arrays of its own right away (the population model: one pass over 42 MB at N = 1024 instead of three)."""
        nloc, N, B, D = self.nloc, self.N, self.B, self.D
        if self.likelihood_only or self.design_only:
            raise _lib.PglError("this engine was built without sweep buffers (likelihood_only / design_only)")
        self._ensure_batch()
        st = self._st()
        a = np.asarray(a).astype(bool)
        rho = np.asarray(rho, dtype=np.float64)
        det = np.all((rho < 1e-6) | (rho > 1 - 1e-6), axis=1)           # regression.py:153-155 (decided again, per row, on the device)
        # chain state + hyper-parameters + random inputs -> ONE pinned staging buffer -> one copy to the device
        label = None
        if isinstance(Jw, BlockPrior):
            label, c0, hw, Jw = Jw.label, Jw.c0_u, Jw.hw_u, Jw.Jw_u        # tables + labels travel; the device gathers c0
        off_a, off_W, off_b, off_ll, off_st, sb = self._io_state_layout()
        items = [("rho", rho, np.float64), ("Jw", Jw, np.float64), ("hw", hw, np.float64), ("Jb", Jb, np.float64), ("hb", hb, np.float64),
                 ("c0", c0, np.float64), ("perm", perm, np.int32), ("u", u, np.float64), ("z", z, np.float64)]
        if label is not None:
            items.append(("label", label, np.int32))
        arrs, offs, off = {}, {}, sb
        for k, v, dt in items:
            arr = np.ascontiguousarray(v, dtype=dt)
            arrs[k], offs[k] = arr, off
            off = (off + arr.nbytes + 15) // 16 * 16
        self._io_reserve(off - sb)
        hin = self._hin_np
        hin[off_a:off_a + 4 * nloc * N].view(np.int32)[:] = a.reshape(-1)
        hin[off_W:off_W + 8 * nloc * D].view(np.float64)[:] = np.asarray(W, dtype=np.float64).reshape(-1)
        hin[off_b:off_b + 8 * nloc].view(np.float64)[:] = np.asarray(b, dtype=np.float64).reshape(-1)
        for k, arr in arrs.items():
            hin[offs[k]:offs[k] + arr.nbytes] = arr.reshape(-1).view(np.uint8)
        self._din[:off].copy_(self._hin[:off], non_blocking=True)
        base = self._din.data_ptr()
        dp = {k: ctypes.c_void_p(base + o) for k, o in offs.items()}
        dp.setdefault("label", None)
        self.logodds = torch.empty((nloc, N), dtype=F64, device=self.dev) if self.keep_logodds else None
        if label is not None and (self._c0_dense is None):
            self._c0_dense = self._z(nloc, N)
        ovs = None
        if omega_override is not None:
            ovs = [torch.from_numpy(np.ascontiguousarray(omega_override[i], dtype=np.float64).reshape(ds.T, nloc)).to(self.dev)
                   for i, ds in enumerate(self.datasets)]
        sw = self._sweep_args(ovs)
        sw.rho, sw.Jw, sw.hw, sw.label, sw.Jb, sw.hb, sw.c0 = dp["rho"], dp["Jw"], dp["hw"], dp["label"], dp["Jb"], dp["hb"], dp["c0"]
        sw.perm, sw.u, sw.z = dp["perm"], dp["u"], dp["z"]
        self._perm_off, self._sweep_serial = offs["perm"], self._sweep_serial + 1
        sw.logodds, sw.c0_dense = ptr(self.logodds), ptr(self._c0_dense)
        n_act = int(a.sum(axis=1).max()) if a.size else 0
        sw.nrun, sw.nfirst, sw.all_deterministic = int(nrun), int(nfirst), int(det.all())
        sw.init_rows_bound = 1 + B * n_act
        sw.active_rows_bound = (1 + B * int(np.round(rho).sum(axis=1).max())) if det.all() else 0
        sw.flip_single_pass = int(self.flip_single_pass)
        t_launch = time.perf_counter()
        if self.K:
            # under the covariates' offsets: omega and ll at psi + o, Kappa left reduced by Omega * o
            offs_arr = (ctypes.c_void_p * len(self.datasets))(*[ds.Off.data_ptr() for ds in self.datasets])
            call("pgl_sweep_offset", ctypes.byref(sw), offs_arr, int(seed), int(sweep), st)
        else:
            call("pgl_sweep", ctypes.byref(sw), int(seed), int(sweep), st)
        self.launch_seconds += time.perf_counter() - t_launch
        self.last_row_stats = None
        if want_stats:
            if getattr(self, "_stats_dev", None) is None:
                self._stats_dev = torch.empty((nloc, 1 + B + B * B), dtype=F64, device=self.dev)
                self._stats_host = torch.empty((nloc, 1 + B + B * B), dtype=F64).pin_memory()
            call("pgl_row_stats", ptr(self.a_dev), ptr(self.W_dev), ptr(self._stats_dev), N, B, nloc, self.n0, st)
            self._stats_host.copy_(self._stats_dev, non_blocking=True)        # (pgl_get_state below waits for the stream)
        if after_queue is not None:
            after_queue(self)
        if host_overlap is not None:
            t_ov = time.perf_counter()
            host_overlap()
            self.overlap_seconds += time.perf_counter() - t_ov
        t_wait = time.perf_counter()
        # state, log-likelihood and flags back into the pinned twin of the state block (pgl_get_state waits for the stream)
        hout = self._hout_np
        hp = self._hout.data_ptr()
        call("pgl_get_state", ctypes.byref(sw), ctypes.c_void_p(hp + off_a) if readback else None, ctypes.c_void_p(hp + off_W) if readback else None,
             ctypes.c_void_p(hp + off_b) if readback else None, ctypes.c_void_p(hp + off_ll), ctypes.c_void_p(hp + off_st), st)
        self.wait_seconds += time.perf_counter() - t_wait
        a_i = hout[off_a:off_a + 4 * nloc * N].view(np.int32).reshape(nloc, N) if readback else None
        W_new = hout[off_W:off_W + 8 * nloc * D].view(np.float64).reshape(nloc, N, B) if readback else None
        b_new = hout[off_b:off_b + 8 * nloc].view(np.float64) if readback else None
        if readback and copy:
            W_new, b_new = W_new.copy(), b_new.copy()
        ll = hout[off_ll:off_ll + 8 * nloc].view(np.float64).copy()
        status = hout[off_st:off_st + 4 * nloc].view(np.int32).copy()
        if want_stats:
            self.last_row_stats = self._stats_host.numpy()
        del ovs
        self.last_status = status
        if status.any() and readback:
            # the reference's np.linalg.cholesky raises at the first such neuron (regression.py:369-370), with the neurons before it already
            # updated.  Here the whole shard has been computed: the exception names every neuron concerned (global indices) and carries the
            # shard's results, of which the rows of the other neurons are good; the caller's state is left as it was before the sweep
            bad = np.nonzero(status)[0]
            err = np.linalg.LinAlgError("posterior system not positive definite for neurons %s (local %s, flags %s)"
                                        % ((bad[:8] + self.n0).tolist(), bad[:8].tolist(), status[bad[:8]].tolist()))
            err.neurons = (bad + self.n0).tolist()
            err.flags = status[bad].tolist()
            err.state = (a_i.astype(bool), W_new.copy(), b_new.copy()) if readback else None
            raise err
        if readback and not copy:
            return a_i, W_new, b_new, self._ll_host_np(ll)
        return (a_i.astype(bool) if readback else None), W_new, b_new, self._ll_host_np(ll)       # (astype copies out of the staging buffer)

    @_on_device
    def row_stats(self):
        """[count, sum w, sum w w'] over the active off-diagonal weight vectors of every local neuron's row, (nloc, 1 + B + B^2) on the device,
        from the state the last sweep left there (pgl_row_stats): what the network prior needs of this shard (networks.py:132-149).
        Queued on the current stream (behind the sweep)."""
        out = torch.empty((self.nloc, 1 + self.B + self.B * self.B), dtype=F64, device=self.dev)
        call("pgl_row_stats", ptr(self.a_dev), ptr(self.W_dev), ptr(out), self.N, self.B, self.nloc, self.n0, self._st())
        return out

    @_on_device
    def packed_state(self):
        """the shard's chain state as the sweep left it on the device, one row of bytes per neuron: W | b | eta (0) | row statistics | a
        (models.state_row_layout) -- what a rank contributes to the per-sweep all_gather.  Queued on the current stream (behind the sweep)."""
        from .models import state_row_layout
        ob, oe, os_, oa, rb = state_row_layout(self.N, self.B)
        nl = self.nloc
        p = torch.zeros((nl, rb), dtype=torch.uint8, device=self.dev)
        p[:, :ob] = self.W_dev.view(torch.uint8).view(nl, ob)
        p[:, ob:oe] = self.b_dev.view(torch.uint8).view(nl, 8)
        if self.obs != OBS_GAUSSIAN:
            # the slot of the Gaussian model's noise variance carries the sweep's status flags here (0 = fine): after the gather EVERY rank sees
            # every neuron's flag and raises the same LinAlgError in the same sweep, instead of one rank leaving the others at a collective
            p[:, oe:os_] = self.status.to(F64).view(torch.uint8).view(nl, 8)
        p[:, os_:oa] = self.row_stats().view(torch.uint8).view(nl, oa - os_)
        p[:, oa:oa + self.N] = self.a_dev.to(torch.uint8)
        return p

    # test hooks --------------------------------------------------------------------------------------------------
    @_on_device
    def sweep_gram(self, first, count):
        """the likelihood Gram (regression.py:251-252) of local neurons [first, first + count) into Jbuf[:count], formed as a sweep forms it
        for a batch that starts at `first` (pgl_sweep_gram) from the omega in each data set's OK: a sweep's, or the caller's own written into
        ds.OK[:T, first:first + count].  Queued on the current stream"""
        self._ensure_batch()
        call("pgl_sweep_gram", ctypes.byref(self._sweep_args()), int(first), int(count), self._st())

    @_on_device
    def posterior(self, i):
        """assembled (J_post (D+1,D+1), h_post (D+1,)) of batch slot i as dense symmetric host arrays"""
        D = self.D
        M = self.Jbuf[i, :D + 2, :D + 2].cpu().numpy()
        L = np.tril(M)
        full = L + np.tril(L, -1).T
        return full[:D + 1, :D + 1], full[D + 1, :D + 1]
