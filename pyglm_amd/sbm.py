"""Learned priors on the adjacency: a stochastic block model over the neurons (K = 1: the Beta-Bernoulli prior), its Gibbs update, and the
label-invariant summary of the sampled partitions.

    net = SBMSparseNetwork(N, B, K=8)
    model = SparseBernoulliGLM(N, B=B, network=net)
    blocks = model.block_structure()
    for it in range(n_sweeps):
        model.resample_model()
        if it >= burn:
            blocks.collect()
    blocks.coassign, blocks.rho_mean, blocks.consensus()

This module states the law once, in NumPy; the kernels (pgl_sbm.hip) and the tests are held to it.  Row n of A is the postsynaptic neuron,
column m the presynaptic one.

Model.  K blocks, 1 <= K <= 32, a truncation level (empty blocks are allowed): pi ~ Dirichlet(alpha / K), z_n ~ Cat(pi), P[k][l] ~ Beta(a_0, b_0),
A[n][m] ~ Bernoulli(P[z_n][z_m]) for n != m; self-connections A[n][n] ~ Bernoulli(rho_self), rho_self ~ Beta(a_self, b_self) or pinned.

One update (sbm_host), from a generator `rng` and the Philox stream (seed, sweep):
  1. counts (block_counts_host): M[k][l] = sum_{n != m} A[n][m] [z_n = k][z_m = l], n_k = #{n : z_n = k}, d = sum_n A[n][n],
     pairs[k][l] = n_k n_l - [k = l] n_k
  2. P ~ Beta(a_0 + M, b_0 + pairs - M) (one call for the K x K array), rho_self ~ Beta(a_self + d, b_self + N - d) unless pinned,
     pi ~ Dirichlet(alpha / K + n), in this order from rng.  P is clamped into [2^-1000, 1 - 2^-53] and pi to >= 2^-1000, so that every
     logarithm is finite (0 * -inf must not occur); LP = log P, LQ = log1p(-P), logpi = log pi in fp64 (tables)
  3. the scan (sbm_scan_host; skipped for K = 1), for n = 0 .. N - 1 in order, with the z of the moment, over the partners m != n:
       cnt[l] = #{m : z_m = l},  cin[l] = #{m : A[n][m], z_m = l},  cout[l] = #{m : A[m][n], z_m = l}
       s = logpi[k];  for l = 0 .. K-1:  s += cin[l] * LP[k][l], then s += (cnt[l] - cin[l]) * LQ[k][l];
                      for l = 0 .. K-1:  s += cout[l] * LP[l][k], then s += (cnt[l] - cout[l]) * LQ[l][k];     lp[k] = s
       (every product rounded, every sum rounded: NumPy's element-wise arithmetic, and no fused multiply-add on the device)
       e_k = exp(lp[k] - max lp), c_k = e_0 + .. + e_k from the left, u_n = the first uniform of Philox call 0, purpose PURPOSE_SBM, key =
       seed, stream = sweep, element = n (scan_uniforms);  z_n = the smallest k with u_n * c_{K-1} < c_k, else K - 1
  4. rho[n][m] = P[z_n][z_m], rho[n][n] = rho_self (rho_of): what the regressions are handed.
"""
import ctypes

import numpy as np

from . import _lib
from .simulate import _device, _unit, philox_words

MAX_BLOCKS = _lib.PGL_SBM_MAX_BLOCKS
MAX_N = _lib.PGL_SBM_MAX_N
PURPOSE_SBM = _lib.PGL_PURPOSE_SBM
P_MIN, P_MAX, PI_MIN = 2.0 ** -1000, 1.0 - 2.0 ** -53, 2.0 ** -1000


def check_blocks(K):
    if int(K) != K or not 1 <= int(K) <= MAX_BLOCKS:
        raise ValueError("K = %r: an integer in 1 .. %d is required" % (K, MAX_BLOCKS))
    return int(K)


def clamp(P, pi):
    """(P, pi) inside the ranges on which every logarithm of `tables` is finite"""
    return np.clip(np.asarray(P, dtype=np.float64), P_MIN, P_MAX), np.maximum(np.asarray(pi, dtype=np.float64), PI_MIN)


def tables(P, pi):
    """(LP, LQ, logpi) = (log P, log1p(-P), log pi) of the clamped (P, pi)"""
    P, pi = clamp(P, pi)
    return np.log(P), np.log1p(-P), np.log(pi)


def scan_uniforms(seed, sweep, N):
    """u (N,): the scan's uniforms of (seed, sweep)"""
    w = philox_words(seed, PURPOSE_SBM, 0, 0, sweep, N)
    return _unit(w[:, 0], w[:, 1])


def _labels(z, K, N=None):
    z = np.asarray(z)
    if z.ndim != 1 or (N is not None and z.shape[0] != N) or not np.issubdtype(z.dtype, np.integer):
        raise ValueError("z: one integer label per neuron is required")
    if z.size and (z.min() < 0 or z.max() >= K):
        raise ValueError("z: a label outside [0, %d)" % K)
    return z.astype(np.int64)


def _lp_of_counts(cnt, cin, cout, LP, LQ, logpi):
    """lp (..., K) from exact counts (..., K) held as doubles, in the stated order of operations"""
    K = LP.shape[0]
    s = np.array(np.broadcast_to(logpi, cin.shape), dtype=np.float64)
    for l in range(K):
        s = s + cin[..., l, None] * LP[:, l]
        s = s + (cnt[..., l, None] - cin[..., l, None]) * LQ[:, l]
    for l in range(K):
        s = s + cout[..., l, None] * LP[l, :]
        s = s + (cnt[..., l, None] - cout[..., l, None]) * LQ[l, :]
    return s


def decide(lp, u, exp=np.exp):
    """the label one step draws from its lp (K,) and its uniform"""
    e = exp(lp - lp.max())
    c = np.add.accumulate(np.asarray(e, dtype=np.float64))
    hit = np.flatnonzero(u * c[-1] < c)
    return int(hit[0]) if hit.size else lp.shape[0] - 1


def sbm_scan_host(A, z, LP, LQ, logpi, u, return_lp=False, exp=np.exp):
    """step 3 of the update -> z after the scan (int64), and with return_lp the lp (N, K) every neuron saw at its turn"""
    LP, LQ, logpi = (np.asarray(v, dtype=np.float64) for v in (LP, LQ, logpi))
    K = check_blocks(LP.shape[0])
    Af = (np.asarray(A) != 0).astype(np.float64)
    N = Af.shape[0]
    assert Af.shape == (N, N) and LP.shape == LQ.shape == (K, K) and logpi.shape == (K,) and len(u) == N
    ATf = np.ascontiguousarray(Af.T)
    z = _labels(z, K, N).copy()
    nk = np.bincount(z, minlength=K).astype(np.float64)
    lps = np.empty((N, K))
    for n in range(N):
        zn, self_edge = z[n], Af[n, n]
        cin = np.bincount(z, weights=Af[n], minlength=K)
        cout = np.bincount(z, weights=ATf[n], minlength=K)
        cin[zn] -= self_edge
        cout[zn] -= self_edge
        nk[zn] -= 1.0                                 # cnt over the partners m != n
        lp = _lp_of_counts(nk, cin, cout, LP, LQ, logpi)
        lps[n] = lp
        k = decide(lp, u[n], exp)
        nk[k] += 1.0
        z[n] = k
    return (z, lps) if return_lp else z


def replay_lp(A, z_before, z_after, tables):
    """lp (N, K) of every step of a scan that went from z_before to z_after: step n saw z_after[:n] and z_before[n + 1:]"""
    LP, LQ, logpi = (np.asarray(v, dtype=np.float64) for v in tables)
    K = LP.shape[0]
    Af = (np.asarray(A) != 0).astype(np.float64)
    N = Af.shape[0]
    zb, za = _labels(z_before, K, N), _labels(z_after, K, N)
    Zb, Za = np.zeros((N, K)), np.zeros((N, K))
    Zb[np.arange(N), zb] = 1.0
    Za[np.arange(N), za] = 1.0
    # (sums of at most N ones: exact in fp64 whatever the order)
    cin = np.tril(Af, -1).dot(Za) + np.triu(Af, 1).dot(Zb)
    cout = np.tril(Af.T, -1).dot(Za) + np.triu(Af.T, 1).dot(Zb)
    cnt = (np.cumsum(Za, axis=0) - Za) + (np.cumsum(Zb[::-1], axis=0)[::-1] - Zb)
    return _lp_of_counts(cnt, cin, cout, LP, LQ, logpi)


def block_counts_host(A, z, K):
    """(M (K, K), n (K,), d) int64: edges between blocks off the diagonal, block sizes, self-connections"""
    K = check_blocks(K)
    Ab = np.asarray(A) != 0
    N = Ab.shape[0]
    z = _labels(z, K, N)
    Z = np.zeros((N, K))
    Z[np.arange(N), z] = 1.0
    off = Ab.astype(np.float64)
    off[np.arange(N), np.arange(N)] = 0.0
    M = Z.T.dot(off).dot(Z)
    return np.rint(M).astype(np.int64), np.bincount(z, minlength=K).astype(np.int64), int(np.count_nonzero(Ab[np.arange(N), np.arange(N)]))


def rho_of(P, z, rho_self):
    """the (N, N) connection probabilities as pushed: P[z_n][z_m] off the diagonal, rho_self on it"""
    rho = np.asarray(P)[z][:, z]
    rho[np.diag_indices(len(z))] = rho_self
    return rho


def sbm_host(A, z, K, rng, a_0=1.0, b_0=1.0, alpha=1.0, a_self=1.0, b_self=1.0, rho_self=None, seed=0, sweep=0, u=None, driver=None):
    """the whole update -> dict(z, P, pi, rho_self, M, n, d).  u: the scan's uniforms (default: scan_uniforms(seed, sweep, N)).  driver: a
    DeviceSBM that takes the counts and the scan to the device (it draws from the Philox stream itself: u must be None then)"""
    K = check_blocks(K)
    A = np.asarray(A) != 0
    N = A.shape[0]
    z = _labels(z, K, N)
    if driver is not None:
        assert u is None, "the device scan draws from the Philox stream (seed, sweep)"
        driver.load(A)
        M, nk, d = driver.counts(z)
    else:
        M, nk, d = block_counts_host(A, z, K)
    pairs = np.outer(nk, nk) - np.diag(nk)
    P = rng.beta(a_0 + M, b_0 + pairs - M)
    rho_self = float(rng.beta(a_self + d, b_self + N - d)) if rho_self is None else float(rho_self)
    pi = rng.dirichlet(alpha / K + nk)
    P, pi = clamp(P, pi)
    if K > 1:
        LP, LQ, logpi = tables(P, pi)
        if driver is not None:
            z = driver.scan(z, LP, LQ, logpi, seed, sweep)
        else:
            z = sbm_scan_host(A, z, LP, LQ, logpi, scan_uniforms(seed, sweep, N) if u is None else u)
    return dict(z=z, P=P, pi=pi, rho_self=rho_self, M=M, n=nk, d=d)


def adjusted_rand(a, b):
    """the adjusted Rand index of two partitions given as label vectors (1.0 for identical partitions, about 0 for independent ones)"""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    assert a.shape == b.shape
    _, ai = np.unique(a, return_inverse=True)
    _, bi = np.unique(b, return_inverse=True)
    table = np.zeros((ai.max() + 1, bi.max() + 1), dtype=np.int64) if a.size else np.zeros((1, 1), dtype=np.int64)
    np.add.at(table, (ai, bi), 1)

    def pairs(x):
        return (x * (x - 1) // 2).sum()
    s, sa, sb, tot = pairs(table), pairs(table.sum(axis=1)), pairs(table.sum(axis=0)), a.size * (a.size - 1) // 2
    if tot == 0:
        return 1.0
    expected = sa * sb / float(tot)
    top = 0.5 * (sa + sb)
    return 1.0 if top == expected else float((s - expected) / (top - expected))


# ---- the device drivers ----------------------------------------------------------------------------------------------------------------------
class DeviceSBM(object):
    """the counts and the scan of an (N, K) model on one device: the gathered A goes up as one byte per cell (1 MB at N = 1024) -- one path for
    one rank, for many ranks and for a shard override, since every rank holds the whole (A, W) after the gather"""

    def __init__(self, N, K, device=None, keep_lp=False):
        import torch
        self.N, self.K = int(N), check_blocks(K)
        if not 0 <= self.N <= MAX_N:
            raise ValueError("N = %d: the scan takes at most %d neurons" % (N, MAX_N))
        self.dev, _ = _device("the block-model update", device)
        N, K, dev = self.N, self.K, self.dev
        self.A = torch.zeros((N, N), dtype=torch.uint8, device=dev)
        self.z = torch.zeros(N, dtype=torch.int32, device=dev)
        self.LP, self.LQ = (torch.zeros((K, K), dtype=torch.float64, device=dev) for _ in range(2))
        self.logpi = torch.zeros(K, dtype=torch.float64, device=dev)
        self.lp = torch.zeros((N, K), dtype=torch.float64, device=dev) if keep_lp else None
        self.work = torch.zeros(max(1, int(_lib.load().pgl_sbm_work_bytes(N))), dtype=torch.uint8, device=dev)
        self.counts_out = torch.zeros(K * K + K + 1, dtype=torch.int64, device=dev)

    def _stream(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def load(self, A):
        import torch
        A = np.ascontiguousarray(np.asarray(A) != 0)
        assert A.shape == (self.N, self.N)
        self.A.copy_(torch.from_numpy(A.view(np.uint8)))

    def counts(self, z):
        """block_counts_host of the loaded A"""
        import torch
        N, K = self.N, self.K
        self.z.copy_(torch.from_numpy(np.asarray(z, dtype=np.int32)))
        out = self.counts_out
        with torch.cuda.device(self.dev):
            _lib.call("pgl_sbm_block_counts", A=_lib.ptr(self.A), z=_lib.ptr(self.z), M=_lib.ptr(out), nk=_lib.ptr(out[K * K:]),
                      diag=_lib.ptr(out[K * K + K:]), N=N, K=K, lda=N, hip_stream=self._stream())
        h = out.cpu().numpy()
        return h[:K * K].reshape(K, K).copy(), h[K * K:K * K + K].copy(), int(h[K * K + K])

    def scan(self, z, LP, LQ, logpi, seed, sweep):
        """sbm_scan_host of the loaded A on the uniforms of (seed, sweep) -> z (int64); self.lp then holds the steps' lp (keep_lp)"""
        import torch
        N, K = self.N, self.K
        self.z.copy_(torch.from_numpy(np.asarray(z, dtype=np.int32)))
        for d, h in ((self.LP, LP), (self.LQ, LQ), (self.logpi, logpi)):
            d.copy_(torch.from_numpy(np.array(h, dtype=np.float64).reshape(d.shape)))
        with torch.cuda.device(self.dev):
            _lib.call("pgl_sbm_scan", A=_lib.ptr(self.A), z=_lib.ptr(self.z), LP=_lib.ptr(self.LP), LQ=_lib.ptr(self.LQ), logpi=_lib.ptr(self.logpi),
                      lp_out=_lib.ptr(self.lp), work=_lib.ptr(self.work), N=N, K=K, lda=N, seed=int(seed) & (2 ** 64 - 1),
                      sweep=int(sweep) & (2 ** 64 - 1), hip_stream=self._stream())
        return self.z.cpu().numpy().astype(np.int64)


class _DeviceFold(object):
    """BlockStructure's accumulators on the device (pgl_sbm_fold)"""

    def __init__(self, N, K, device):
        import torch
        self.N, self.K = N, K
        self.dev, _ = _device("block_structure", device)
        self.coassign = torch.zeros((N, N), dtype=torch.int32, device=self.dev)      # (the bits of a uint32: the counts stay far below 2^31)
        self.rho_sum = torch.zeros((N, N), dtype=torch.float64, device=self.dev)
        self.z = torch.zeros(N, dtype=torch.int32, device=self.dev)
        self.P = torch.zeros((K, K), dtype=torch.float64, device=self.dev)

    def reset(self):
        self.coassign.zero_()
        self.rho_sum.zero_()

    def fold(self, z, P, rho_self):
        import torch
        self.z.copy_(torch.from_numpy(np.asarray(z, dtype=np.int32)))
        self.P.copy_(torch.from_numpy(np.ascontiguousarray(P, dtype=np.float64)))
        with torch.cuda.device(self.dev):
            _lib.call("pgl_sbm_fold", z=_lib.ptr(self.z), P=_lib.ptr(self.P), rho_self=float(rho_self), coassign=_lib.ptr(self.coassign),
                      rho_sum=_lib.ptr(self.rho_sum), N=self.N, K=self.K,
                      hip_stream=ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))

    def read(self):
        return self.coassign.cpu().numpy().astype(np.int64), self.rho_sum.cpu().numpy()


class _HostFold(object):
    """the same accumulators in NumPy"""

    def __init__(self, N, K):
        self.N = N
        self.reset()

    def reset(self):
        self.coassign = np.zeros((self.N, self.N), dtype=np.uint32)
        self.rho_sum = np.zeros((self.N, self.N))

    def fold(self, z, P, rho_self):
        z = np.asarray(z)
        self.coassign += (z[:, None] == z[None, :]).astype(np.uint32)
        self.rho_sum += rho_of(P, z, rho_self)                      # one IEEE addition per cell and sample

    def read(self):
        return self.coassign.astype(np.int64), self.rho_sum.copy()


def connected_components(adj):
    """labels (N,) of the connected components of a symmetric boolean adjacency, numbered by their smallest member"""
    adj = np.asarray(adj, dtype=bool)
    N = adj.shape[0]
    label = np.full(N, -1, dtype=np.int64)
    nxt = 0
    for i in range(N):
        if label[i] >= 0:
            continue
        label[i] = nxt
        todo = [i]
        while todo:
            j = todo.pop()
            for k in np.flatnonzero((adj[j] | adj[:, j]) & (label < 0)):
                label[k] = nxt
                todo.append(int(k))
        nxt += 1
    return label


class BlockStructure(object):
    """the label-switching-invariant summary of a chain's partitions (model.block_structure): collect() folds the network's CURRENT (z, P,
    rho_self), once per kept sweep, after resample_model().  Every rank holds the same network, so nothing here is collective."""

    def __init__(self, source, device=None, gpu=False):
        self.source = source             # a model (its network of the moment is read at every collect: set_state replaces it) or a network
        N, K = self.network.N, self.network.K
        self._acc = _DeviceFold(N, K, device) if gpu else _HostFold(N, K)
        self.on_device = bool(gpu)
        self.reset(_acc=False)

    @property
    def network(self):
        return getattr(self.source, "network", self.source)

    def reset(self, _acc=True):
        if _acc:
            self._acc.reset()
        self.count = 0
        self.occupied = []               # the trace of the number of non-empty blocks

    def collect(self):
        net = self.network
        self._acc.fold(net.z, net.P, net.rho_diag)
        self.count += 1
        self.occupied.append(int(np.count_nonzero(net.block_sizes)))

    def _read(self):
        if self.count < 1:
            raise RuntimeError("no sample folded so far")
        return self._acc.read()

    @property
    def coassign(self):
        """(N, N): the fraction of the collected partitions in which i and j share a block"""
        return self._read()[0] / float(self.count)

    @property
    def rho_mean(self):
        """(N, N): the mean of the connection probabilities as pushed"""
        return self._read()[1] / float(self.count)

    def consensus(self, threshold=0.5):
        """labels (N,): the connected components of coassign > threshold"""
        return connected_components(self.coassign > threshold)
