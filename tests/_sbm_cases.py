"""Inputs shared by tests/test_sbm_host.py and tests/test_gpu_sbm.py: the scan cases (adjacency, starting labels, tables, uniforms) and the
rule that says which draws a one-ulp difference between two exp implementations may turn."""
import functools

import numpy as np

from pyglm_amd import sbm

SCAN_N = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2500)     # no partner; a wave edge; one, exactly one and several passes of the workgroup
SCAN_K = (1, 2, 3, 32)
SEED, SWEEP = 0x5EEDB10C5, 7
EPS = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def adjacency(N):
    """(N, N) uint8 at density 0.1, read-only"""
    A = (np.random.default_rng(1000 + N).random((N, N)) < 0.1).astype(np.uint8)
    A.setflags(write=False)
    return A


def padded(A, lda):
    """A in rows of lda bytes, the padding filled with garbage (non-zero bytes the kernels must never read as edges)"""
    N = A.shape[0]
    out = np.random.default_rng(7).integers(1, 256, size=(max(N, 1), lda), dtype=np.uint8)
    out[:N, :N] = A
    return out[:N]


@functools.lru_cache(maxsize=None)
def scan_case(N, K, clamps=False):
    """(z0 (N,) int64, (LP, LQ, logpi), u (N,)) of a case: P log-spread over [1e-6, 1 - 1e-6], or sitting at the clamps"""
    rng = np.random.default_rng(100 * N + K + (50000 if clamps else 0))
    z0 = rng.integers(0, K, size=N).astype(np.int64)
    if clamps:
        P = rng.choice(np.array([0.0, 1.0, 1e-320, 0.5]), size=(K, K))
        pi = rng.choice(np.array([0.0, 1e-320, 1.0]), size=K)
    else:
        lo = 10.0 ** rng.uniform(-6, np.log10(0.5), size=(K, K))
        P = np.where(rng.random((K, K)) < 0.5, lo, 1.0 - lo)
        pi = rng.dirichlet(np.ones(K))
    t = sbm.tables(P, pi)
    u = sbm.scan_uniforms(SEED, SWEEP, N)
    for v in (z0, u) + t:
        v.setflags(write=False)
    return z0, t, u


def host_decisions(lp, u, exp=np.exp):
    """(labels (N,), turnable (N,) bool) of the host rule applied to every row of lp (N, K) and its uniform: turnable marks the draws with
    |u c_{K-1} - c_k| <= 8 K 2^-53 c_{K-1} for some k, which a one-ulp difference in exp could decide the other way"""
    lp = np.asarray(lp, dtype=np.float64)
    N, K = lp.shape
    e = np.asarray(exp(lp - lp.max(axis=1, keepdims=True)), dtype=np.float64)
    c = np.add.accumulate(e, axis=1)
    t = (u * c[:, -1])[:, None]
    hit = t < c
    labels = np.where(hit.any(axis=1), hit.argmax(axis=1), K - 1)
    turnable = (np.abs(t - c) <= 8 * K * EPS * c[:, -1:]).any(axis=1)
    return labels, turnable


def exp_long_double(x):
    """exp evaluated in long double and rounded to double once"""
    return np.exp(np.asarray(x, dtype=np.longdouble)).astype(np.float64)
