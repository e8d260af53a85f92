"""The block-model kernels (pgl_sbm.hip) against the law in pyglm_amd/sbm.py: the scan bit for bit along the device's own path, the counts
and the fold exactly, the entry points' refusals, and a model chain whose network updates run on the device against one that scans on the host."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import _sbm_cases as C

GUARD = 64               # sentinel elements behind every output buffer
SENT_F, SENT_I, SENT_B = -12345.678, -77, 0xA5


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).cuda()


class ScanBuffers(object):
    """the device buffers of one pgl_sbm_scan call, every output followed by GUARD sentinels"""

    def __init__(self, A, lda, z0, tables, K):
        import torch
        from pyglm_amd import _lib
        N = A.shape[0]
        self.N, self.K, self.lda = N, K, lda
        self.A = _dev(C.padded(A, lda))
        self.tables = [_dev(t) for t in tables]
        self.z = torch.full((N + GUARD,), SENT_I, dtype=torch.int32, device="cuda")
        self.z[:N] = _dev(np.asarray(z0, dtype=np.int32))
        self.lp = torch.full((N * K + GUARD,), SENT_F, dtype=torch.float64, device="cuda")
        self.wb = int(_lib.load().pgl_sbm_work_bytes(N))
        assert self.wb >= N * N
        self.work = torch.full((self.wb + GUARD,), SENT_B, dtype=torch.uint8, device="cuda")

    def scan(self, seed=C.SEED, sweep=C.SWEEP, lp=True, **override):
        from pyglm_amd import _lib
        kw = dict(A=_lib.ptr(self.A), z=_lib.ptr(self.z), LP=_lib.ptr(self.tables[0]), LQ=_lib.ptr(self.tables[1]), logpi=_lib.ptr(self.tables[2]),
                  lp_out=_lib.ptr(self.lp) if lp else None, work=_lib.ptr(self.work), N=self.N, K=self.K, lda=self.lda, seed=seed, sweep=sweep,
                  hip_stream=_stream())
        kw.update(override)
        return _lib.load().pgl_sbm_scan(*[kw[k] for k in _lib.SBM_PARAMS["pgl_sbm_scan"]])

    def read(self):
        import torch
        torch.cuda.synchronize()
        z, lp, work = self.z.cpu().numpy(), self.lp.cpu().numpy(), self.work.cpu().numpy()
        N, K = self.N, self.K
        assert np.all(z[N:] == SENT_I) and np.all(lp[N * K:] == SENT_F) and np.all(work[self.wb:] == SENT_B), "written behind a buffer"
        return z[:N].astype(np.int64), lp[:N * K].reshape(N, K), work[:N * N].reshape(N, N)


def check_scan(N, K, lda, clamps=False):
    from pyglm_amd import sbm
    A = C.adjacency(N)
    z0, t, u = C.scan_case(N, K, clamps)
    buf = ScanBuffers(A, lda, z0, t, K)
    assert buf.scan() == 0
    z1, lp, AT = buf.read()
    assert z1.min() >= 0 and z1.max() < K
    assert np.array_equal(AT, A.T)                                   # the transpose the scan read its columns from: 0 / 1 bytes
    want = sbm.replay_lp(A, z0, z1, t)
    assert np.array_equal(lp.view(np.int64), want.view(np.int64)), "lp differs from the replay along the device's path in %d entries" % np.count_nonzero(lp != want)
    labels, turnable = C.host_decisions(lp, u)
    wrong = labels != z1
    print("N %d K %d lda %d: %d draws, %d decided otherwise than the host rule, %d of them excused" % (N, K, lda, N, wrong.sum(), (wrong & turnable).sum()))
    assert not np.any(wrong & ~turnable) and wrong.sum() <= 1
    # the same inputs, the same z
    again = ScanBuffers(A, lda, z0, t, K)
    assert again.scan(lp=False) == 0
    z2, lp2, _ = again.read()
    assert np.array_equal(z2, z1) and np.all(lp2 == SENT_F)          # lp_out = NULL: nothing recorded
    return z1


@pytest.mark.parametrize("K", C.SCAN_K)
@pytest.mark.parametrize("N", C.SCAN_N)
def test_scan_against_the_replay(N, K):
    z_tight = check_scan(N, K, N)
    z_padded = check_scan(N, K, N + 3)
    assert np.array_equal(z_tight, z_padded)


@pytest.mark.parametrize("N, K", [(65, 3), (1025, 32)])
def test_scan_at_the_clamps(N, K):
    check_scan(N, K, N + 3, clamps=True)


def test_scan_beyond_the_passes_kept_in_registers():
    """N > 4096: the workgroup's fifth pass on loads its row bytes where it uses them"""
    check_scan(4133, 3, 4133 + 3)


def test_scan_follows_the_host_scan():
    """not only step by step: the whole path is the host definition's on the same Philox uniforms"""
    from pyglm_amd import sbm
    N, K = 1025, 3
    A = C.adjacency(N)
    z0, t, u = C.scan_case(N, K)
    drv = sbm.DeviceSBM(N, K, keep_lp=True)
    drv.load(A)
    z_dev = drv.scan(z0, *t, C.SEED, C.SWEEP)
    z_host, lp_host = sbm.sbm_scan_host(A, z0, *t, u, return_lp=True)
    assert np.array_equal(z_dev, z_host) and np.array_equal(drv.lp.cpu().numpy(), lp_host)


def test_scan_refusals_write_nothing():
    N, K = 65, 3
    A = C.adjacency(N)
    z0, t, _ = C.scan_case(N, K)
    from pyglm_amd import _lib
    for override in (dict(K=0), dict(K=33), dict(N=-1), dict(N=_lib.PGL_SBM_MAX_N + 1), dict(lda=N - 1), dict(A=None), dict(z=None), dict(LP=None),
                     dict(LQ=None), dict(logpi=None), dict(work=None)):
        buf = ScanBuffers(A, N, z0, t, K)
        assert buf.scan(**override) == 1, override
        z, lp, work = buf.read()
        assert np.array_equal(z, z0) and np.all(lp == SENT_F) and np.all(work == SENT_B), override
    for bad in (K, -1, 255, 256):                                    # a z entry outside [0, K): found by the pre-pass
        zb = z0.copy()
        zb[N - 1] = bad
        buf = ScanBuffers(A, N, zb, t, K)
        assert buf.scan() == 1
        assert b"outside" in _lib.load().pgl_last_error()
        z, lp, work = buf.read()
        assert np.array_equal(z, zb) and np.all(lp == SENT_F) and np.all(work == SENT_B), bad
    buf = ScanBuffers(A, N, z0, t, K)                                # N * K = 0 launches nothing
    assert buf.scan(N=0, lda=0) == 0
    z, lp, work = buf.read()
    assert np.array_equal(z, z0) and np.all(lp == SENT_F) and np.all(work == SENT_B)
    assert _lib.load().pgl_sbm_work_bytes(-1) == 0 and _lib.load().pgl_sbm_work_bytes(_lib.PGL_SBM_MAX_N + 1) == 0


@pytest.mark.parametrize("K", [1, 32])
@pytest.mark.parametrize("N", [1, 65, 1025])
def test_block_counts(N, K):
    import torch
    from pyglm_amd import _lib, sbm
    A = C.adjacency(N)
    z = C.scan_case(N, K)[0]
    want = sbm.block_counts_host(A, z, K)
    for lda in (N, N + 3):
        out = torch.full((K * K + K + 1 + GUARD,), SENT_I, dtype=torch.int64, device="cuda")
        A_d, z_d = _dev(C.padded(A, lda)), _dev(z.astype(np.int32))      # (named: they must outlive the call)
        _lib.call("pgl_sbm_block_counts", A=_lib.ptr(A_d), z=_lib.ptr(z_d), M=_lib.ptr(out),
                  nk=_lib.ptr(out[K * K:]), diag=_lib.ptr(out[K * K + K:]), N=N, K=K, lda=lda, hip_stream=_stream())
        h = out.cpu().numpy()
        assert np.all(h[K * K + K + 1:] == SENT_I)
        assert np.array_equal(h[:K * K].reshape(K, K), want[0]) and np.array_equal(h[K * K:K * K + K], want[1]) and h[K * K + K] == want[2]
    drv = sbm.DeviceSBM(N, K)
    drv.load(A)
    got = drv.counts(z)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    lib = _lib.load()
    assert lib.pgl_sbm_block_counts(None, None, None, None, None, N, K, N, None) == 1
    assert lib.pgl_sbm_block_counts(_lib.ptr(drv.A), _lib.ptr(drv.z), _lib.ptr(drv.counts_out), _lib.ptr(drv.counts_out), _lib.ptr(drv.counts_out), N, 33, N, None) == 1


@pytest.mark.parametrize("N, K", [(1, 1), (65, 3), (1025, 32)])
def test_fold_over_three_samples(N, K):
    from pyglm_amd import _lib, sbm
    rng = np.random.default_rng(N)
    dev, host = sbm._DeviceFold(N, K, None), sbm._HostFold(N, K)
    for _ in range(3):
        z, P, rho_self = rng.integers(0, K, size=N), rng.random((K, K)), rng.random()
        dev.fold(z, P, rho_self)
        host.fold(z, P, rho_self)
    (cd, rd), (ch, rh) = dev.read(), host.read()
    assert np.array_equal(cd, ch) and cd.max() == 3 and np.array_equal(rd.view(np.int64), rh.view(np.int64))
    assert _lib.load().pgl_sbm_fold(_lib.ptr(dev.z), _lib.ptr(dev.P), 0.5, _lib.ptr(dev.coassign), None, N, K, None) == 1
    assert _lib.load().pgl_sbm_fold(_lib.ptr(dev.z), _lib.ptr(dev.P), 0.5, _lib.ptr(dev.coassign), _lib.ptr(dev.rho_sum), N, 0, None) == 1
    assert np.array_equal(dev.read()[0], ch)


def _model(network_gpu, N=16, B=2, T=2000, seed=1):
    from pyglm_amd import models as M
    from pyglm_amd import networks as NW
    np.random.seed(0)
    net = NW.SBMSparseNetwork(N, B, K=4)
    model = M.SparseBernoulliGLM(N, B=B, network=net, regression_kwargs=dict(S_w=1.0, mu_b=-1.0), seed=seed)
    model.network_gpu = network_gpu
    model.add_data((np.random.default_rng(3).random((T, N)) < 0.2).astype(float))
    return model


def test_model_chain_device_scan_equals_host_scan():
    on, off = _model(None), _model(False)
    assert on._network_device() is not None and off._network_device() is None
    blocks_on, blocks_off = on.block_structure(), off.block_structure(gpu=False)
    assert blocks_on.on_device and not blocks_off.on_device
    for it in range(20):
        on.resample_model()
        off.resample_model()
        if it >= 10:
            blocks_on.collect()
            blocks_off.collect()
    assert on.network._driver is not None and off.network._driver is None
    np.testing.assert_array_equal(on.network.z, off.network.z)
    np.testing.assert_array_equal(on.network.P, off.network.P)
    assert on.network.rho_self == off.network.rho_self
    np.testing.assert_array_equal(on.adjacency, off.adjacency)
    np.testing.assert_allclose(on.weights, off.weights, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(on.biases, off.biases, rtol=1e-7, atol=1e-9)
    assert len(set(np.asarray(on.network.z).tolist())) >= 1 and blocks_on.count == 10
    np.testing.assert_array_equal(blocks_on.coassign, blocks_off.coassign)
    np.testing.assert_array_equal(blocks_on.rho_mean, blocks_off.rho_mean)
    assert blocks_on.occupied == blocks_off.occupied
    # the chain state travels without the device buffers
    st = on.get_state()
    assert st["network"]._driver is None and np.array_equal(st["network"].z, on.network.z)
