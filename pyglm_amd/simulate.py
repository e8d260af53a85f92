"""Forward simulation of a population model on the GPU: the device path of `NetworkGLM.generate()` (reference pyglm/models.py:98-151).

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
from ._lib import PglError, call, ptr

OBS_BERNOULLI, OBS_GAUSSIAN = 0, 1
MAX_CHUNK_BINS = 16384          # bins per launch at most
CHUNK_DRAWS = 1 << 22           # host draws per chunk (N * bins): 32 MiB of U
CHUNK_MACS = 1 << 33            # multiply-adds per launch (N * N * B * bins): no single launch runs for long
X_BLOCK_BYTES = 1 << 30         # device scratch of the design matrix, formed in blocks of rows


def chunk_bins(N, B):
    """bins per launch for an N-neuron, B-basis model"""
    return int(max(1, min(MAX_CHUNK_BINS, CHUNK_DRAWS // N, CHUNK_MACS // (N * N * B))))


def generate(Wm, bias, basis, T, obs, noise_scale=0.0, device=None, verbose=False, intvl=10, chunk=None):
    """(X (T, N, B), Y (T, N)) of the host loop at pyglm_amd/models.py (generate), from the current state of NumPy's global generator,
    which is left where that loop leaves it.  Wm (N, N*B), bias (N,), basis (L, B) as the model holds them (basis row 0 = previous bin);
    obs OBS_BERNOULLI or OBS_GAUSSIAN (noise_scale = sqrt(eta) of the regression whose rvs the loop calls)."""
    import torch
    if not torch.cuda.is_available():
        raise PglError("the device path of generate() needs a ROCm GPU (torch.cuda.is_available() is False)")
    _lib.load()
    Wm = np.ascontiguousarray(Wm, dtype=np.float64)
    basis = np.ascontiguousarray(basis, dtype=np.float64)
    N = Wm.shape[0]
    L, B = basis.shape
    assert Wm.shape == (N, N * B) and obs in (OBS_BERNOULLI, OBS_GAUSSIAN)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    Tc = int(chunk) if chunk else chunk_bins(N, B)
    draw = npr.rand if obs == OBS_BERNOULLI else npr.randn
    with torch.cuda.device(dev):
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        f64 = dict(dtype=torch.float64, device=dev)
        Wm_d = torch.from_numpy(Wm).to(dev)
        bias_d = torch.from_numpy(np.ascontiguousarray(bias, dtype=np.float64).reshape(N)).to(dev)
        basis_d = torch.from_numpy(basis).to(dev)
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
            call("pgl_generate", ptr(Wm_d), ptr(bias_d), ptr(basis_d), N, B, L, obs, float(noise_scale), ptr(U_d), ptr(ring),
                 ptr(Y_d[t0:t0 + n]), t0, n, ptr(work), ptr(status), st)
            status_h.copy_(status, non_blocking=True)
            if t0 + n < T:
                U = draw(min(Tc, T - t0 - n), N)            # the next chunk's draws, while this one runs
            torch.cuda.current_stream(dev).synchronize()
            if int(status_h[0]):
                raise PglError("pgl_generate: a grid barrier timed out at bin %d (chunk of bins %d..%d)" % (int(status_h[1]), t0, t0 + n - 1))
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
            call("pgl_design_matrix", ptr(Y_d[r0 - h:]), N, ptr(basis_d), ptr(Xs), D + 1, None, 0, r1 - r0 + h, N, B, L, 0, st)
            X2[r0:r1].copy_(Xs[h:h + r1 - r0, :D])
    return X, Y
