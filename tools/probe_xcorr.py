"""Time of the lagged products of the cross-correlogram check (pgl_lagged_products) at one shape: the fold of one simulate() chunk in the int8
mode and in the fp64 mode (the contraction kernel the project had before: the baseline), against the pgl_simulate launch that produced the
chunk, for R = 1 and 8 replicates; the int8 rate against pgl_ubench_mfma kind 0 of the same run; and model.simulate(T, replicates=8,
keep_paths=False) end to end with and without lags.  HIP events around the calls, wall time around the model calls; one warm-up, mean of --reps.

    python tools/probe_xcorr.py [--N 1024] [--B 5] [--L 100] [--K 50] [--T 100000] [--reps 5] [--out profiles/xcorr_probe.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyglm_amd import _lib, simulate  # noqa: E402
from pyglm_amd._lib import call, ptr  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def ms_stats(ms):
    ms = np.asarray(ms)
    return dict(ms_mean=float(ms.mean()), ms_min=float(ms.min()), ms_max=float(ms.max()))


def kernels(N, B, L, K, reps, Rs):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    f64 = dict(dtype=torch.float64, device=dev)
    from pyglm_amd.utils.basis import cosine_basis
    Wm = torch.from_numpy(rng.standard_normal((N, N * B)) / np.sqrt(N) * (rng.random((N, N * B)) < 0.5)).to(dev)
    bias = torch.from_numpy(-2.0 + 0.3 * rng.standard_normal(N)).to(dev)
    basis = torch.from_numpy(np.ascontiguousarray(cosine_basis(B, L=L) / L)).to(dev)
    kind = torch.zeros(N, dtype=torch.int32, device=dev)
    par = torch.zeros(N, **f64)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {}
    for R in Rs:
        rows = simulate.chunk_bins(N, B, R)
        Tb = K - 1 + rows
        buf = torch.zeros(R, Tb, N, **f64)
        ring = torch.zeros(R, L, N, **f64)
        s, ss = torch.zeros(R, N, **f64), torch.zeros(R, N, **f64)
        S = torch.zeros(R, K, N, N, **f64)
        work = torch.zeros(lib.pgl_simulate_work_bytes(N, B, R), dtype=torch.uint8, device=dev)
        lwork = torch.empty(lib.pgl_lagged_work_bytes(N, K, R, rows), dtype=torch.uint8, device=dev)
        status, lstatus = torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
        t = [0]

        def sim():
            if K > 1:
                buf[:, :K - 1] = buf[:, rows:rows + K - 1].clone()
            call("pgl_simulate", ptr(Wm), ptr(bias), ptr(basis), N, B, L, ptr(kind), ptr(par), R, 0, 1, ptr(ring), ptr(buf[0, K - 1:]), Tb * N,
                 ptr(s), ptr(ss), t[0], rows, ptr(work), ptr(status), st)
            t[0] += rows

        def fold(mode):
            call("pgl_lagged_products", ptr(buf[0, K - 1:]), N, Tb * N, rows, K - 1, N, K, R, ptr(S), K * N * N, 1, mode, ptr(lwork), ptr(lstatus), st)

        sim()
        res = dict(rows=rows, ops=2.0 * N * N * K * rows * R, S_bytes=8 * R * K * N * N)
        res["pgl_simulate"] = ms_stats([timed(sim) for _ in range(reps)])
        for name, mode in (("int8", simulate.LAG_I8), ("fp64", simulate.LAG_F64)):
            fold(mode)
            res[name] = ms_stats([timed(lambda: fold(mode)) for _ in range(reps)])
            res[name]["ops_per_s"] = res["ops"] / (res[name]["ms_mean"] * 1e-3)
            res[name]["S_GB_per_s_read_and_write"] = 2 * res["S_bytes"] / (res[name]["ms_mean"] * 1e-3) / 1e9
        assert int(status[0]) == 0 and int(lstatus[0]) == 0, (status.tolist(), lstatus.tolist())
        res["mean_rate"] = float(s.sum() / (R * N * t[0]))
        res["int8_speedup_over_fp64"] = res["fp64"]["ms_mean"] / res["int8"]["ms_mean"]
        res["int8_fold_over_simulate_launch"] = res["int8"]["ms_mean"] / res["pgl_simulate"]["ms_mean"]
        out["R%d" % R] = res
        del buf, S, lwork
        torch.cuda.empty_cache()
    rate, ms = ctypes.c_double(0.0), ctypes.c_double(0.0)
    call("pgl_ubench_mfma", 0, 0.5, ctypes.byref(rate), ctypes.byref(ms), st)
    out["ubench_mfma_i8_ops_per_s"] = rate.value
    for R in Rs:
        out["R%d" % R]["int8"]["fraction_of_ubench_mfma_i8"] = out["R%d" % R]["int8"]["ops_per_s"] / rate.value
    return out


def end_to_end(N, B, L, K, T, R):
    from pyglm_amd.models import NonlinearAutoregressiveModel
    from pyglm_amd.regression import SparseBernoulliRegression
    from pyglm_amd.utils.basis import cosine_basis
    np.random.seed(0)
    rng = np.random.default_rng(0)
    regs = [SparseBernoulliRegression(N, B, rho=0.5, mu_b=-2.0, S_b=0.1) for _ in range(N)]
    model = NonlinearAutoregressiveModel(N, regs, basis=cosine_basis(B, L=L) / L)
    A, W, b = model._adopt_state()
    A[...] = True
    W[...] = rng.standard_normal(W.shape) / np.sqrt(N)
    b[:, 0] = -2.0 + 0.3 * rng.standard_normal(N)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    out = {}
    model.simulate(2 * K + 300, replicates=R, keep_paths=False, gpu=True, lags=K, lagged_on_device=True)
    out["simulate_s"] = [wall(lambda: model.simulate(T, replicates=R, seed=k, keep_paths=False, gpu=True)) for k in range(2)]
    out["simulate_lags_s"] = [wall(lambda: model.simulate(T, replicates=R, seed=k, keep_paths=False, gpu=True, lags=K, lagged_on_device=True))
                              for k in range(2)]
    plain, lagged = float(np.mean(out["simulate_s"])), float(np.mean(out["simulate_lags_s"]))
    out["lags_add_s"] = lagged - plain
    out["lags_add_over_simulate"] = (lagged - plain) / plain
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--R", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--no-model", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = dict(N=args.N, B=args.B, L=args.L, K=args.K, T=args.T, reps=args.reps, device=torch.cuda.get_device_name(0), boxes=1,
               source_hash=_lib.source_hash(),
               unit="kernels: HIP events around one call (a fold = every launch of pgl_lagged_products), milliseconds; model: wall seconds of "
                    "the call, lagged products left on the device")
    out["kernels"] = kernels(args.N, args.B, args.L, args.K, args.reps, args.R)
    torch.cuda.empty_cache()
    if not args.no_model:
        out["model"] = end_to_end(args.N, args.B, args.L, args.K, args.T, 8)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
