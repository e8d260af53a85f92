"""Time of posterior predictive simulation (pgl_simulate) at one shape against the single-trajectory generate() path in the same run:
kernel time per bin and per replicate-bin for R = 1, 4, 16, 64 replicates per launch (paths not kept), the kernel time per bin of pgl_generate,
the batching ratio (R x generate's time per bin) / (one R-replicate launch's time per bin), and end to end model.simulate(T, replicates=16,
keep_paths=False) against model.generate(T).  HIP events around the kernel calls, wall time around the model calls; one warm-up, mean of --reps.

    python tools/probe_simulate.py [--N 1024] [--B 5] [--L 100] [--T 100000] [--bins 2000] [--reps 5] [--out profiles/simulate_probe.json]
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


def stats(ms, bins, R=1):
    us = np.asarray(ms) * 1e3 / bins
    return dict(us_per_bin_mean=float(us.mean()), us_per_bin_min=float(us.min()), us_per_bin_max=float(us.max()),
                us_per_replicate_bin=float(us.mean() / R), bins_per_launch=bins)


def kernels(N, B, L, bins, reps, Rs):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    f64 = dict(dtype=torch.float64, device=dev)
    Wm = torch.from_numpy(rng.standard_normal((N, N * B)) / np.sqrt(N) * (rng.random((N, N * B)) < 0.5)).to(dev)
    bias = torch.from_numpy(-2.0 + 0.3 * rng.standard_normal(N)).to(dev)
    from pyglm_amd.utils.basis import cosine_basis
    basis = torch.from_numpy(np.ascontiguousarray(cosine_basis(B, L=L) / L)).to(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {}
    # the yardstick: pgl_generate, one trajectory, host-drawn uniforms already on the device
    U = torch.rand(bins, N, **f64)
    ring, Y = torch.zeros(L, N, **f64), torch.empty(bins, N, **f64)
    work = torch.zeros(lib.pgl_generate_work_bytes(N, B), dtype=torch.uint8, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    t = [0]

    def gen():
        call("pgl_generate", ptr(Wm), ptr(bias), ptr(basis), N, B, L, 0, 0.0, ptr(U), ptr(ring), ptr(Y), t[0], bins, ptr(work), ptr(status), st)
        t[0] += bins
    gen()
    out["pgl_generate"] = stats([timed(gen) for _ in range(reps)], bins)
    assert int(status[0]) == 0
    kind = torch.zeros(N, dtype=torch.int32, device=dev)
    par = torch.zeros(N, **f64)
    for R in Rs:
        nb = max(50, min(bins, simulate.chunk_bins(N, B, R), bins * 8 // max(R, 8)))
        ring = torch.zeros(R, L, N, **f64)
        s, ss = torch.zeros(R, N, **f64), torch.zeros(R, N, **f64)
        work = torch.zeros(lib.pgl_simulate_work_bytes(N, B, R), dtype=torch.uint8, device=dev)
        status.zero_()
        t = [0]

        def sim():
            call("pgl_simulate", ptr(Wm), ptr(bias), ptr(basis), N, B, L, ptr(kind), ptr(par), R, 0, 1, ptr(ring), None, 0, ptr(s), ptr(ss),
                 t[0], nb, ptr(work), ptr(status), st)
            t[0] += nb
        sim()
        res = stats([timed(sim) for _ in range(reps)], nb, R)
        assert int(status[0]) == 0, status.tolist()
        res["mean_rate"] = float(s.sum() / (R * N * t[0]))
        res["batching_ratio_R_x_generate_over_launch"] = R * out["pgl_generate"]["us_per_bin_mean"] / res["us_per_bin_mean"]
        out["pgl_simulate_R%d" % R] = res
    return out


def end_to_end(N, B, L, T, R):
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
    model.simulate(200, replicates=R, keep_paths=False, gpu=True)
    model.generate(keep=False, T=200, gpu=True)
    out["simulate_R%d_no_paths_s" % R] = [wall(lambda: model.simulate(T, replicates=R, seed=k, keep_paths=False, gpu=True)) for k in range(2)]
    out["simulate_R1_keep_paths_s"] = [wall(lambda: model.simulate(T, replicates=1, seed=k, keep_paths=True, gpu=True)) for k in range(2)]
    out["generate_s"] = [wall(lambda: model.generate(keep=False, T=T, gpu=True)) for _ in range(2)]
    out["replicate_bins_per_second_simulate"] = R * T / float(np.mean(out["simulate_R%d_no_paths_s" % R]))
    out["bins_per_second_generate"] = T / float(np.mean(out["generate_s"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--bins", type=int, default=2000, help="bins per timed launch (fewer for many replicates)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--R", type=int, nargs="*", default=[1, 4, 16, 64])
    ap.add_argument("--no-model", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = dict(N=args.N, B=args.B, L=args.L, T=args.T, reps=args.reps, device=torch.cuda.get_device_name(0), boxes=1, source_hash=_lib.source_hash(),
               unit="kernels: HIP events around one launch, microseconds per bin; model: wall seconds of the call")
    out["kernels"] = kernels(args.N, args.B, args.L, args.bins, args.reps, args.R)
    torch.cuda.empty_cache()
    if not args.no_model:
        out["model"] = end_to_end(args.N, args.B, args.L, args.T, 16)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
