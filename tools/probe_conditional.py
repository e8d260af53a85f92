"""Time of conditional simulation (pgl_conditional_simulate) beside posterior predictive simulation (pgl_simulate) in the same run, on one
box: kernel time per bin of the conditional kernel for F = 1, 16, 64, 256 free neurons of an N = 1024, B = 5, L = 100 model and R = 1, 8, 64
replicates (one workgroup per replicate, paths not kept), pgl_simulate's time per bin at the same R, their ratio, and
conditional_check(...).collect() end to end at T = 100 000, F = 16, R = 8.  HIP events around the kernel calls, wall time around collect();
one warm-up, mean of --reps.

    python tools/probe_conditional.py [--N 1024] [--B 5] [--L 100] [--T 100000] [--bins 2000] [--reps 5] [--out profiles/conditional_probe.json]
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
from pyglm_amd.utils.basis import cosine_basis  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms, bins):
    us = np.asarray(ms) * 1e3 / bins
    return dict(us_per_bin_mean=float(us.mean()), us_per_bin_min=float(us.min()), us_per_bin_max=float(us.max()), bins_per_launch=bins)


def kernels(N, B, L, bins, reps, Fs, Rs):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    f64 = dict(dtype=torch.float64, device=dev)
    Wm_h = rng.standard_normal((N, N * B)) / np.sqrt(N) * (rng.random((N, N * B)) < 0.5)
    bias_h = -2.0 + 0.3 * rng.standard_normal(N)
    Wm, bias = torch.from_numpy(Wm_h).to(dev), torch.from_numpy(bias_h).to(dev)
    basis = torch.from_numpy(np.ascontiguousarray(cosine_basis(B, L=L) / L)).to(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    out = {}
    for R in Rs:
        # the yardstick of this R: pgl_simulate of the whole population, Bernoulli, paths not kept
        nb = max(50, min(bins, simulate.chunk_bins(N, B, R), bins * 8 // max(R, 8)))
        ring = torch.zeros(R, L, N, **f64)
        s, ss = torch.zeros(R, N, **f64), torch.zeros(R, N, **f64)
        work = torch.zeros(lib.pgl_simulate_work_bytes(N, B, R), dtype=torch.uint8, device=dev)
        kind, par = torch.zeros(N, dtype=torch.int32, device=dev), torch.zeros(N, **f64)
        status.zero_()
        t = [0]

        def sim():
            call("pgl_simulate", ptr(Wm), ptr(bias), ptr(basis), N, B, L, ptr(kind), ptr(par), R, 0, 1, ptr(ring), None, 0, ptr(s), ptr(ss), t[0], nb,
                 ptr(work), ptr(status), st)
            t[0] += nb
        sim()
        ref = stats([timed(sim) for _ in range(reps)], nb)
        assert int(status[0]) == 0, status.tolist()
        out["pgl_simulate_R%d" % R] = ref
        for F in Fs:
            free = np.sort(rng.choice(N, F, replace=False))
            cols = (free[:, None] * B + np.arange(B)).ravel()
            Wff = torch.from_numpy(np.ascontiguousarray(Wm_h[free][:, cols])).to(dev)
            base = torch.from_numpy(bias_h[free] + 0.3 * rng.standard_normal((bins, F))).to(dev)
            neuron = torch.from_numpy(free.astype(np.int32)).to(dev)
            kf, pf = torch.zeros(F, dtype=torch.int32, device=dev), torch.zeros(F, **f64)
            ringf = torch.zeros(R, L, F, **f64)
            sf, ssf = torch.zeros(R, F, **f64), torch.zeros(R, F, **f64)
            status.zero_()
            tf = [0]

            def cond():
                call("pgl_conditional_simulate", ptr(Wff), ptr(base), F, ptr(basis), F, B, L, ptr(kf), ptr(pf), ptr(neuron), R, 0, 1, ptr(ringf), None, 0,
                     None, 0, ptr(sf), ptr(ssf), tf[0], bins, ptr(status), st)
                tf[0] += bins
            cond()
            res = stats([timed(cond) for _ in range(reps)], bins)
            assert int(status[0]) == 0, status.tolist()
            res["mean_rate"] = float(sf.sum() / (R * F * tf[0]))
            res["pgl_simulate_over_conditional"] = ref["us_per_bin_mean"] / res["us_per_bin_mean"]
            out["pgl_conditional_simulate_F%d_R%d" % (F, R)] = res
    return out


def end_to_end(N, B, L, T, F, R):
    from pyglm_amd.models import NonlinearAutoregressiveModel
    from pyglm_amd.regression import SparseBernoulliRegression
    np.random.seed(0)
    rng = np.random.default_rng(0)
    regs = [SparseBernoulliRegression(N, B, rho=0.5, mu_b=-2.0, S_b=0.1) for _ in range(N)]
    model = NonlinearAutoregressiveModel(N, regs, basis=cosine_basis(B, L=L) / L)
    A, W, b = model._adopt_state()
    A[...] = rng.random((N, N)) < 0.5
    W[...] = rng.standard_normal(W.shape) / np.sqrt(N)
    b[:, 0] = -2.0 + 0.3 * rng.standard_normal(N)
    model.add_data(model.simulate(T, seed=1, gpu=True).Y[0])
    free = np.sort(rng.choice(N, F, replace=False))

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    cp = model.conditional_check(free, replicates=R, seed=2, gpu=True)
    out = dict(F=F, R=R, T=T)
    out["collect_s"] = [wall(cp.collect) for _ in range(3)]
    out["inputs_s"] = [wall(lambda: model._conditional_inputs(free, 0, 0, T)) for _ in range(2)]      # base: the activation GEMM and its read-back
    out["conditional_simulate_no_paths_s"] = [wall(lambda: model.conditional_simulate(free, replicates=R, seed=k, keep_paths=False, gpu=True)) for k in range(2)]
    out["log_score_total"] = cp.log_score()["total"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--bins", type=int, default=2000, help="bins per timed launch of the conditional kernel")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--F", type=int, nargs="*", default=[1, 16, 64, 256])
    ap.add_argument("--R", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--no-model", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = dict(N=args.N, B=args.B, L=args.L, T=args.T, reps=args.reps, device=torch.cuda.get_device_name(0), boxes=1, source_hash=_lib.source_hash(),
               unit="kernels: HIP events around one launch, microseconds per bin (all R replicates); model: wall seconds of the call")
    out["kernels"] = kernels(args.N, args.B, args.L, args.bins, args.reps, args.F, args.R)
    torch.cuda.empty_cache()
    if not args.no_model:
        out["model"] = end_to_end(args.N, args.B, args.L, args.T, 16, 8)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
