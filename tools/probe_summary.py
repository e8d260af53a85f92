"""Time of the posterior accumulator's fold (pgl_summary_fold) at one shape, rates only and rates + pointwise, per observation mode --
Bernoulli (obs 0), binomial n = 10 (obs 3) and the Bernoulli terms through the hooks mode (obs 4) -- as GB/s against the bytes the kernel has
to move; and end to end on a model of the same shape: collect() against the only way to the same sample without the accumulator
(model.means[0] + model.log_likelihood()) and against log_likelihood() alone (the floor: same upload, same activation, one pass without
accumulators).  HIP events around the kernel calls, wall time around the model calls; one warm-up, mean of --reps.

    python tools/probe_summary.py [--N 1024] [--T 100000] [--B 5] [--reps 5]
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
from pyglm_amd import _lib  # noqa: E402
from pyglm_amd._lib import call, ptr  # noqa: E402

COPY_TBS = 6.3      # what a device-to-device copy reaches on MI355X (TB/s): the yardstick for a streaming kernel


def kernels(N, T, reps):
    ldn = N + (N & 1)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    Psi = torch.randn(T, ldn, dtype=torch.float64, device=dev, generator=g) - 2.0
    u = torch.rand(T, ldn, dtype=torch.float64, device=dev, generator=g)
    Ybern = (u < 0.1).to(torch.float64)
    Ybin = torch.floor(u * 3.0)
    del u
    hooks = torch.zeros(T, 3, ldn, dtype=torch.float64, device=dev)
    hooks[:, 0] = Ybern
    hooks[:, 1] = 1.0
    part = torch.zeros(_lib.load().pgl_pg_loglik_partials(T), N, dtype=torch.float64, device=dev)
    ll = torch.zeros(N, dtype=torch.float64, device=dev)
    acc = [torch.zeros(T, ldn, dtype=torch.float64, device=dev) for _ in range(6)]
    link = torch.zeros(N, dtype=torch.int32, device=dev)
    par = torch.ones(N, dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def fold(obs, Y, xi, hk, pointwise, k):
        pw = [ptr(a) for a in acc[2:]] if pointwise else [None] * 4
        call("pgl_summary_fold", ptr(Psi), ldn, None, ptr(Y), ptr(part), ptr(ll), 0, T, N, obs, xi, None, ptr(hk), ldn, None, ptr(acc[0]), ptr(acc[1]),
             ptr(link) if obs == 4 else None, 3 if obs == 3 else 0, ptr(par) if obs == 4 else None, xi, *pw, k, st)

    def plain(obs, Y, xi, hk):       # the log-likelihood pass without accumulators
        call("pgl_pg_loglik_ex", ptr(Psi), ldn, None, ptr(Y), ldn, None, 0, None, 0, ptr(part), ptr(ll), 0, T, N, obs, xi, None, ptr(hk), ldn, 1, 0, 0, 0, st)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    res = {}
    for name, (obs, Y, xi, hk) in {"bernoulli_obs0": (0, Ybern, 1.0, None), "binomial_n10_obs3": (3, Ybin, 10.0, None),
                                   "bernoulli_hooks_obs4": (4, Ybern, 1.0, hooks)}.items():
        plain(obs, Y, xi, hk)
        ms = [timed(lambda: plain(obs, Y, xi, hk)) for _ in range(reps)]
        ll_plain = ll.clone()
        # (pg_loglik writes psi back; the fold does not)
        res[name] = dict(loglik_only=dict(ms_mean=float(np.mean(ms)), ms_min=float(np.min(ms)), bytes_per_cell=24 + (24 if obs == 4 else 0)))
        for mode, pointwise in (("rates", False), ("rates_pointwise", True)):
            for a in acc:
                a.zero_()
            fold(obs, Y, xi, hk, pointwise, 1)
            ms = [timed(lambda: fold(obs, Y, xi, hk, pointwise, 2 + r)) for r in range(reps)]
            bpc = 16 + (24 if obs == 4 else 0) + 32 + (64 if pointwise else 0)
            gbs = bpc * T * N / (float(np.mean(ms)) * 1e-3) / 1e9
            res[name][mode] = dict(ms_mean=float(np.mean(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)), bytes_per_cell=bpc,
                                   GBps=gbs, fraction_of_copy=gbs / (COPY_TBS * 1e3))
        res[name]["ll_bit_equal_to_loglik"] = bool(torch.equal(ll, ll_plain))
    return res


def end_to_end(N, B, T, reps):
    from pyglm_amd.models import SparseBernoulliGLM
    from pyglm_amd.utils.basis import cosine_basis
    np.random.seed(0)
    rng = np.random.default_rng(0)
    model = SparseBernoulliGLM(N, basis=cosine_basis(B, L=100) / 100, seed=1, engine_kwargs=dict(likelihood_only=True),
                               regression_kwargs=dict(rho=0.1, S_w=0.01, mu_b=-2.0))
    model.add_data((rng.random((T, N)) < 0.08).astype(np.float64))
    acc = {mode: model.summarize(rates=True, pointwise=pw) for mode, pw in (("rates", False), ("rates_pointwise", True))}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = {}
    for name, fn in [("log_likelihood", model.log_likelihood), ("means0_plus_log_likelihood", lambda: (model.means[0], model.log_likelihood())),
                     ("collect_rates", acc["rates"].collect), ("collect_rates_pointwise", acc["rates_pointwise"].collect)]:
        fn()
        ms = [wall(fn) for _ in range(reps)]
        out[name] = dict(ms_mean=float(np.mean(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)))
    base, floor = out["means0_plus_log_likelihood"]["ms_mean"], out["log_likelihood"]["ms_mean"]
    for k in ("collect_rates", "collect_rates_pointwise"):
        out[k]["speedup_vs_means_plus_ll"] = base / out[k]["ms_mean"]
        out[k]["ratio_to_log_likelihood"] = out[k]["ms_mean"] / floor
    assert acc["rates"].log_likelihoods[-1] == model.log_likelihood()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-model", action="store_true", help="kernels only")
    args = ap.parse_args()
    out = dict(N=args.N, B=args.B, T=args.T, reps=args.reps, device=torch.cuda.get_device_name(0), boxes=1, source_hash=_lib.source_hash(),
               unit="ms; kernels: HIP events around one pgl_summary_fold / pgl_pg_loglik_ex call; model: wall time of the call", copy_TBps=COPY_TBS)
    out["kernels"] = kernels(args.N, args.T, args.reps)
    torch.cuda.empty_cache()
    if not args.no_model:
        out["model"] = end_to_end(args.N, args.B, args.T, max(2, args.reps // 2))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
