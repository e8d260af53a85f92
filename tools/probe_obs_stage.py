"""Time of the pg_loglik stage (PG draw + kappa + log-likelihood, pgl_pg_loglik / pgl_pg_loglik_ex with omega and kappa written) per
observation model at one shape: Bernoulli fused (obs 0), the same Bernoulli terms through the hooks mode (obs 4: a | b | log c read
from HBM) and binomial n = 10 (obs 3).  HIP events around the call, mean of --reps after one warm-up.

    python tools/probe_obs_stage.py [--N 1024] [--T 100000] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyglm_amd import _lib  # noqa: E402
from pyglm_amd._lib import call, ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    N, T = args.N, args.T
    ldn = N + (N & 1)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    Psi = torch.randn(T, ldn, dtype=torch.float64, device=dev, generator=g) - 2.0
    OK = torch.zeros(T, 2 * ldn, dtype=torch.float64, device=dev)
    part = torch.zeros(_lib.load().pgl_pg_loglik_partials(T), N, dtype=torch.float64, device=dev)
    ll = torch.zeros(N, dtype=torch.float64, device=dev)
    u = torch.rand(T, ldn, dtype=torch.float64, device=dev, generator=g)
    Ybern = (u < 0.1).to(torch.float64)
    Ybin = torch.floor(u * 3.0)                       # counts 0..2 of n = 10 trials
    hooks = torch.zeros(T, 3, ldn, dtype=torch.float64, device=dev)
    hooks[:, 0] = Ybern
    hooks[:, 1] = 1.0
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    kp = ctypes.c_void_p(OK.data_ptr() + 8 * ldn)

    def run(obs, Y, xi, hk):
        if obs == 0:
            call("pgl_pg_loglik", ptr(Psi), ldn, None, ptr(Y), ldn, ptr(OK), 2 * ldn, kp, 2 * ldn, ptr(part), ptr(ll), 0, T, N, 0, 1.0, 1, 0, 0, 0, st)
        else:
            call("pgl_pg_loglik_ex", ptr(Psi), ldn, None, ptr(Y), ldn, ptr(OK), 2 * ldn, kp, 2 * ldn, ptr(part), ptr(ll), 0, T, N, obs, xi, None,
                 ptr(hk), ldn, 1, 0, 0, 0, st)

    out = dict(N=N, T=T, reps=args.reps, unit="ms per call (one sweep's pg_loglik stage)")
    res = {}
    for name, (obs, Y, xi, hk) in {"bernoulli_obs0": (0, Ybern, 1.0, None), "bernoulli_hooks_obs4": (4, Ybern, 1.0, hooks),
                                   "binomial_n10_obs3": (3, Ybin, 10.0, None)}.items():
        run(obs, Y, xi, hk)
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(obs, Y, xi, hk)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        res[name] = dict(ms_mean=float(np.mean(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)), ll_sum=float(ll.sum().item()))
        if name == "bernoulli_obs0":
            om0 = OK.clone()
        elif name == "bernoulli_hooks_obs4":
            res[name]["bit_equal_to_obs0"] = bool(torch.equal(om0, OK))
    out["stages"] = res
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
