"""Time of free-running simulation under covariates and latent factors at one shape, every figure beside its yardstick in the same run:
  kernels   pgl_simulate_offset with `Off` given (per replicate) and with Off = NULL beside pgl_simulate, microseconds per bin, R = 1 and 8;
  chunk     the two launches a chunk adds -- pgl_latent_prior_paths + pgl_simulate_offset_build at K_obs = 2, Q = 8 -- beside that chunk's
            pgl_simulate_offset launch (the chunk model.simulate() would cut: simulate.chunk_bins), and their share of it (the line for a
            per-chunk add-on is 5 %);
  model     model.simulate(T, replicates=8, keep_paths=False) with and without covariates= + latents="prior", wall seconds.
HIP events around the calls, one warm-up, mean of --reps.

    python tools/probe_simulate_offset.py [--N 1024] [--B 5] [--L 100] [--T 100000] [--bins 0] [--reps 5] [--out profiles/simulate_offset_probe.json]
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

K_OBS, Q = 2, 8


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def mean_ms(fn, reps):
    fn()
    ms = [timed(fn) for _ in range(reps)]
    return float(np.mean(ms)), float(np.min(ms)), float(np.max(ms))


def kernels(N, B, L, bins, reps, Rs):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    f64 = dict(dtype=torch.float64, device=dev)
    Wm = torch.from_numpy(rng.standard_normal((N, N * B)) / np.sqrt(N) * (rng.random((N, N * B)) < 0.5)).to(dev)
    bias = torch.from_numpy(-2.0 + 0.3 * rng.standard_normal(N)).to(dev)
    basis = torch.from_numpy(np.ascontiguousarray(cosine_basis(B, L=L) / L)).to(dev)
    beta = torch.from_numpy(rng.standard_normal((K_OBS + Q, N)) * 0.2).to(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    kind, par = torch.zeros(N, dtype=torch.int32, device=dev), torch.zeros(N, **f64)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    phi = np.full(Q, 0.9)
    phi_c, s_c = (ctypes.c_double * Q)(*phi), (ctypes.c_double * Q)(*np.sqrt(1 - phi * phi))
    out = {}
    for R in Rs:
        nb = simulate.chunk_bins(N, B, R) if bins <= 0 else min(bins, simulate.chunk_bins(N, B, R))
        ring = torch.zeros(R, L, N, **f64)
        s, ss = torch.zeros(R, N, **f64), torch.zeros(R, N, **f64)
        work = torch.zeros(lib.pgl_simulate_work_bytes(N, B, R), dtype=torch.uint8, device=dev)
        S = torch.from_numpy(rng.standard_normal((nb, K_OBS))).to(dev)
        X, carry = torch.empty(R, nb, Q, **f64), torch.zeros(R, Q, **f64)
        Off = torch.empty(R, nb, N, **f64)
        t = [0]
        common = dict(Wm=ptr(Wm), bias=ptr(bias), basis=ptr(basis), N=N, B=B, L=L, kind=ptr(kind), par=ptr(par), R=R, rep0=0, seed=1, ring=ptr(ring),
                      Y=None, ldr=0, sum=ptr(s), sumsq=ptr(ss), Tc=nb, work=ptr(work), status=ptr(status), hip_stream=st)

        def paths():
            call("pgl_latent_prior_paths", X=ptr(X), ldx_r=nb * Q, R=R, rep0=0, t0=t[0], Tc=nb, Q=Q, phi=ctypes.cast(phi_c, ctypes.c_void_p),
                 s=ctypes.cast(s_c, ctypes.c_void_p), carry=ptr(carry), has_carry=1, z_override=None, seed=1, hip_stream=st)

        def build():
            call("pgl_simulate_offset_build", S=ptr(S), lds=K_OBS, X=ptr(X), ldx_r=nb * Q if R > 1 else 0, Beta=ptr(beta), ldn=N, Off=ptr(Off), ldo_t=N,
                 ldo_r=nb * N, Tc=nb, N=N, K_obs=K_OBS, Q=Q, R=R, hip_stream=st)

        def plain():
            call("pgl_simulate", t0=t[0], **common)
            t[0] += nb

        def null():
            call("pgl_simulate_offset", t0=t[0], Off=None, ldo_t=0, ldo_r=0, **common)
            t[0] += nb

        def offset():
            call("pgl_simulate_offset", t0=t[0], Off=ptr(Off), ldo_t=N, ldo_r=nb * N, **common)
            t[0] += nb

        paths()
        build()
        res = dict(bins_per_launch=nb)
        for name, fn in (("pgl_simulate", plain), ("pgl_simulate_offset_null", null), ("pgl_simulate_offset", offset), ("pgl_simulate_again", plain)):
            m, lo, hi = mean_ms(fn, reps)
            res[name] = dict(us_per_bin_mean=m * 1e3 / nb, us_per_bin_min=lo * 1e3 / nb, us_per_bin_max=hi * 1e3 / nb)
        assert int(status[0]) == 0, status.tolist()
        res["mean_rate"] = float(s.sum() / (R * N * t[0]))
        res["offset_over_plain"] = res["pgl_simulate_offset"]["us_per_bin_mean"] / res["pgl_simulate"]["us_per_bin_mean"]
        res["null_over_plain"] = res["pgl_simulate_offset_null"]["us_per_bin_mean"] / res["pgl_simulate"]["us_per_bin_mean"]
        pm, bm = mean_ms(paths, reps)[0], mean_ms(build, reps)[0]
        launch_ms = res["pgl_simulate_offset"]["us_per_bin_mean"] * nb / 1e3
        res["chunk"] = dict(K_obs=K_OBS, Q=Q, paths_ms=pm, build_ms=bm, simulate_launch_ms=launch_ms, added_share=(pm + bm) / launch_ms,
                            off_bytes=8 * R * nb * N)
        out["R%d" % R] = res
    return out


def end_to_end(N, B, L, T, R):
    from pyglm_amd.models import NonlinearAutoregressiveModel
    from pyglm_amd.regression import SparseBernoulliRegression
    np.random.seed(0)
    rng = np.random.default_rng(0)
    regs = [SparseBernoulliRegression(N, B, rho=0.5, mu_b=-2.0, S_b=0.1) for _ in range(N)]
    model = NonlinearAutoregressiveModel(N, regs, basis=cosine_basis(B, L=L) / L)
    A, W, b = model._adopt_state()
    A[...] = True
    W[...] = rng.standard_normal(W.shape) / np.sqrt(N)
    b[:, 0] = -2.0 + 0.3 * rng.standard_normal(N)
    kind, par = simulate.observation_kinds(regs)
    Wm = (W * A[:, :, None]).reshape(N, N * B)
    drive = simulate.Drive(rng.standard_normal((N, K_OBS + Q)) * 0.2, S_obs=rng.standard_normal((T, K_OBS)), latents="prior", phi=np.full(Q, 0.9))

    def run(seed, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sim = simulate.simulate(Wm, b.ravel(), np.asarray(model.basis, dtype=np.float64), kind, par, T, replicates=R, seed=seed, keep_paths=False,
                                on_device=True, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, float(sim.sum.sum() / (R * N * T))

    run(0)                                                           # warm-up of both paths
    run(0, drive=drive)
    plain = [run(k) for k in range(2)]
    driven = [run(k, drive=drive) for k in range(2)]
    return dict(T=T, replicates=R, K_obs=K_OBS, Q=Q, simulate_s=[p[0] for p in plain], simulate_driven_s=[d[0] for d in driven],
                mean_rate=plain[0][1], mean_rate_driven=driven[0][1], driven_over_plain=float(np.mean([d[0] for d in driven]) / np.mean([p[0] for p in plain])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--bins", type=int, default=0, help="bins per timed launch at most; 0: the chunk simulate() cuts (simulate.chunk_bins)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--R", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--no-model", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = dict(N=args.N, B=args.B, L=args.L, reps=args.reps, device=torch.cuda.get_device_name(0), boxes=1, source_hash=_lib.source_hash(),
               unit="kernels: HIP events around one launch, mean of reps after a warm-up; model: wall seconds of the call")
    out["kernels"] = kernels(args.N, args.B, args.L, args.bins, args.reps, args.R)
    torch.cuda.empty_cache()
    if not args.no_model:
        out["model"] = end_to_end(args.N, args.B, args.L, args.T, 8)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
