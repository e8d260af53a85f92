"""Time of the latent fold (pgl_latent_fold) at Q = 1 and Q = 8 beside the covariate fold (pgl_covariate_fold) at K = 8 on the same buffers in
the same run -- the latent fold reads 24 B per cell (Psi, Omega, Kappa), the covariate fold 32 (the offset too); both do about 44 multiply-
adds per cell at 8 columns; what the latent fold has and the column fold lacks is the cross-lane tree --, the draw (pgl_latent_draw) alone,
and end to end at the BASELINE configs[1] and configs[3] shapes: resample_model() with one latent beside the same model without, and the
latent step alone with its stages.  HIP events around the kernel calls, wall time around the model calls; one warm-up, mean of --reps.
The gate of DESIGN.md section 20: the latent fold at Q = 8 takes at most 1.5 x the covariate fold's time at K = 8 in this run.

    python tools/probe_latents.py [--N 1024] [--T 100000] [--reps 5] [--no-model] [--out profiles/latent_probe.json]
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
GATE = 1.5


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


def kernels(N, T, reps):
    lib = _lib.load()
    ldn = N + (N & 1)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, device=dev, generator=g)
    Psi = rnd(T, ldn) * 0.5 - 2.0
    OK = torch.empty(T, 2 * ldn, dtype=torch.float64, device=dev)
    OK[:, :ldn] = torch.rand(T, ldn, dtype=torch.float64, device=dev, generator=g) * 0.2 + 0.05
    OK[:, ldn:] = (torch.rand(T, ldn, dtype=torch.float64, device=dev, generator=g) < 0.12).double() - 0.5
    Off = rnd(T, ldn) * 0.3
    bias = torch.zeros(N, dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    kappa = ctypes.c_void_p(OK.data_ptr() + 8 * ldn)
    cells = float(T) * N
    res = dict(lds_columns=_lib.PGL_LATENT_LDS_COLS, loadings_in_lds=bool(N <= _lib.PGL_LATENT_LDS_COLS))

    def rate(entry, bytes_per_cell):
        gbs = bytes_per_cell * cells / (entry["ms_mean"] * 1e-3) / 1e9
        entry.update(bytes_per_cell=bytes_per_cell, GBps=gbs, fraction_of_copy=gbs / (COPY_TBS * 1e3))
        return entry

    K = 8
    S = rnd(T, K)
    Lam, r = torch.zeros(N, K * (K + 1) // 2, dtype=torch.float64, device=dev), torch.zeros(N, K, dtype=torch.float64, device=dev)
    work = torch.empty(lib.pgl_covariate_work_bytes(N, T, K), dtype=torch.uint8, device=dev)
    cfold = lambda: call("pgl_covariate_fold", Psi=ptr(Psi), ldn=ldn, bias=ptr(bias), Omega=ptr(OK), ldo=2 * ldn, Kappa=kappa, ldk=2 * ldn, Off=ptr(Off),
                         S=ptr(S), lds=K, T=T, nloc=N, K=K, Lambda=ptr(Lam), r=ptr(r), accumulate=0, work=ptr(work), hip_stream=st)
    cfold()
    res["pgl_covariate_fold_K8"] = rate(ms_stats([timed(cfold) for _ in range(reps)]), 32)
    res["pgl_covariate_fold_K8"]["multiply_adds_per_cell"] = 44
    del work, Lam, r
    torch.cuda.empty_cache()
    Bt = torch.zeros(K, ldn, dtype=torch.float64, device=dev)
    Bt[:, :N] = rnd(K, N) * 0.5
    for Q in (1, 8):
        P = Q * (Q + 1) // 2
        LamT, rT = torch.zeros(T, P, dtype=torch.float64, device=dev), torch.zeros(T, Q, dtype=torch.float64, device=dev)
        lfold = lambda: call("pgl_latent_fold", Psi=ptr(Psi), ldn=ldn, bias=ptr(bias), Omega=ptr(OK), ldo=2 * ldn, Kappa=kappa, ldk=2 * ldn, S=ptr(S),
                             lds=K, col0=K - Q, Beta=ptr(Bt), ldb=ldn, T=T, nloc=N, Q=Q, Lambda=ptr(LamT), r=ptr(rT), hip_stream=st)
        lfold()
        e = rate(ms_stats([timed(lfold) for _ in range(reps)]), 24)
        e.update(multiply_adds_per_cell=P + 3 * Q + 2, sums_per_bin=P + Q, values_across_lanes_per_bin=63 if Q == 8 else 6,
                 over_covariate_fold_K8=e["ms_mean"] / res["pgl_covariate_fold_K8"]["ms_mean"])
        res["pgl_latent_fold_Q%d" % Q] = e
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        Sd = S.clone()
        draw = lambda k: call("pgl_latent_draw", Lambda=ptr(LamT), r=ptr(rT), z_override=None, seed=1, sweep=k, elem0=0, S=ptr(Sd), lds=K, col0=K - Q,
                              status=ptr(status), T=T, Q=Q, hip_stream=st)
        draw(0)
        res["pgl_latent_draw_Q%d" % Q] = ms_stats([timed(lambda: draw(1 + i)) for i in range(reps)])
        assert not int(status.item())
        del LamT, rT, Sd
    res["gate"] = dict(limit=GATE, latent_fold_Q8_over_covariate_fold_K8=res["pgl_latent_fold_Q8"]["over_covariate_fold_K8"],
                       met=bool(res["pgl_latent_fold_Q8"]["over_covariate_fold_K8"] <= GATE))
    return res


def end_to_end(name, cls, N, B, T, reps, Q=1, **reg_kw):
    from pyglm_amd import models
    from pyglm_amd.utils.basis import cosine_basis
    rng = np.random.default_rng(1)
    Y = (rng.negative_binomial(2, 0.85, size=(T, N)) if "Negative" in cls else (rng.random((T, N)) < 0.1)).astype(np.float64)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = dict(config=name, model=cls, N=N, B=B, T=T, Q=Q)
    for label, q in (("without_latents", 0), ("with_latents", Q)):
        np.random.seed(0)
        kw = dict(regression_kwargs=reg_kw) if reg_kw else {}
        model = getattr(models, cls)(N, basis=cosine_basis(B, L=100) / 100, seed=0, **(dict(n_latents=q) if q else {}), **kw)
        model.add_data(Y)
        model.resample_model()
        out["resample_model_" + label] = ms_stats([wall(model.resample_model) for _ in range(reps)])
        if q:
            eng = model.engine
            a, W, b = model._local_state()
            step = lambda: model._lat_step.latent_step(a, W, b, model.seed, model.sweeps_done)
            step()
            out["latent_step"] = ms_stats([wall(step) for _ in range(reps)])
            eng.profile = True
            step()
            out["latent_step_stages_ms"] = {n: v["ms"] / v["calls"] for n, v in eng.collect_timings().items()}
            eng.profile = False
        del model
        torch.cuda.empty_cache()
    out["latent_step_share_of_resample_model"] = out["latent_step"]["ms_mean"] / out["resample_model_with_latents"]["ms_mean"]
    out["with_over_without"] = out["resample_model_with_latents"]["ms_mean"] / out["resample_model_without_latents"]["ms_mean"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-model", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = dict(N=args.N, T=args.T, reps=args.reps, device=torch.cuda.get_device_name(0), boxes=1, source_hash=_lib.source_hash(),
               unit="ms; kernels: HIP events around one call (a fold = all its launches); model: wall time of the call", copy_TBps=COPY_TBS)
    out["kernels"] = kernels(args.N, args.T, args.reps)
    torch.cuda.empty_cache()
    if not args.no_model:
        r = max(2, args.reps // 2)
        out["models"] = [end_to_end("configs[1]", "SparseBernoulliGLM", 128, 5, 50000, r),
                         end_to_end("configs[3] shape", "NegativeBinomialGLM", 512, 5, 100000, r, S_w=1.0, mu_b=-2.0, xi=2.0)]
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
