"""Time of the covariate fold (pgl_covariate_fold) at K = 1, 8, 32 beside the dispersion fold and the time-rescaling fold on the same buffers
in the same run -- it reads 32 B per cell at K <= 8 (Omega, Kappa, the offset, Psi), they 16 B --, the draw and the offset rebuild, and end to
end at the BASELINE configs[1] and configs[3] shapes: resample_model() with covariates beside the same model without, and the covariate
step alone (activation, fold, draw, offset rebuild) with its stages.  HIP events around the kernel calls, wall time around the model calls;
one warm-up, mean of --reps.

    python tools/probe_covariates.py [--N 1024] [--T 100000] [--reps 5] [--no-model] [--out profiles/covariates_probe.json]
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
KS = (1, 8, 32)


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


def kernels(N, T, reps, D=64):
    lib = _lib.load()
    ldn = N + (N & 1)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, device=dev, generator=g)
    Psi = rnd(T, ldn) * 0.5 - 2.0
    Y = (torch.rand(T, ldn, dtype=torch.float64, device=dev, generator=g) < 0.12).double()
    OK = torch.empty(T, 2 * ldn, dtype=torch.float64, device=dev)
    OK[:, :ldn] = torch.rand(T, ldn, dtype=torch.float64, device=dev, generator=g) * 0.2 + 0.05
    OK[:, ldn:] = Y - 0.5
    Off = rnd(T, ldn) * 0.3
    bias = torch.zeros(N, dtype=torch.float64, device=dev)
    xid = torch.full((N,), 2.0, dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    hist = torch.zeros(N, D, dtype=torch.int32, device=dev)
    zsum = torch.zeros(N, 2, dtype=torch.float64, device=dev)
    Ld, Sd = torch.zeros(N, dtype=torch.int64, device=dev), torch.zeros(N, dtype=torch.float64, device=dev)
    work_r = torch.empty(lib.pgl_rescale_work_bytes(N, T), dtype=torch.uint8, device=dev)
    work_d = torch.empty(lib.pgl_dispersion_work_bytes(N, T), dtype=torch.uint8, device=dev)
    cells = float(T) * N
    res = dict(rows_per_workgroup=_lib.PGL_COVARIATE_ROWS)

    def rate(entry, bytes_per_cell):
        gbs = bytes_per_cell * cells / (entry["ms_mean"] * 1e-3) / 1e9
        entry.update(bytes_per_cell=bytes_per_cell, GBps=gbs, fraction_of_copy=gbs / (COPY_TBS * 1e3))
        return entry

    rescale = lambda k: call("pgl_rescale_fold", ptr(Psi), ldn, ptr(bias), ptr(Y), T, N, None, 1.0, D, 1, k - 1, 0, 0, ptr(hist), ptr(zsum), 0, ptr(work_r), st)
    disp = lambda k: call("pgl_dispersion_fold", Psi=ptr(Psi), ldn=ldn, bias=ptr(bias), Y=ptr(Y), T=T, nloc=N, xi=ptr(xid), seed=1, sweep=k, neuron0=0,
                          elem0=0, L=ptr(Ld), S=ptr(Sd), accumulate=0, work=ptr(work_d), hip_stream=st)
    rescale(1)
    res["pgl_rescale_fold"] = rate(ms_stats([timed(lambda: rescale(2 + r)) for r in range(reps)]), 16)
    disp(1)
    res["pgl_dispersion_fold"] = rate(ms_stats([timed(lambda: disp(2 + r)) for r in range(reps)]), 16)
    del work_r, work_d
    for K in KS:
        P = K * (K + 1) // 2
        S = rnd(T, K)
        Lam, r = torch.zeros(N, P, dtype=torch.float64, device=dev), torch.zeros(N, K, dtype=torch.float64, device=dev)
        work = torch.empty(lib.pgl_covariate_work_bytes(N, T, K), dtype=torch.uint8, device=dev)
        fold = lambda: call("pgl_covariate_fold", Psi=ptr(Psi), ldn=ldn, bias=ptr(bias), Omega=ptr(OK), ldo=2 * ldn,
                            Kappa=ctypes.c_void_p(OK.data_ptr() + 8 * ldn), ldk=2 * ldn, Off=ptr(Off), S=ptr(S), lds=K, T=T, nloc=N, K=K, Lambda=ptr(Lam),
                            r=ptr(r), accumulate=0, work=ptr(work), hip_stream=st)
        fold()
        KB = -(-K // 8)
        e = rate(ms_stats([timed(fold) for _ in range(reps)]), 32 * KB + 8 * KB * (KB - 1) // 2)
        # executed: 44 per diagonal block (36 of Lambda, k <= j, and 8 of r) and 64 per block below it, whatever K -- the sums past K run
        # over zero padding; useful: the K (K + 1) / 2 + K sums the law asks for.  The two agree where K is a multiple of 8
        e.update(work_bytes=int(work.numel()), multiply_adds_per_cell=44 * KB + 64 * KB * (KB - 1) // 2, useful_multiply_adds_per_cell=P + K,
                 over_dispersion_fold=e["ms_mean"] / res["pgl_dispersion_fold"]["ms_mean"],
                 rate_over_dispersion_fold=e["GBps"] / res["pgl_dispersion_fold"]["GBps"])
        e["Gfma_per_s"] = e["multiply_adds_per_cell"] * cells / (e["ms_mean"] * 1e-3) / 1e9
        e["useful_Gfma_per_s"] = e["useful_multiply_adds_per_cell"] * cells / (e["ms_mean"] * 1e-3) / 1e9
        res["pgl_covariate_fold_K%d" % K] = e
        # the draw and the offset rebuild at the same K
        L0, h0 = torch.eye(K, dtype=torch.float64, device=dev), torch.zeros(K, dtype=torch.float64, device=dev)
        z, beta, status = rnd(N, K), torch.zeros(N, K, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
        draw = lambda: call("pgl_covariate_draw", Lambda=ptr(Lam), r=ptr(r), Lambda0=ptr(L0), h0=ptr(h0), z=ptr(z), Beta_out=ptr(beta), status=ptr(status),
                            nloc=N, K=K, hip_stream=st)
        draw()
        res["pgl_covariate_draw_K%d" % K] = ms_stats([timed(draw) for _ in range(reps)])
        assert not bool(status.any())
        Bt = torch.zeros(K, ldn, dtype=torch.float64, device=dev)
        Bt[:, :N] = beta.t()
        offs = lambda: call("pgl_covariate_offset", S=ptr(S), lds=K, Beta=ptr(Bt), Off=ptr(Off), ldn=ldn, T=T, nloc=N, K=K, hip_stream=st)
        offs()
        res["pgl_covariate_offset_K%d" % K] = rate(ms_stats([timed(offs) for _ in range(reps)]), 8)
        Off.normal_(generator=g).mul_(0.3)
        del work, S
        torch.cuda.empty_cache()
    return res


def end_to_end(name, cls, N, B, T, reps, K=2, **reg_kw):
    from pyglm_amd import models
    from pyglm_amd.utils.basis import cosine_basis
    rng = np.random.default_rng(1)
    Y = (rng.negative_binomial(2, 0.85, size=(T, N)) if "Negative" in cls else (rng.random((T, N)) < 0.1)).astype(np.float64)
    t = np.arange(T)
    S = np.column_stack([np.sin(2 * np.pi * t / 500.0), (t % 2000 >= 1000).astype(float)] + [rng.standard_normal(T) for _ in range(K - 2)])[:, :K]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = dict(config=name, model=cls, N=N, B=B, T=T, K=K)
    for label, k in (("without_covariates", 0), ("with_covariates", K)):
        np.random.seed(0)
        kw = dict(regression_kwargs=reg_kw) if reg_kw else {}
        model = getattr(models, cls)(N, basis=cosine_basis(B, L=100) / 100, seed=0, n_covariates=k, **kw)
        model.add_data(Y, **(dict(covariates=S) if k else {}))
        model.resample_model()
        out["resample_model_" + label] = ms_stats([wall(model.resample_model) for _ in range(reps)])
        if k:
            eng = model.engine
            a, W, b = model._local_state()
            step = lambda: model._cov_step.covariate_step(a, W, b, model.seed, model.sweeps_done)
            step()
            out["covariate_step"] = ms_stats([wall(step) for _ in range(reps)])
            eng.profile = True
            step()
            out["covariate_step_stages_ms"] = {n: v["ms"] / v["calls"] for n, v in eng.collect_timings().items()}
            eng.profile = False
            out["beta_range"] = [float(model.covariate_weights.min()), float(model.covariate_weights.max())]
        del model
        torch.cuda.empty_cache()
    out["covariate_step_share_of_resample_model"] = out["covariate_step"]["ms_mean"] / out["resample_model_with_covariates"]["ms_mean"]
    out["with_over_without"] = out["resample_model_with_covariates"]["ms_mean"] / out["resample_model_without_covariates"]["ms_mean"]
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
