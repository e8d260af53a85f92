"""Time of the latents' joint draw under the temporal prior (pgl_latent_ar_draw) at Q = 1 and Q = 8 beside, in the same run on the same
buffers: the same entry as ONE serial chain (seg = T), the latent fold that feeds it (pgl_latent_fold) and the independent bins' draw
(pgl_latent_draw); the draw over a few segment lengths, which is what the default (pgl_latent_ar_seg) rests on; and end to end at the
BASELINE configs[1] and configs[3] shapes, resample_model() with one latent under latent_ar = .9 beside latent_ar = None in the same run.
HIP events around the kernel calls (a draw = all its 2 levels + 1 launches), wall time around the model calls; one warm-up, mean of --reps
(the serial chain: of 2; every entry records its own count).
The gate of DESIGN.md section 21: at each Q the draw at the default seg takes at most 2 x the fold's time, and less than the serial chain's.

    python tools/probe_latent_ar.py [--N 1024] [--T 100000] [--reps 5] [--segs 8,10,12,16,24,32,64,128] [--no-model] [--out profiles/latent_ar_probe.json]
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

GATE = 2.0
PHI = 0.9


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


def levels(T, seg):
    n, k = T, 0
    while n >= 2 * seg:
        n, k = n // seg, k + 1
    return k


def kernels(N, T, reps, segs):
    lib = _lib.load()
    ldn = N + (N & 1)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, device=dev, generator=g)
    Psi = rnd(T, ldn) * 0.5 - 2.0
    OK = torch.empty(T, 2 * ldn, dtype=torch.float64, device=dev)
    OK[:, :ldn] = torch.rand(T, ldn, dtype=torch.float64, device=dev, generator=g) * 0.2 + 0.05
    OK[:, ldn:] = (torch.rand(T, ldn, dtype=torch.float64, device=dev, generator=g) < 0.12).double() - 0.5
    bias = torch.zeros(N, dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    kappa = ctypes.c_void_p(OK.data_ptr() + 8 * ldn)
    K = 8
    S = rnd(T, K)
    Bt = torch.zeros(K, ldn, dtype=torch.float64, device=dev)
    Bt[:, :N] = rnd(K, N) * 0.5
    seg0 = int(lib.pgl_latent_ar_seg())
    res = dict(default_seg=seg0, phi=PHI)
    for Q in (1, 8):
        P = Q * (Q + 1) // 2
        LamT, rT = torch.zeros(T, P, dtype=torch.float64, device=dev), torch.zeros(T, Q, dtype=torch.float64, device=dev)
        lfold = lambda: call("pgl_latent_fold", Psi=ptr(Psi), ldn=ldn, bias=ptr(bias), Omega=ptr(OK), ldo=2 * ldn, Kappa=kappa, ldk=2 * ldn, S=ptr(S),
                             lds=K, col0=K - Q, Beta=ptr(Bt), ldb=ldn, T=T, nloc=N, Q=Q, Lambda=ptr(LamT), r=ptr(rT), hip_stream=st)
        lfold()
        e = dict(Q=Q, pgl_latent_fold=dict(ms_stats([timed(lfold) for _ in range(reps)]), reps=reps))
        e["pgl_latent_fold"]["bytes_per_bin"] = 24 * N
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        Sd = S.clone()
        draw = lambda k: call("pgl_latent_draw", Lambda=ptr(LamT), r=ptr(rT), z_override=None, seed=1, sweep=k, elem0=0, S=ptr(Sd), lds=K, col0=K - Q,
                              status=ptr(status), T=T, Q=Q, hip_stream=st)
        draw(0)
        e["pgl_latent_draw"] = dict(ms_stats([timed(lambda: draw(1 + i)) for i in range(reps)]), reps=reps)
        phi = (ctypes.c_double * Q)(*([PHI] * Q))
        nbytes = max(int(lib.pgl_latent_ar_scratch(T, Q, s)) for s in set(segs) | {seg0, T})
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)

        def ar(k, seg):
            call("pgl_latent_ar_draw", Lambda=ptr(LamT), r=ptr(rT), phi=ctypes.cast(phi, ctypes.c_void_p), z_override=None, seed=1, sweep=k, elem0=0,
                 S=ptr(Sd), lds=K, col0=K - Q, status=ptr(status), T=T, Q=Q, seg=seg, scratch=ptr(scratch), scratch_bytes=nbytes, hip_stream=st)

        def ar_entry(seg, n):
            ar(0, seg)
            out = ms_stats([timed(lambda: ar(1 + i, seg)) for i in range(n)])
            out.update(reps=n, seg=seg, levels=levels(T, seg), launches=2 * levels(T, seg) + 1, scratch_bytes_per_bin=int(lib.pgl_latent_ar_scratch(T, Q, seg)) / T)
            return out

        e["pgl_latent_ar_draw"] = ar_entry(seg0, reps)
        e["pgl_latent_ar_draw_serial"] = ar_entry(T, min(reps, 2))
        e["pgl_latent_ar_draw_by_seg"] = [ar_entry(s, reps) for s in segs]
        assert not int(status.item())
        d, f, s1 = e["pgl_latent_ar_draw"]["ms_mean"], e["pgl_latent_fold"]["ms_mean"], e["pgl_latent_ar_draw_serial"]["ms_mean"]
        e["gate"] = dict(limit_over_fold=GATE, draw_over_fold=d / f, serial_over_draw=s1 / d, met=bool(d <= GATE * f and d < s1))
        res["Q%d" % Q] = e
        del LamT, rT, Sd, scratch
        torch.cuda.empty_cache()
    return res


def end_to_end(name, cls, N, B, T, reps, **reg_kw):
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

    out = dict(config=name, model=cls, N=N, B=B, T=T, Q=1, phi=PHI)
    for label, ar in (("phi_0", None), ("phi_%g" % PHI, PHI)):
        np.random.seed(0)
        kw = dict(regression_kwargs=reg_kw) if reg_kw else {}
        model = getattr(models, cls)(N, basis=cosine_basis(B, L=100) / 100, seed=0, n_latents=1, latent_ar=ar, **kw)
        model.add_data(Y)
        model.resample_model()
        out["resample_model_" + label] = ms_stats([wall(model.resample_model) for _ in range(reps)])
        eng = model.engine
        a, W, b = model._local_state()
        step = lambda: model._lat_step.latent_step(a, W, b, model.seed, model.sweeps_done)
        step()
        eng.profile = True
        step()
        out["latent_step_stages_ms_" + label] = {n: v["ms"] / v["calls"] for n, v in eng.collect_timings().items()}
        eng.profile = False
        del model
        torch.cuda.empty_cache()
    out["phi_over_zero"] = out["resample_model_phi_%g" % PHI]["ms_mean"] / out["resample_model_phi_0"]["ms_mean"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--segs", default="8,10,12,16,24,32,64,128")
    ap.add_argument("--no-model", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = dict(N=args.N, T=args.T, reps=args.reps, device=torch.cuda.get_device_name(0), boxes=1, source_hash=_lib.source_hash(),
               unit="ms; kernels: HIP events around one call (a draw = all its launches); model: wall time of the call")
    out["kernels"] = kernels(args.N, args.T, args.reps, [int(s) for s in args.segs.split(",")])
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
