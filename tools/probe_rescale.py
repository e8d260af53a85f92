"""Time of the time-rescaling fold (pgl_rescale_fold) beside the posterior accumulator's fold (pgl_summary_fold, rates only) on the same Psi and
Y in the same run -- the first reads 16 B per cell, the second moves 48 --, the same fold on 64 columns of the same length (the scan has a
sixteenth of the work there, the stitch walks as many records: what the stitch launch costs at least), pgl_rescale_ks, and end to end on a
model of the same shape: TimeRescaling.collect() beside PosteriorSummary.collect().  HIP events around the kernel calls, wall time around
the model calls; one warm-up, mean of --reps.

    python tools/probe_rescale.py [--N 1024] [--B 5] [--T 100000] [--D 64] [--reps 5] [--out profiles/rescale_probe.json]
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
from pyglm_amd import _lib, rescale  # noqa: E402
from pyglm_amd._lib import call, ptr  # noqa: E402

COPY_TBS = 6.3      # what a device-to-device copy reaches on MI355X (TB/s): the yardstick for a streaming kernel


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


def kernels(N, T, D, reps, rate=0.08):
    lib = _lib.load()
    ldn = N + (N & 1)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    Psi = torch.randn(T, ldn, dtype=torch.float64, device=dev, generator=g) - 2.5
    Y = (torch.rand(T, ldn, dtype=torch.float64, device=dev, generator=g) < rate).to(torch.float64)
    bias = torch.zeros(N, dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    part = torch.zeros(lib.pgl_pg_loglik_partials(T), N, dtype=torch.float64, device=dev)
    ll = torch.zeros(N, dtype=torch.float64, device=dev)
    acc = [torch.zeros(T, ldn, dtype=torch.float64, device=dev) for _ in range(2)]
    hist = torch.zeros(N, D, dtype=torch.int32, device=dev)
    hist_sum = torch.zeros(N, D, dtype=torch.int64, device=dev)
    zsum = torch.zeros(N, 2, dtype=torch.float64, device=dev)
    ks, mean, M2 = (torch.zeros(N, dtype=torch.float64, device=dev) for _ in range(3))
    exceed = torch.zeros(N, dtype=torch.int32, device=dev)
    work = torch.empty(lib.pgl_rescale_work_bytes(N, T), dtype=torch.uint8, device=dev)

    def summary(k):
        call("pgl_summary_fold", ptr(Psi), ldn, ptr(bias), ptr(Y), ptr(part), ptr(ll), 0, T, N, 0, 1.0, None, None, ldn, None, ptr(acc[0]), ptr(acc[1]),
             None, 0, None, 1.0, None, None, None, None, k, st)

    def fold(k, nloc=N):
        call("pgl_rescale_fold", ptr(Psi), ldn, ptr(bias), ptr(Y), T, nloc, None, 1.0, D, 1, k - 1, 0, 0, ptr(hist), ptr(zsum), 0, ptr(work), st)

    def ks_step(k):
        call("pgl_rescale_ks", ptr(hist), N, D, 1.36, ptr(ks), ptr(mean), ptr(M2), ptr(exceed), ptr(hist_sum), k, st)

    res = dict(segment_rows=lib.pgl_rescale_segment_rows(), work_bytes=int(work.numel()), event_rate=rate)
    summary(1)
    res["pgl_summary_fold_rates"] = dict(ms_stats([timed(lambda: summary(2 + r)) for r in range(reps)]), bytes_per_cell=48)
    fold(1, 64)
    res["pgl_rescale_fold_64_columns"] = ms_stats([timed(lambda: fold(2 + r, 64)) for r in range(reps)])
    fold(1)
    res["pgl_rescale_fold"] = dict(ms_stats([timed(lambda: fold(2 + r)) for r in range(reps)]), bytes_per_cell=16)
    for name in ("pgl_summary_fold_rates", "pgl_rescale_fold"):
        gbs = res[name]["bytes_per_cell"] * T * N / (res[name]["ms_mean"] * 1e-3) / 1e9
        res[name].update(GBps=gbs, fraction_of_copy=gbs / (COPY_TBS * 1e3))
    res["rescale_over_summary"] = res["pgl_rescale_fold"]["ms_mean"] / res["pgl_summary_fold_rates"]["ms_mean"]
    ks_step(1)
    res["pgl_rescale_ks"] = ms_stats([timed(lambda: ks_step(2 + r)) for r in range(reps)])
    # the last fold against the definition on a few columns
    cols = list(range(min(N, 4)))
    want = rescale.rescale_host(Psi[:, cols].cpu().numpy(), Y[:, cols].cpu().numpy(), 1.0, D, 1, reps, 0, 0)[0]
    got = hist.cpu().numpy()
    res["intervals_per_column_mean"] = float(got.sum(axis=1).mean())
    assert np.array_equal(got[cols], want)
    return res


def end_to_end(N, B, T, D, reps):
    from pyglm_amd.models import SparseBernoulliGLM
    from pyglm_amd.utils.basis import cosine_basis
    np.random.seed(0)
    rng = np.random.default_rng(0)
    model = SparseBernoulliGLM(N, basis=cosine_basis(B, L=100) / 100, seed=1, engine_kwargs=dict(likelihood_only=True),
                               regression_kwargs=dict(rho=0.1, S_w=0.01, mu_b=-2.0))
    model.add_data((rng.random((T, N)) < 0.08).astype(np.float64))
    acc = model.summarize(rates=True)
    gof = model.time_rescaling(bins=D)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = {}
    for name, fn in [("PosteriorSummary.collect", acc.collect), ("TimeRescaling.collect", gof.collect)]:
        fn()
        out[name] = ms_stats([wall(fn) for _ in range(reps)])
    eng = model.engine
    eng.profile = True
    gof.collect()
    acc.collect()
    out["stages_ms"] = {k: v["ms"] / v["calls"] for k, v in eng.collect_timings().items()}
    eng.profile = False
    out["ks_mean_range"] = [float(np.nanmin(gof.ks_mean)), float(np.nanmax(gof.ks_mean))]
    out["band_range"] = [float(gof.band.min()), float(gof.band.max())]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-model", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = dict(N=args.N, B=args.B, T=args.T, D=args.D, reps=args.reps, device=torch.cuda.get_device_name(0), boxes=1, source_hash=_lib.source_hash(),
               unit="ms; kernels: HIP events around one call (a fold = every launch of pgl_rescale_fold); model: wall time of the call",
               copy_TBps=COPY_TBS)
    out["kernels"] = kernels(args.N, args.T, args.D, args.reps)
    torch.cuda.empty_cache()
    if not args.no_model:
        out["model"] = end_to_end(args.N, args.B, args.T, args.D, max(2, args.reps // 2))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
