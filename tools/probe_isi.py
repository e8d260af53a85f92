"""Time of the inter-spike-interval fold (pgl_isi_fold) : the fold of one simulate() chunk beside the pgl_simulate launch that produced the
chunk, for R = 1 and 8 replicates; the fold of a data set's own series (R = 1, N columns, T rows) with its share of the copy rate, and a
narrow series (N = 4) where only the split of time gives any parallelism; and model.simulate(T, replicates=8, keep_paths=False) end to end
with and without isi.  HIP events around the calls, wall time around the model calls; one warm-up, mean of --reps.

    python tools/probe_isi.py [--N 1024] [--B 5] [--L 100] [--D 64] [--T 100000] [--reps 5] [--out profiles/isi_probe.json]
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

COPY_BYTES_PER_S = 6.3e12         # what a copy reaches on these boxes


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


def chunks(N, B, L, D, reps, Rs):
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
        buf = torch.zeros(R, rows, N, **f64)
        ring = torch.zeros(R, L, N, **f64)
        s, ss = torch.zeros(R, N, **f64), torch.zeros(R, N, **f64)
        work = torch.zeros(lib.pgl_simulate_work_bytes(N, B, R), dtype=torch.uint8, device=dev)
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        fold = simulate._IsiFold(dev, st, N, D, R, rows)
        t = [0]

        def sim():
            call("pgl_simulate", ptr(Wm), ptr(bias), ptr(basis), N, B, L, ptr(kind), ptr(par), R, 0, 1, ptr(ring), ptr(buf), rows * N, ptr(s), ptr(ss),
                 t[0], rows, ptr(work), ptr(status), st)
            t[0] += rows

        sim()
        res = dict(rows=rows, bytes=8 * R * rows * N)
        res["pgl_simulate"] = ms_stats([timed(sim) for _ in range(reps)])
        fold.fold(buf, N, rows * N, rows)
        res["pgl_isi_fold"] = ms_stats([timed(lambda: fold.fold(buf, N, rows * N, rows)) for _ in range(reps)])
        assert int(status[0]) == 0, status.tolist()
        res["mean_rate"] = float(s.sum() / (R * N * t[0]))
        res["fold_over_simulate_launch"] = res["pgl_isi_fold"]["ms_mean"] / res["pgl_simulate"]["ms_mean"]
        out["R%d" % R] = res
    return out


def series(N, T, D, reps, rate=0.08):
    """one fold of a whole series (T, N) of Bernoulli(rate) columns, checked against the definition on a few columns"""
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    Y = (torch.rand((T, N), dtype=torch.float64, device=dev) < rate).to(torch.float64)
    fold = simulate._IsiFold(dev, st, N, D, 1, T)

    def run():
        fold.first = True
        fold.fold(Y, N, T * N, T)

    run()
    res = dict(N=N, T=T, bytes=8 * T * N)
    res.update(ms_stats([timed(run) for _ in range(reps)]))
    res["bytes_per_s"] = res["bytes"] / (res["ms_mean"] * 1e-3)
    res["fraction_of_copy_rate"] = res["bytes_per_s"] / COPY_BYTES_PER_S
    hist, moments = fold.finish()
    cols = list(range(min(N, 4)))
    want = simulate.isi_host(Y[:, cols].cpu().numpy(), D)
    assert np.array_equal(hist[0, cols], want[0]) and np.array_equal(moments[0, cols], want[1])
    return res


def end_to_end(N, B, L, D, T, R):
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
    model.simulate(600, replicates=R, keep_paths=False, gpu=True, isi=D)
    out["simulate_s"] = [wall(lambda: model.simulate(T, replicates=R, seed=k, keep_paths=False, gpu=True)) for k in range(2)]
    out["simulate_isi_s"] = [wall(lambda: model.simulate(T, replicates=R, seed=k, keep_paths=False, gpu=True, isi=D)) for k in range(2)]
    plain, isi = float(np.mean(out["simulate_s"])), float(np.mean(out["simulate_isi_s"]))
    out["isi_adds_s"] = isi - plain
    out["isi_adds_over_simulate"] = (isi - plain) / plain
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--R", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--no-model", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = dict(N=args.N, B=args.B, L=args.L, D=args.D, T=args.T, reps=args.reps, device=torch.cuda.get_device_name(0), boxes=1,
               source_hash=_lib.source_hash(), segment_rows=_lib.load().pgl_isi_segment_rows(),
               unit="kernels: HIP events around one call (a fold = every launch of pgl_isi_fold), milliseconds; model: wall seconds of the call")
    out["chunks"] = chunks(args.N, args.B, args.L, args.D, args.reps, args.R)
    torch.cuda.empty_cache()
    out["series"] = series(args.N, args.T, args.D, args.reps)
    out["series_narrow"] = series(4, 10000, args.D, args.reps)
    torch.cuda.empty_cache()
    if not args.no_model:
        out["model"] = end_to_end(args.N, args.B, args.L, args.D, args.T, 8)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
