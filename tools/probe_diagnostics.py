"""Time and bandwidth of the chain diagnostics' fold (pgl_diag_fold, all four sections) at its cheapest sample (k = 1: one level) and its
worst (k = 128 with 8 levels: every level), beside pgl_summary_state on the same state in the same run -- all three are streaming passes
with no reuse, so the gate is a bandwidth ratio: the fold's achieved TB/s at k = 128 is at least two thirds of pgl_summary_state's --; the
two launches of pgl_diag_edge_conditional; then, on a model of the same size, ChainDiagnostics.collect() beside PosteriorSummary.collect()
(wall time) and the device bytes the accumulators hold.  HIP events around the kernel calls; one warm-up, mean of --reps.  A missed gate is
written into the result as MISSED.

Bytes moved, per entry: 40 per touched level (pending read or written, mean and M2 read and written) plus the entry's value -- 4 (a) for an
edge, 8 (p) for a conditional, 8 + 4 / B (W and its edge's a) for a weight, 8 for a bias.  pgl_summary_state: 40 per weight (the k-major
copy read, two moments read and written), 20 per edge (a read, the count read and written), 40 per bias.

    python tools/probe_diagnostics.py [--N 1024] [--B 5] [--levels 8] [--reps 5] [--model-T 1000] [--no-model] [--out profiles/diagnostics_probe.json]
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
GATE = 2.0 / 3.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms, nbytes):
    ms = np.asarray(ms)
    tbs = nbytes / (ms.mean() * 1e-3) / 1e12
    return dict(ms_mean=float(ms.mean()), ms_min=float(ms.min()), ms_max=float(ms.max()), bytes=int(nbytes), TBps=float(tbs),
                fraction_of_copy=float(tbs / COPY_TBS))


def kernels(N, B, levels, reps):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    nloc, D = N, N * B
    Dp, ldn = (D + 1 + 15) // 16 * 16, N + (N & 1)
    f64 = dict(dtype=torch.float64, device=dev)
    a = (torch.rand(nloc, N, device=dev, generator=g) < 0.3).to(torch.int32)
    W = torch.randn(nloc, D, generator=g, **f64)
    b = torch.randn(nloc, generator=g, **f64)
    lo = torch.randn(nloc, N, generator=g, **f64) * 3
    perm = torch.stack([torch.randperm(N, device=dev, generator=g) for _ in range(nloc)]).to(torch.int32)
    p = torch.zeros(nloc, N, **f64)
    Wt = torch.zeros(Dp, ldn, **f64)                             # the k-major copy pgl_summary_state reads
    Wt[:D, :nloc] = (W.view(nloc, N, B) * a[:, :, None]).view(nloc, D).t()
    what = _lib.PGL_DIAG_ALL
    E = lib.pgl_diag_entries(N, B, nloc, what)
    held = lib.pgl_diag_bytes(E, levels)
    pending, mean, M2 = (torch.zeros(levels, E, **f64) for _ in range(3))
    edge, wm, wM2, bm, bM2 = torch.zeros(nloc, N, **f64), torch.zeros(nloc, D, **f64), torch.zeros(nloc, D, **f64), torch.zeros(nloc, **f64), \
        torch.zeros(nloc, **f64)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def fold(k):
        call("pgl_diag_fold", a=ptr(a), W=ptr(W), b=ptr(b), p=ptr(p), pending=ptr(pending), mean=ptr(mean), M2=ptr(M2), N=N, B=B, nloc=nloc,
             levels=levels, k=k, what=what, hip_stream=st)

    def state(k):
        call("pgl_summary_state", a=ptr(a), Wt=ptr(Wt), ldw=ldn, bias=ptr(b), edge=ptr(edge), w_mean=ptr(wm), w_M2=ptr(wM2), b_mean=ptr(bm),
             b_M2=ptr(bM2), N=N, B=B, nloc=nloc, k=k, hip_stream=st)

    def conditional():
        call("pgl_diag_edge_conditional", logodds=ptr(lo), perm=ptr(perm), a=ptr(a), p=ptr(p), nloc=nloc, N=N, hip_stream=st)

    e = nloc * N
    value_bytes = 4 * e + 8 * e + 8 * e * B + 4 * e + 8 * nloc
    k_all = 1 << (levels - 1)                                    # the first sample that touches every level (128 with 8 levels)
    res = dict(entries=int(E), levels=levels, accumulator_bytes=int(held), formula="3 * 8 * levels * nloc * (2 N + N B + 1)")
    conditional()
    res["pgl_diag_edge_conditional"] = stats([timed(conditional) for _ in range(reps)], e * (4 + 8 + 8 + 4 + 8))
    fold(1)
    res["pgl_diag_fold_k1"] = dict(stats([timed(lambda: fold(1)) for _ in range(reps)], 40 * E + value_bytes), levels_touched=1)
    fold(k_all)
    res["pgl_diag_fold_k%d" % k_all] = dict(stats([timed(lambda: fold(k_all)) for _ in range(reps)], 40 * levels * E + value_bytes),
                                            levels_touched=levels)
    state(1)
    res["pgl_summary_state"] = stats([timed(lambda: state(2 + r)) for r in range(reps)], 40 * nloc * D + 20 * e + 40 * nloc)
    ratio = res["pgl_diag_fold_k%d" % k_all]["TBps"] / res["pgl_summary_state"]["TBps"]
    res["fold_over_summary_state_TBps"] = float(ratio)
    res["gate"] = dict(bound=GATE, met=bool(ratio >= GATE), verdict="met" if ratio >= GATE else "MISSED")
    res["note"] = ("a repeated call that moves less than the 256 MiB Infinity Cache holds (the fold at k = 1, pgl_summary_state, the "
                   "conditionals at N = 1024) may be served from it; the fold over every level cannot")
    return res


def end_to_end(N, B, T, levels, reps):
    from pyglm_amd.diagnostics import _DeviceDiag
    from pyglm_amd.models import SparseBernoulliGLM
    from pyglm_amd.utils.basis import cosine_basis
    Y = (np.random.default_rng(1).random((T, N)) < 0.05).astype(np.float64)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def ms(v):
        return dict(ms_mean=float(np.mean(v)), ms_min=float(np.min(v)), ms_max=float(np.max(v)))

    np.random.seed(0)
    model = SparseBernoulliGLM(N, basis=cosine_basis(B, L=100) / 100, seed=0, regression_kwargs=dict(S_w=1.0, mu_b=-2.0))
    model.add_data(Y)
    out = {}
    acc = model.summarize(rates=False)
    acc.collect()
    out["PosteriorSummary.collect(rates=False)"] = ms([wall(acc.collect) for _ in range(reps)])
    plain = model.diagnose(levels=levels, rb=False)
    plain.collect(ll=0.0)
    out["ChainDiagnostics.collect(rb=False)"] = ms([wall(lambda: plain.collect(ll=0.0)) for _ in range(reps)])
    out["accumulator_bytes_rb_False"] = int(_DeviceDiag.bytes(model.engine, levels, plain.sections))
    del plain
    torch.cuda.empty_cache()
    diag = model.diagnose(levels=levels)
    out["accumulator_bytes"] = int(_DeviceDiag.bytes(model.engine, levels, diag.sections))
    out["sweep_ms"], walls = [], []
    for _ in range(2):                                           # the conditionals belong to a sweep: one collect() per sweep
        out["sweep_ms"].append(wall(model.resample_model))
        walls.append(wall(lambda: diag.collect(ll=0.0)))
    out["ChainDiagnostics.collect(rb=True)"] = ms(walls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model-T", type=int, default=1000)
    ap.add_argument("--no-model", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = dict(N=args.N, B=args.B, reps=args.reps, device=torch.cuda.get_device_name(0), boxes=1, source_hash=_lib.source_hash(),
               unit="ms; kernels: HIP events around one call; model: wall time of the call", copy_TBps=COPY_TBS)
    out["kernels"] = kernels(args.N, args.B, args.levels, args.reps)
    torch.cuda.empty_cache()
    if not args.no_model:
        out["model"] = dict(N=args.N, B=args.B, T=args.model_T, levels=args.levels,
                            **end_to_end(args.N, args.B, args.model_T, args.levels, max(2, args.reps // 2)))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
