"""Time of the dispersion fold (pgl_dispersion_fold) beside the time-rescaling fold (pgl_rescale_fold, D = 64) on the same Psi and Y in the
same run -- both read 16 B per cell; the gate is dispersion <= 1.1 x rescale --; a column that holds one cell of 100 000 beside the same
column without it (what the cooperative path buys: the lane-per-column walk would serialise its wave behind that cell); and end to end at
the BASELINE configs[3] shape: a sweep with xi learned beside a sweep with xi fixed, the xi step alone (activation + fold + host draw), and
PosteriorSummary.collect(), which pays the same activation.  HIP events around the kernel calls, wall time around the model calls; one
warm-up, mean of --reps.  A missed gate is written into the result as missed.

    python tools/probe_dispersion.py [--N 1024] [--T 100000] [--reps 5] [--model-N 512] [--model-T 100000] [--out profiles/dispersion_probe.json]
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
from pyglm_amd import _lib, dispersion  # noqa: E402
from pyglm_amd._lib import call, ptr  # noqa: E402

COPY_TBS = 6.3      # what a device-to-device copy reaches on MI355X (TB/s): the yardstick for a streaming kernel
GATE = 1.1


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


def kernels(N, T, reps, xi=2.0, mean=0.1, D=64):
    lib = _lib.load()
    ldn = N + (N & 1)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    g = torch.Generator(device=dev).manual_seed(0)
    Psi = torch.randn(T, ldn, dtype=torch.float64, device=dev, generator=g) * 0.5 + float(np.log(mean / xi))
    Y = torch.empty(T, ldn, dtype=torch.float64, device=dev)
    for lo in range(0, T, 8192):                                   # NB(xi, sigma(psi)) counts, drawn on the host in slabs
        psi = Psi[lo:lo + 8192].cpu().numpy()
        Y[lo:lo + 8192] = torch.from_numpy(rng.negative_binomial(xi, 1.0 / (1.0 + np.exp(psi))).astype(np.float64)).to(dev)
    bias = torch.zeros(N, dtype=torch.float64, device=dev)
    xid = torch.full((N,), xi, dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    hist = torch.zeros(N, D, dtype=torch.int32, device=dev)
    zsum = torch.zeros(N, 2, dtype=torch.float64, device=dev)
    Ld, Sd = torch.zeros(N, dtype=torch.int64, device=dev), torch.zeros(N, dtype=torch.float64, device=dev)
    work_r = torch.empty(lib.pgl_rescale_work_bytes(N, T), dtype=torch.uint8, device=dev)
    work_d = torch.empty(lib.pgl_dispersion_work_bytes(N, T), dtype=torch.uint8, device=dev)

    def rescale_fold(k):
        call("pgl_rescale_fold", ptr(Psi), ldn, ptr(bias), ptr(Y), T, N, None, xi, D, 1, k - 1, 0, 0, ptr(hist), ptr(zsum), 0, ptr(work_r), st)

    def disp_fold(k, nloc=N, Yp=None):
        call("pgl_dispersion_fold", Psi=ptr(Psi), ldn=ldn, bias=ptr(bias), Y=ptr(Y if Yp is None else Yp), T=T, nloc=nloc, xi=ptr(xid), seed=1, sweep=k,
             neuron0=0, elem0=0, L=ptr(Ld), S=ptr(Sd), accumulate=0, work=ptr(work_d), hip_stream=st)

    res = dict(rows_per_workgroup=dispersion.ROWS, cooperative_above=dispersion.COOP_COUNT, work_bytes=int(work_d.numel()), xi=xi,
               mean_count=float(Y[:, :N].mean()), cells_of_two_or_more=float((Y[:, :N] >= 2).double().mean()))
    rescale_fold(1)
    res["pgl_rescale_fold"] = dict(ms_stats([timed(lambda: rescale_fold(2 + r)) for r in range(reps)]), bytes_per_cell=16)
    disp_fold(1)
    res["pgl_dispersion_fold"] = dict(ms_stats([timed(lambda: disp_fold(2 + r)) for r in range(reps)]), bytes_per_cell=16)
    for name in ("pgl_rescale_fold", "pgl_dispersion_fold"):
        gbs = 16.0 * T * N / (res[name]["ms_mean"] * 1e-3) / 1e9
        res[name].update(GBps=gbs, fraction_of_copy=gbs / (COPY_TBS * 1e3))
    ratio = res["pgl_dispersion_fold"]["ms_mean"] / res["pgl_rescale_fold"]["ms_mean"]
    res["dispersion_over_rescale"] = ratio
    res["gate"] = dict(bound=GATE, met=bool(ratio <= GATE), verdict="met" if ratio <= GATE else "MISSED")
    # the last fold against the definition on a few columns
    cols = list(range(min(N, 2)))
    want = dispersion.dispersion_host(Psi[:, cols].cpu().numpy(), Y[:, cols].cpu().numpy(), xi, 1, 1 + reps, 0, 0)
    assert np.array_equal(Ld.cpu().numpy()[cols], want[0]) and np.allclose(Sd.cpu().numpy()[cols], want[1], rtol=1e-10)
    # 64 columns, one of which holds one cell of 100 000, beside the same columns without it
    Y1 = Y.clone()
    disp_fold(1, 64)
    res["columns_64"] = ms_stats([timed(lambda: disp_fold(2 + r, 64)) for r in range(reps)])
    Y1[T // 2, 5] = 100000.0
    disp_fold(1, 64, Y1)
    res["columns_64_with_one_cell_of_100000"] = ms_stats([timed(lambda: disp_fold(2 + r, 64, Y1)) for r in range(reps)])
    res["one_cell_of_100000_costs_ms"] = res["columns_64_with_one_cell_of_100000"]["ms_mean"] - res["columns_64"]["ms_mean"]
    return res


def end_to_end(N, B, T, reps, xi=2.0):
    from pyglm_amd.models import NegativeBinomialGLM
    from pyglm_amd.utils.basis import cosine_basis
    Y = np.random.default_rng(1).negative_binomial(2, 0.85, size=(T, N)).astype(np.float64)     # bench.py's configs[3] counts, mean 0.35

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = {}
    for label, prior in (("xi_fixed", None), ("xi_learned", (1.0, 1.0))):
        np.random.seed(0)
        kw = dict(S_w=1.0, mu_b=-2.0, xi=xi)
        if prior:
            kw["xi_prior"] = prior
        model = NegativeBinomialGLM(N, basis=cosine_basis(B, L=100) / 100, seed=0, regression_kwargs=kw)
        model.add_data(Y)
        model.resample_model()
        out["sweep_" + label] = ms_stats([wall(model.resample_model) for _ in range(reps)])
        out["xi_range_" + label] = [float(np.min([r.xi for r in model.regressions])), float(np.max([r.xi for r in model.regressions]))]
        model.engine.profile = True                                # the next sweep of the chain, every stage timed with HIP events
        model.resample_model()
        out["sweep_stages_ms_" + label] = {k: v["ms"] for k, v in model.engine.collect_timings().items()}
        model.engine.profile = False
        if prior:
            a, W, b = model._local_state()
            step = lambda: model._resample_xi(a, W, b)
            step()
            out["xi_step"] = ms_stats([wall(step) for _ in range(reps)])
            acc = model.summarize(rates=True)
            acc.collect()
            out["PosteriorSummary.collect"] = ms_stats([wall(acc.collect) for _ in range(reps)])
            eng = model.engine
            eng.profile = True
            step()
            out["xi_step_stages_ms"] = {k: v["ms"] / v["calls"] for k, v in eng.collect_timings().items()}
            eng.profile = False
            out["xi_last"] = [float(np.min([r.xi for r in model.regressions])), float(np.max([r.xi for r in model.regressions]))]
        del model
        torch.cuda.empty_cache()
    out["xi_step_over_sweep"] = out["xi_step"]["ms_mean"] / out["sweep_xi_fixed"]["ms_mean"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model-N", type=int, default=512)
    ap.add_argument("--model-B", type=int, default=5)
    ap.add_argument("--model-T", type=int, default=100000)
    ap.add_argument("--no-model", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = dict(N=args.N, T=args.T, reps=args.reps, device=torch.cuda.get_device_name(0), boxes=1, source_hash=_lib.source_hash(),
               unit="ms; kernels: HIP events around one call (a fold = both launches); model: wall time of the call", copy_TBps=COPY_TBS)
    out["kernels"] = kernels(args.N, args.T, args.reps)
    torch.cuda.empty_cache()
    if not args.no_model:
        out["model"] = dict(N=args.model_N, B=args.model_B, T=args.model_T, **end_to_end(args.model_N, args.model_B, args.model_T, max(2, args.reps // 2)))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
