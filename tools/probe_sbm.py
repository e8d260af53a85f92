"""Time of the block-model update (pgl_sbm.hip) on one box:
  * the device update -- upload of A as bytes, pgl_sbm_block_counts, the tables' upload and pgl_sbm_scan (pre-pass, transpose, scan) -- at
    N = 4, 128, 1024, 4096 and K = 8, beside sbm.sbm_host (the NumPy definition) on the same inputs in the same run: HIP events around the
    device calls, wall time of sbm_host with and without the device driver.  THE GATE: at N = 1024 the device update (wall, everything
    included) is faster than the host definition;
  * the scan's time per neuron beside pgl_conditional_simulate's time per bin at F = 1, R = 1, the project's other single-workgroup chain
    (recorded, not gated);
  * resample_model() with SBMSparseNetwork(K = 8) beside NIWSparseNetwork at the BASELINE configs[1] and configs[0] shapes: wall time over
    2 runs after a warm-up, and the ratio.

    python tools/probe_sbm.py [--K 8] [--reps 5] [--no-model] [--out profiles/sbm_probe.json]
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
from pyglm_amd import _lib, sbm  # noqa: E402
from pyglm_amd._lib import call, ptr  # noqa: E402
from pyglm_amd.utils.basis import cosine_basis  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def mean_ms(fn, reps):
    fn()
    return float(np.mean([timed(fn) for _ in range(reps)]))


def update(N, K, reps):
    rng = np.random.default_rng(N)
    A = rng.random((N, N)) < 0.1
    z0 = rng.integers(0, K, size=N)
    P, pi = rng.uniform(0.02, 0.3, size=(K, K)), rng.dirichlet(np.ones(K))
    t = sbm.tables(P, pi)
    drv = sbm.DeviceSBM(N, K)
    out = dict(N=N, K=K)
    out["upload_ms"] = mean_ms(lambda: drv.load(A), reps)
    out["counts_ms"] = mean_ms(lambda: drv.counts(z0), reps)                       # with the read-back of the K^2 + K + 1 counts
    out["scan_ms"] = mean_ms(lambda: drv.scan(z0, *t, 1, 2), reps)                 # tables up, pre-pass, transpose, scan, z back
    out["device_events_ms"] = out["upload_ms"] + out["counts_ms"] + out["scan_ms"]
    out["scan_us_per_neuron"] = 1e3 * out["scan_ms"] / N

    def whole(driver):
        return lambda: sbm.sbm_host(A, z0, K, np.random.RandomState(0), seed=1, sweep=2, driver=driver)
    whole(drv)()
    out["device_update_wall_ms"] = 1e3 * float(np.mean([wall(whole(drv)) for _ in range(reps)]))
    out["host_update_wall_ms"] = 1e3 * float(np.mean([wall(whole(None)) for _ in range(max(1, reps if N <= 1024 else 1))]))
    out["host_over_device"] = out["host_update_wall_ms"] / out["device_update_wall_ms"]
    same = np.array_equal(whole(drv)()["z"], whole(None)()["z"])
    out["device_z_equals_host_z"] = bool(same)
    return out


def conditional_chain(bins, reps):
    """pgl_conditional_simulate at F = 1, R = 1 (N = 1024, B = 5, L = 100): microseconds per bin"""
    B, L, F, R = 5, 100, 1, 1
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    f64 = dict(dtype=torch.float64, device=dev)
    Wff = torch.from_numpy(rng.standard_normal((F, F * B)) / 32.0).to(dev)
    base = torch.from_numpy(-2.0 + 0.3 * rng.standard_normal((bins, F))).to(dev)
    basis = torch.from_numpy(np.ascontiguousarray(cosine_basis(B, L=L) / L)).to(dev)
    neuron = torch.zeros(F, dtype=torch.int32, device=dev)
    kf, pf = torch.zeros(F, dtype=torch.int32, device=dev), torch.zeros(F, **f64)
    ring, s, ss = torch.zeros(R, L, F, **f64), torch.zeros(R, F, **f64), torch.zeros(R, F, **f64)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    t = [0]

    def cond():
        call("pgl_conditional_simulate", ptr(Wff), ptr(base), F, ptr(basis), F, B, L, ptr(kf), ptr(pf), ptr(neuron), R, 0, 1, ptr(ring), None, 0,
             None, 0, ptr(s), ptr(ss), t[0], bins, ptr(status), st)
        t[0] += bins
    ms = mean_ms(cond, reps)
    assert int(status[0]) == 0, status.tolist()
    return dict(bins=bins, us_per_bin=1e3 * ms / bins)


def model_pair(N, B, L, T, K):
    from pyglm_amd import models as M
    from pyglm_amd import networks as NW
    out = dict(N=N, B=B, L=L, T=T, K=K)
    Y = (np.random.default_rng(1).random((T, N)) < 0.05).astype(float)
    for name, make in (("niw", lambda: NW.NIWSparseNetwork(N, B, rho=0.5)), ("sbm", lambda: NW.SBMSparseNetwork(N, B, K=K))):
        np.random.seed(0)
        model = M.SparseBernoulliGLM(N, B=B, basis=cosine_basis(B, L=L) / L, network=make(), seed=1)
        model.add_data(Y)
        for _ in range(2):
            model.resample_model()
        out["%s_resample_model_s" % name] = [wall(model.resample_model) for _ in range(2)]
        out["%s_resample_network_s" % name] = [wall(model.resample_network) for _ in range(2)]
        del model
        torch.cuda.empty_cache()
    out["sbm_over_niw"] = float(np.mean(out["sbm_resample_model_s"]) / np.mean(out["niw_resample_model_s"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--N", type=int, nargs="*", default=[4, 128, 1024, 4096])
    ap.add_argument("--no-model", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.load()
    out = dict(K=args.K, reps=args.reps, device=torch.cuda.get_device_name(0), boxes=1, source_hash=_lib.source_hash(),
               unit="kernels: HIP events, mean of reps after a warm-up, milliseconds; updates and model calls: wall time")
    out["update"] = {"N%d" % N: update(N, args.K, args.reps) for N in args.N}
    out["conditional_simulate_F1_R1"] = conditional_chain(2000, args.reps)
    if "N1024" in out["update"]:
        u = out["update"]["N1024"]
        out["scan_per_neuron_over_conditional_per_bin"] = u["scan_us_per_neuron"] / out["conditional_simulate_F1_R1"]["us_per_bin"]
        out["gate_device_faster_than_host_at_N1024"] = bool(u["device_update_wall_ms"] < u["host_update_wall_ms"])
    if not args.no_model:
        out["model_configs1"] = model_pair(128, 5, 100, 50000, args.K)
        out["model_configs0"] = model_pair(4, 1, 100, 10000, args.K)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    if out.get("gate_device_faster_than_host_at_N1024") is False:
        sys.exit("the gate failed: the device update at N = 1024 is not faster than the host definition")


if __name__ == "__main__":
    main()
