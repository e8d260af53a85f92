"""generate() end to end: the device path (pyglm_amd/simulate.py, pgl_generate) against the host loop, at the metric's shape (N = 1024,
B = 5, cosine_basis(5, L=100), T = 10^5; the host loop timed over 2000 bins and extrapolated) and at configs[0]'s (N = 4, B = 1, L = 100,
T = 10^4; both paths timed in full).  One JSON line per shape; with --out, the lines also go to that file.
    python tools/probe_generate.py [--out FILE] [--only small|full]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pyglm_amd.models import NonlinearAutoregressiveModel  # noqa: E402
from pyglm_amd.regression import SparseBernoulliRegression  # noqa: E402
from pyglm_amd.utils.basis import cosine_basis  # noqa: E402


def model(N, B, L, seed=0):
    np.random.seed(seed)
    m = NonlinearAutoregressiveModel(N, [SparseBernoulliRegression(N, B, rho=0.0, mu_b=-2.0, S_b=0.1) for _ in range(N)],
                                     basis=cosine_basis(B, L=L) / L)
    _, W, b = m._adopt_state()
    rng = np.random.default_rng(seed)
    W[...] = rng.standard_normal(W.shape) / np.sqrt(N)
    b[:, 0] = -2.0 + 0.3 * rng.standard_normal(N)
    return m


def timed(m, T, gpu):
    np.random.seed(1)
    t = time.perf_counter()
    X, Y = m.generate(keep=False, T=T, gpu=gpu)
    return time.perf_counter() - t, Y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", choices=("small", "full"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the probe times the device path: it needs a GPU"
    lines = []
    shapes = [("small", 4, 1, 100, 10000, 10000), ("full", 1024, 5, 100, 100000, 2000)]
    for name, N, B, L, T, T_host in shapes:
        if args.only and args.only != name:
            continue
        m = model(N, B, L)
        timed(m, min(T, 200), True)                       # warm-up: code objects, pinned buffers
        dev_s, Yd = timed(m, T, True)
        host_s, Yh = timed(m, T_host, False)
        same = bool(np.array_equal(Yd[:T_host], Yh))
        rec = dict(shape=name, N=N, B=B, L=L, T=T, device_s=round(dev_s, 3), device_us_per_bin=round(1e6 * dev_s / T, 2),
                   host_bins_timed=T_host, host_s=round(host_s * T / T_host, 3), host_us_per_bin=round(1e6 * host_s / T_host, 2),
                   host_extrapolated=T_host != T, speedup=round(host_s * T / T_host / dev_s, 1), prefix_equal=same,
                   spike_rate=round(float(Yd.mean()), 4))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
