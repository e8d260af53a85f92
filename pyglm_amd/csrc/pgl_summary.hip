// Posterior accumulators for gfx950: running moments of the rates, of the per-cell log-likelihood term and of the chain state, folded once per
// collected sample, so that nothing of size T x N leaves the GPU (the reference stacks the samples on the host: examples/synthetic.py:51-84).
//
// pgl_summary_fold is ONE pass over a data set's Psi.  It is HBM-bound: per cell it reads psi and y (16 B; + 24 B of a | b | log c in the hooks
// mode), reads and writes the two rate accumulators (16 + 16 B) and, with the pointwise accumulators, four more (32 + 32 B).  Lane = neuron
// column, wave = time bin: a wave touches 64 consecutive doubles of a row in every array (they share the leading dimension).  The
// log-likelihood goes through the shared walk of pgl_obs.h (block shape, partials, order of addition, and the per-cell terms), as
// pg_loglik_kernel / pg_loglik_narrow_kernel do, so the per-neuron totals are those of pgl_pg_loglik_ex / pgl_gaussian_stats bit for bit.
#include "pgl_common.h"
#include "pgl_obs.h"

namespace {

// Welford step k (1-based) of (mean, M2) at index i with the new value x
__device__ __forceinline__ void welford(double* __restrict__ mean, double* __restrict__ M2, long i, double x, double k) {
    const double m0 = mean[i], d = x - m0, m1 = m0 + d / k;
    mean[i] = m1;
    M2[i] += d * (x - m1);
}

// one cell (t, n): adds its log-likelihood term (Gaussian: its squared residual, as pgl_gaussian_stats) to ll and folds the rate and the
// pointwise term into their accumulators
__device__ __forceinline__ void fold_cell(const PglSummaryFold& f, int n, long t, double& ll) {
    const long i = t * f.ldpsi + n;
    const double bn = f.bias ? f.bias[n] : 0.0;
    const double psi = f.Psi[i] + bn;
    const double y = f.Y[i];
    const double kd = (double)f.k;
    double l;
    if (f.obs == 2) {
        double omega, kappa;
        const double ie = f.inv_eta[n], r = gauss_cell(y, psi, ie, ll, omega, kappa);
        l = -0.5 * log(6.283185307179586 / ie) - 0.5 * (r * r) * ie;      // regression.py:399-403 with eta = 1 / inv_eta
    } else {
        double a, b, logc;
        pg_abc(f, n, t, y, a, b, logc);
        l = pg_ll_term(logc, a, b, psi);
        ll += l;
    }
    if (f.rmean) {
        const int code = f.link ? f.link[n] : f.link0;
        const double par = f.link_par ? f.link_par[n] : f.link_par0;
        double x = psi;                                                    // E[y | psi] as models.means defines it (models.py:153-163)
        if (code == 0) x = 1.0 / (1.0 + exp(-psi));
        else if (code == 2) x = par * exp(psi);
        else if (code == 3) x = par * (1.0 / (1.0 + exp(-psi)));
        welford(f.rmean, f.rM2, i, x, kd);
    }
    if (f.lmean) {
        welford(f.lmean, f.lM2, i, l, kd);
        if (f.k == 1) {
            f.lse_m[i] = l; f.lse_s[i] = 1.0;
        } else {
            const double m0 = f.lse_m[i], m1 = fmax(m0, l);
            f.lse_m[i] = m1;
            f.lse_s[i] = f.lse_s[i] * exp(m0 - m1) + exp(l - m1);
        }
    }
}

// OBS is a template parameter of the kernels: f.obs = OBS (what pgl_k_summary_fold's switch launched) makes the model a constant, one
// observation model's arithmetic per instantiation.  The Bernoulli, Gaussian and hooks passes carry no lgamma and fit 80-106 VGPRs, 4-6
// waves per SIMD; with every model in one kernel all of them ran at 244 VGPRs, 2 waves per SIMD, too few to cover the HBM latency.  The
// lgamma modes (obs 1, 3) stay at 220 VGPRs and are VALU-bound.
template <int OBS>
__global__ __launch_bounds__(256) void summary_fold_kernel(PglSummaryFold f) {
    f.obs = OBS;
    psi_walk(f.T, f.nloc, f.llpart, [&](int n, long t, double& ll) { fold_cell(f, n, t, ll); });
}

template <int OBS>
__global__ __launch_bounds__(256) void summary_fold_narrow_kernel(PglSummaryFold f) {
    f.obs = OBS;
    psi_walk_narrow(f.T, f.nloc, f.llpart, [&](int n, long t, double& ll) { fold_cell(f, n, t, ll); });
}

// per-neuron sums over time of V [T][ldv]: block partials of the same walk, added up by colsum_partials_kernel
__global__ __launch_bounds__(256) void summary_colpart_kernel(const double* __restrict__ V, long ldv, int T, int nloc, double* __restrict__ part) {
    psi_walk(T, nloc, part, [&](int n, long t, double& s) { s += V[t * ldv + n]; });
}

// the shard's state: one thread per entry (n, d) of the effective weights a * W -- read from the k-major copy the activation contracts with --
// with the edge count of (n, m) taken by the thread of its first basis function, and one thread per bias behind them
__global__ __launch_bounds__(256) void summary_state_kernel(const int* __restrict__ a, const double* __restrict__ Wt, long ldw,
                                                            const double* __restrict__ bias, double* __restrict__ edge, double* __restrict__ wmean,
                                                            double* __restrict__ wM2, double* __restrict__ bmean, double* __restrict__ bM2, int N, int B,
                                                            int nloc, int k) {
    const long D = (long)N * B;
    const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const double kd = (double)k;
    if (idx < nloc * D) {
        const int n = (int)(idx / D);
        const long d = idx - n * D;
        welford(wmean, wM2, idx, Wt[d * ldw + n], kd);
        if (d % B == 0) {
            const long e = (long)n * N + d / B;
            edge[e] += a[e] != 0 ? 1.0 : 0.0;
        }
    } else if (idx < nloc * D + nloc) {
        const int n = (int)(idx - nloc * D);
        welford(bmean, bM2, n, bias[n], kd);
    }
}

}  // namespace

template <int OBS>
static void launch_fold(const PglSummaryFold& f, hipStream_t st) {
    const bool narrow = psi_narrow(f.nloc, OBS);
    if (narrow) hipLaunchKernelGGL(summary_fold_narrow_kernel<OBS>, psi_grid(f.T, f.nloc, narrow), dim3(256), 0, st, f);
    else hipLaunchKernelGGL(summary_fold_kernel<OBS>, psi_grid(f.T, f.nloc, narrow), dim3(256), 0, st, f);
}

int pgl_k_summary_fold(const PglSummaryFold& f, hipStream_t st) {
    switch (f.obs) {
        case 0: launch_fold<0>(f, st); break;
        case 1: launch_fold<1>(f, st); break;
        case 2: launch_fold<2>(f, st); break;
        case 3: launch_fold<3>(f, st); break;
        default: launch_fold<4>(f, st); break;
    }
    PGL_CHECK_LAUNCH();
    return pgl_k_colsum_partials(f.llpart, psi_row_blocks(f.T), f.nloc, f.ll_out, f.accumulate, st);
}

int pgl_k_summary_state(const int* a, const double* Wt, long ldw, const double* bias, double* edge, double* wmean, double* wM2, double* bmean,
                        double* bM2, int N, int B, int nloc, int k, hipStream_t st) {
    const long total = (long)nloc * N * B + nloc;
    hipLaunchKernelGGL(summary_state_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, Wt, ldw, bias, edge, wmean, wM2, bmean, bM2,
                       N, B, nloc, k);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}

int pgl_k_summary_colsum(const double* V, long ldv, int T, int nloc, double* part, double* out, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL(summary_colpart_kernel, psi_grid(T, nloc, false), dim3(256), 0, st, V, ldv, T, nloc, part);
    PGL_CHECK_LAUNCH();
    return pgl_k_colsum_partials(part, psi_row_blocks(T), nloc, out, accumulate, st);
}
