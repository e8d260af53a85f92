// Posterior accumulators for gfx950: running moments of the rates, of the per-cell log-likelihood term and of the chain state, folded once per
// collected sample, so that nothing of size T x N leaves the GPU (the reference stacks the samples on the host: examples/synthetic.py:51-84).
//
// pgl_summary_fold is ONE pass over a data set's Psi.  It is HBM-bound: per cell it reads psi and y (16 B; + 24 B of a | b | log c in the hooks
// mode), reads and writes the two rate accumulators (16 + 16 B) and, with the pointwise accumulators, four more (32 + 32 B).  Lane = neuron
// column, wave = time bin, as in pg_loglik_kernel: a wave touches 64 consecutive doubles of a row in every array (they share the leading
// dimension).  The log-likelihood goes through the block shape, the partials and the order of addition of pg_loglik_kernel /
// pg_loglik_narrow_kernel (pgl_obs.h has the shared terms), so the per-neuron totals are those of pgl_pg_loglik_ex / pgl_gaussian_stats bit for
// bit; the grid is therefore one block per PGLL_ROWS time bins and column group, not a capped grid-stride.  No atomics: every cell has one owner.
#include "pgl_common.h"
#include "pgl_obs.h"

namespace {

// (OBS is a template parameter of the kernels: one observation model's arithmetic per instantiation, and the row loop is not unrolled.  The
// Bernoulli, Gaussian and hooks passes carry no lgamma and fit 80-106 VGPRs, 4-6 waves per SIMD; with every model in one kernel all of them
// ran at 244 VGPRs, 2 waves per SIMD, too few to cover the HBM latency.  The lgamma modes (obs 1, 3) stay at 220 VGPRs and are VALU-bound.)
template <int OBS>
__device__ __forceinline__ PgLlArgs obs_args(const PglSummaryFold& f) {
    PgLlArgs g{};
    g.obs = OBS; g.xi = f.xi; g.param = f.param; g.hooks = f.hooks; g.ldh = f.ldh;
    return g;
}

// Welford step k (1-based) of (mean, M2) at index i with the new value x
__device__ __forceinline__ void welford(double* __restrict__ mean, double* __restrict__ M2, long i, double x, double k) {
    const double m0 = mean[i], d = x - m0, m1 = m0 + d / k;
    mean[i] = m1;
    M2[i] += d * (x - m1);
}

// one cell (t, n): adds its log-likelihood term (Gaussian: its squared residual, as pgl_gaussian_stats) to ll and folds the rate and the
// pointwise term into their accumulators
template <int OBS>
__device__ __forceinline__ void fold_cell(const PglSummaryFold& f, const PgLlArgs& g, int n, long t, double& ll) {
    const long i = t * f.ld + n;
    const double bn = f.bias ? f.bias[n] : 0.0;
    const double psi = f.Psi[i] + bn;
    const double y = f.Y[i];
    const double kd = (double)f.k;
    double l;
    if (OBS == 2) {
        const double ie = f.inv_eta[n], r = y - psi;
        ll += r * r;
        l = -0.5 * log(6.283185307179586 / ie) - 0.5 * (r * r) * ie;      // regression.py:399-403 with eta = 1 / inv_eta
    } else {
        double a, b, logc;
        pg_abc(g, n, t, y, a, b, logc);
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

// block shape and order of addition of pg_loglik_kernel
template <int OBS>
__global__ __launch_bounds__(256) void summary_fold_kernel(PglSummaryFold f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y * 64 + lane;
    const int t0 = blockIdx.x * PGLL_ROWS;
    __shared__ double red[4][64];
    const PgLlArgs g = obs_args<OBS>(f);
    double ll = 0.0;
    if (n < f.nloc) {
#pragma unroll 1
        for (int r = wave; r < PGLL_ROWS; r += 4) {
            const int t = t0 + r;
            if (t >= f.T) break;
            fold_cell<OBS>(f, g, n, t, ll);
        }
    }
    red[wave][lane] = ll;
    __syncthreads();
    if (wave == 0 && n < f.nloc) f.llpart[(long)blockIdx.x * f.nloc + n] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// the same for a narrow shard (fewer than 64 local neurons), in the shape and order of pg_loglik_narrow_kernel
template <int OBS>
__global__ __launch_bounds__(256) void summary_fold_narrow_kernel(PglSummaryFold f) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nl = f.nloc;                                    // < 64
    const int t0 = blockIdx.x * PGLL_ROWS;
    __shared__ double term[PGLL_ROWS][64];
    __shared__ double red[4][64];
    const PgLlArgs g = obs_args<OBS>(f);
#pragma unroll 1
    for (int c = tid; c < PGLL_ROWS * nl; c += 256) {
        const int r = c / nl, n = c - r * nl, t = t0 + r;
        double v = 0.0;
        if (t < f.T) fold_cell<OBS>(f, g, n, t, v);
        term[r][n] = v;
    }
    __syncthreads();
    double ll = 0.0;
    if (lane < nl)
        for (int r = wave; r < PGLL_ROWS; r += 4) {
            if (t0 + r >= f.T) break;
            ll += term[r][lane];
        }
    red[wave][lane] = ll;
    __syncthreads();
    if (wave == 0 && lane < nl) f.llpart[(long)blockIdx.x * nl + lane] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// per-neuron sums over time of V [T][ldv]: block partials in the shape above (a column's partial never depends on its neighbours or on
// how many there are), added up by colsum_partials_kernel
__global__ __launch_bounds__(256) void summary_colpart_kernel(const double* __restrict__ V, long ldv, int T, int nloc, double* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y * 64 + lane;
    const int t0 = blockIdx.x * PGLL_ROWS;
    __shared__ double red[4][64];
    double s = 0.0;
    if (n < nloc)
        for (int r = wave; r < PGLL_ROWS; r += 4) {
            const int t = t0 + r;
            if (t >= T) break;
            s += V[(long)t * ldv + n];
        }
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && n < nloc) part[(long)blockIdx.x * nloc + n] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
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
static void launch_fold(const PglSummaryFold& f, int nblk, hipStream_t st) {
    if (f.nloc < 64 && OBS != 2) hipLaunchKernelGGL(summary_fold_narrow_kernel<OBS>, dim3(nblk), dim3(256), 0, st, f);
    else hipLaunchKernelGGL(summary_fold_kernel<OBS>, dim3(nblk, (f.nloc + 63) / 64), dim3(256), 0, st, f);
}

int pgl_k_summary_fold(const PglSummaryFold& f, hipStream_t st) {
    const int nblk = (f.T + PGLL_ROWS - 1) / PGLL_ROWS;
    switch (f.obs) {
        case 0: launch_fold<0>(f, nblk, st); break;
        case 1: launch_fold<1>(f, nblk, st); break;
        case 2: launch_fold<2>(f, nblk, st); break;
        case 3: launch_fold<3>(f, nblk, st); break;
        default: launch_fold<4>(f, nblk, st); break;
    }
    PGL_CHECK_LAUNCH();
    return pgl_k_colsum_partials(f.llpart, nblk, f.nloc, f.ll_out, f.accumulate, st);
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
    const int nblk = (T + PGLL_ROWS - 1) / PGLL_ROWS;
    hipLaunchKernelGGL(summary_colpart_kernel, dim3(nblk, (nloc + 63) / 64), dim3(256), 0, st, V, ldv, T, nloc, part);
    PGL_CHECK_LAUNCH();
    return pgl_k_colsum_partials(part, nblk, nloc, out, accumulate, st);
}
