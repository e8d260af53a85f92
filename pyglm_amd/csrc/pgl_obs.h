// A pass over Psi, shared by the kernels that make one (pgl_elementwise.hip: PG draws + log-likelihood; pgl_summary.hip: the posterior
// accumulators): ONE argument block, ONE definition of a(y), b(y), log c(y) and of the log-likelihood term, and ONE walk -- who owns which
// cell and in which order a column's terms are added -- so that every pass rounds alike and adds in the same order: a neuron's total has the
// same bits whatever the pass and whatever the shard.
#pragma once
#include "pgl_common.h"

// Each block covers PGLL_ROWS time bins of one 64-neuron column group and leaves one partial per neuron; a second pass
// (pgl_k_colsum_partials) adds the partials in a fixed order.
constexpr int PGLL_ROWS = 64;

// ------------------------------------------------------------------ the argument block
// the observation model of a pass: what pg_abc reads
struct PgObs {
    int obs;                            // 0 Bernoulli (a=y,b=1,c=1)  1 negative binomial (a=y, b=y+xi, c=C(y+xi-1,y))
                                        // 2 Gaussian (regression.py:380-446): omega = 1/eta, kappa = y/eta, "ll" = sum of squared residuals
                                        // 3 binomial (a=y, b=n, c=C(n,y))  4 hooks: a, b, log c read from `hooks`
    double xi;                          // xi (obs 1) or n (obs 3) where param is null
    const double* param;                // optional [nloc]: xi (obs 1) or n (obs 3) per neuron
    const double* hooks; long ldh;      // obs 4: [T][3 ldh] = a | b | log c of the local neurons
};
struct PsiPass : PgObs {
    double* Psi; long ldpsi;            // [T][ldpsi] X.w as pgl_activation left it (bias not added)
    const double* bias;                 // [nloc], or null
    const double* Y; long ldy;          // spikes/counts of the local neurons: Y[t*ldy + n]
    double* llpart;                     // [psi_row_blocks(T)][nloc] the blocks' partial sums
    int T, nloc;
    const double* inv_eta;              // [nloc] 1/eta per neuron (obs == 2 only)
};
// PG draws + log-likelihood (pgl_elementwise.hip): writes psi = X.w + bias back to Psi
struct PgLlArgs : PsiPass {
    double* Omega; long ldo;            // out [T][ldo]   (may be null: log-likelihood only)
    double* Kappa; long ldk;            // out [T][ldk]   (may be null)
    uint64_t seed, sweep, neuron0, elem0;
};
// posterior accumulators (pgl_summary.hip): Psi is only read; ldy = ldpsi, and the accumulators share it
struct PglSummaryFold : PsiPass {
    double* ll_out; int accumulate;
    double* rmean; double* rM2;         // rates: Welford mean / M2 of E[y | psi], or null
    const int* link; int link0;         // link code per neuron, or null: link0 for all (0 logistic, 1 identity, 2 par * exp, 3 par * logistic)
    const double* link_par; double link_par0;
    double* lmean; double* lM2; double* lse_m; double* lse_s;   // pointwise: Welford of the term l and its streaming log-sum-exp, or null
    int k;                              // 1-based index of the sample being folded
};
int pgl_k_pg_loglik(const PgLlArgs& a, double* ll_out, int accumulate, hipStream_t st);   // ll_out[n] (+)= the column sums (obs 2: of squared residuals)
int pgl_k_summary_fold(const PglSummaryFold& f, hipStream_t st);

// ------------------------------------------------------------------ launch geometry: one block per PGLL_ROWS bins x 64-neuron column group
inline int psi_row_blocks(int T) { return (T + PGLL_ROWS - 1) / PGLL_ROWS; }
// A NARROW shard (fewer than 64 local neurons: a small model, BASELINE configs[0]) takes psi_walk_narrow: with a lane per neuron most lanes
// would idle and every busy one walk 16 time bins one after the other (0.37 of that sweep's 1.0 ms of GPU time at N = 4).  The Gaussian pass
// always takes the wide walk.
inline bool psi_narrow(int nloc, int obs) { return nloc < 64 && obs != 2; }
inline dim3 psi_grid(int T, int nloc, bool narrow) { return dim3(psi_row_blocks(T), narrow ? 1 : (nloc + 63) / 64); }

// ------------------------------------------------------------------ the walk
// cell(n, t, acc) handles cell (t, n) and adds its term to acc.  Every cell has one owner (no atomics), and the grid is one block per
// PGLL_ROWS bins, not a capped grid-stride: a column's partial never depends on its neighbours, on how many there are, or on the launch.
// The row loops are not unrolled: that is what keeps the accumulator passes at 80-106 VGPRs, and the PG pass, whose cell is thousands of
// instructions, has no use for it.

// the four waves' sums of a column, added in wave order: part[block][n], written where `own`
__device__ __forceinline__ void psi_walk_reduce(double acc, int n, bool own, int nloc, double* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ double red[4][64];
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && own) part[(long)blockIdx.x * nloc + n] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// Lane = neuron column, wave = row: a wave touches 64 consecutive doubles of one time bin; wave w adds rows w, w + 4, ... of the block
template <class Cell>
__device__ __forceinline__ void psi_walk(int T, int nloc, double* part, Cell cell) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y * 64 + lane;
    const int t0 = blockIdx.x * PGLL_ROWS;
    double acc = 0.0;
    if (n < nloc) {
#pragma unroll 1
        for (int r = wave; r < PGLL_ROWS; r += 4) {
            const int t = t0 + r;
            if (t >= T) break;
            cell(n, t, acc);
        }
    }
    psi_walk_reduce(acc, n, n < nloc, nloc, part);
}

// The same for nl < 64 columns: the block's PGLL_ROWS x nl cells are dealt to its 256 threads, each cell's term goes to LDS, and then thread
// (wave, neuron) adds ITS rows' terms in the order psi_walk adds them -- the same numbers in the same order: the same sum to the last bit.
template <class Cell>
__device__ __forceinline__ void psi_walk_narrow(int T, int nl, double* part, Cell cell) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t0 = blockIdx.x * PGLL_ROWS;
    __shared__ double term[PGLL_ROWS][64];
#pragma unroll 1
    for (int c = tid; c < PGLL_ROWS * nl; c += 256) {
        const int r = c / nl, n = c - r * nl, t = t0 + r;
        double v = 0.0;
        if (t < T) cell(n, t, v);
        term[r][n] = v;
    }
    __syncthreads();
    double acc = 0.0;
    if (lane < nl)
        for (int r = wave; r < PGLL_ROWS; r += 4) {
            if (t0 + r >= T) break;
            acc += term[r][lane];
        }
    psi_walk_reduce(acc, lane, lane < nl, nl, part);
}

// ------------------------------------------------------------------ the per-cell terms
// a(y), b(y), log c(y) of one cell (regression.py:479-489) for the PG observation models; (a, b, logc) = (y, 1, 0) for Bernoulli
__device__ __forceinline__ void pg_abc(const PgObs& g, int n, long t, double y, double& a, double& b, double& logc) {
    a = y; b = 1.0; logc = 0.0;
    if (g.obs == 1) {
        const double xi = g.param ? g.param[n] : g.xi;
        b = y + xi; logc = lgamma(y + xi) - lgamma(y + 1.0) - lgamma(xi);
    } else if (g.obs == 3) {
        const double m = g.param ? g.param[n] : g.xi;
        b = m; logc = lgamma(m + 1.0) - lgamma(y + 1.0) - lgamma(m - y + 1.0);
    } else if (g.obs == 4) {
        const double* h = g.hooks + t * 3 * g.ldh + n;
        a = h[0]; b = h[g.ldh]; logc = h[2 * g.ldh];
    }
}

// one time bin's term of the log-likelihood (regression.py:491-494); one function for every kernel that forms it, so that they round alike
__device__ __forceinline__ double pg_ll_term(double logc, double a, double b, double psi) { return logc + a * psi - b * log1p(exp(psi)); }

// the Gaussian cell (regression.py:421-423): its squared residual added to ll, omega = 1/eta, kappa = y/eta; returns the residual
__device__ __forceinline__ double gauss_cell(double y, double psi, double ie, double& ll, double& omega, double& kappa) {
    const double r = y - psi;
    ll += r * r;
    omega = ie; kappa = y * ie;
    return r;
}
