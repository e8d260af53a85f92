// The observation models' per-cell terms, shared by the kernels that walk Psi (pgl_elementwise.hip: PG draws + log-likelihood;
// pgl_summary.hip: the posterior accumulators): one definition of a(y), b(y), log c(y) and of the log-likelihood term, one block shape,
// so that every pass rounds alike and adds in the same order.
#pragma once
#include "pgl_common.h"

// Each block covers PGLL_ROWS time bins of one 64-neuron column group and leaves one partial per neuron; a second pass
// (pgl_k_colsum_partials) adds the partials in a fixed order.
constexpr int PGLL_ROWS = 64;

struct PgLlArgs {
    double* Psi; long ldpsi;            // in: X.w   out: psi = X.w + bias   [T][ldpsi]
    const double* bias;                 // [nloc]
    const double* Y; long ldy;          // spikes/counts of the local neurons: Y[t*ldy + n]
    double* Omega; long ldo;            // out [T][ldo]   (may be null: log-likelihood only)
    double* Kappa; long ldk;            // out [T][ldk]   (may be null)
    double* llpart;                     // [nblk_t][nloc]
    int T, nloc;
    int obs;                            // 0 Bernoulli (a=y,b=1,c=1)  1 negative binomial (a=y, b=y+xi, c=C(y+xi-1,y))
                                        // 2 Gaussian (regression.py:380-446): omega = 1/eta, kappa = y/eta, "ll" = sum of squared residuals
                                        // 3 binomial (a=y, b=n, c=C(n,y))  4 hooks: a, b, log c read from `hooks`
    double xi;                          // xi (obs 1) or n (obs 3) where param is null
    const double* inv_eta;              // [nloc] 1/eta per neuron (obs == 2 only)
    uint64_t seed, sweep, neuron0, elem0;
    const double* param;                // optional [nloc]: xi (obs 1) or n (obs 3) per neuron
    const double* hooks; long ldh;      // obs 4: [T][3 ldh] = a | b | log c of the local neurons
};

// a(y), b(y), log c(y) of one cell (regression.py:479-489) for the PG observation models; (a, b, logc) = (y, 1, 0) for Bernoulli
__device__ __forceinline__ void pg_abc(const PgLlArgs& g, int n, long t, double y, double& a, double& b, double& logc) {
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
