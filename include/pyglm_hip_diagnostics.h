/*
 * pyglm_hip_diagnostics.h -- the entries of libpyglm_hip.so behind the chain diagnostics (pgl_diag.hip): dyadic batch means of the chain
 * state, and the conditional (Rao-Blackwell) edge probabilities of a sweep.
 *
 * A third header beside pyglm_hip.h and pyglm_hip_dispersion.h; the conventions of pyglm_hip.h hold here word for word (device pointers, the
 * current HIP device, `hip_stream` a hipStream_t passed as void*, 0 = ok, the message from pgl_last_error()); pyglm_hip.h stays the statement
 * of ABI 11 and is not changed by what is declared here.  The headers may be included together, in any order.
 */
#ifndef PYGLM_HIP_DIAGNOSTICS_H
#define PYGLM_HIP_DIAGNOSTICS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- dyadic batch means of the chain state (pyglm_amd/diagnostics.py: batch_means_host states the definition) ------------------------------ */
/* This project's own step; it replaces no reference call site.  An ENTRY is one scalar of the shard's chain state; the entries of a call are
 * the sections its `what` names, in this order:
 *   PGL_DIAG_EDGE     nloc * N       x = a[n][m] != 0 ? 1.0 : 0.0
 *   PGL_DIAG_EDGE_RB  nloc * N       x = p[n][m]                      (pgl_diag_edge_conditional)
 *   PGL_DIAG_WEIGHT   nloc * N * B   x = a[n][m] != 0 ? W[n][m * B + beta] : 0.0    (W is [nloc][N * B], the chain-state layout)
 *   PGL_DIAG_BIAS     nloc           x = b[n]
 * pgl_diag_entries(N, B, nloc, what) is their number E (-1 for a negative size or an unknown bit).  pending, mean and M2 are [levels][E]
 * doubles each, level-major (pgl_diag_bytes(E, levels) = 3 * levels * E * 8 bytes in all), zero before the first sample.  Sample k (1-based)
 * of entry i touches levels l = 0 .. min(tz(k), levels - 1), tz = trailing zero bits of k, with s_0 = x:
 *   (mean, M2)[l][i]  <- Welford step number k >> l with the value s_l / 2^l       (the step of pgl_summary_state)
 *   l <  tz(k) and l + 1 < levels:   s_{l+1} = pending[l][i] + s_l                 (the earlier half first: one IEEE addition)
 *   l == tz(k):                      pending[l][i] = s_l
 * One thread per entry; no atomics, no LDS, no cross-lane traffic: an entry's bits do not depend on nloc, the shard or the launch geometry.
 * a is required by EDGE and WEIGHT, p by EDGE_RB, W by WEIGHT, b by BIAS; what the mask does not name may be NULL and is not read.  A refused
 * argument -- levels outside 1 .. PGL_DIAG_MAX_LEVELS, k < 1, a negative size, B < 1 with WEIGHT, an unknown or empty mask, a NULL pointer of a
 * named section or of an accumulator -- returns PGL_ERR_ARG (1) and writes nothing.  E = 0 launches nothing. */
#define PGL_DIAG_MAX_LEVELS 16
#define PGL_DIAG_EDGE 1
#define PGL_DIAG_EDGE_RB 2
#define PGL_DIAG_WEIGHT 4
#define PGL_DIAG_BIAS 8
#define PGL_DIAG_ALL 15
long pgl_diag_entries(int N, int B, int nloc, unsigned int what);
size_t pgl_diag_bytes(long entries, int levels);
int pgl_diag_fold(const int* a, const double* W, const double* b, const double* p, double* pending, double* mean, double* M2, int N, int B,
                  int nloc, int levels, long long k, unsigned int what, void* hip_stream);

/* ---- the conditional edge probabilities of one sweep (diagnostics.py: edge_conditional_host) ------------------------------------------------- */
/* p[n][m] = a[n][m] != 0 ? 1.0 : 0.0, then for every proposal step kk of row n whose logodds[n][kk] is not NaN and whose perm[n][kk] lies in
 * [0, N):  p[n][perm[n][kk]] = 1 / (1 + exp(-logodds[n][kk])).  logodds and perm are the sweep's (pgl_sweep_t.logodds, .perm), a its result;
 * all four arrays are [nloc][N].  Two launches, the fill first: a row of perm that is a permutation stores to every address once.  A NULL
 * pointer or a negative size returns PGL_ERR_ARG and writes nothing; nloc * N = 0 launches nothing. */
int pgl_diag_edge_conditional(const double* logodds, const int* perm, const int* a, double* p, int nloc, int N, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
