/*
 * pyglm_hip_covariates.h -- the entries of libpyglm_hip.so behind the external covariates (pgl_covariates.hip; pgl_sweep_offset lives with the
 * sweep in pgl_sweep.hip): the offset o = S beta, the sufficient statistics of beta | omega, W, b, the draw of beta, and the sweep under an
 * offset.
 *
 * A fifth header beside pyglm_hip.h, pyglm_hip_dispersion.h, pyglm_hip_diagnostics.h and pyglm_hip_sbm.h; the conventions of pyglm_hip.h hold
 * here word for word (device pointers, the current HIP device, `hip_stream` a hipStream_t passed as void*, 0 = ok, the message from
 * pgl_last_error()); pyglm_hip.h stays the statement of ABI 11 and is not changed by what is declared here.  This header uses pgl_sweep_t and
 * includes pyglm_hip.h for it; the headers may be included together, in any order.
 *
 * This project's own step; it replaces no reference call site.  pyglm_amd/covariates.py states the law in NumPy: data set i carries
 * covariates S (T x K doubles, rows lds >= K apart, shared by all neurons, 1 <= K <= PGL_COVARIATE_MAX), neuron n the weights beta_n in R^K,
 * and psi = X . vec(a * W) + b + o with o[t][n] = sum_k S[t][k] beta_n[k].
 */
#ifndef PYGLM_HIP_COVARIATES_H
#define PYGLM_HIP_COVARIATES_H
#include <stddef.h>
#include <stdint.h>
#include "pyglm_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PGL_COVARIATE_MAX 32
#define PGL_COVARIATE_ROWS 256
int pgl_covariate_max(void);

/* ---- the offset (covariates.py: offset_host) ------------------------------------------------------------------------------------------------ */
/* Off[t * ldn + n] = sum_{k = 0 .. K-1} S[t * lds + k] * Beta[k * ldn + n] for t < T, n < nloc: the sum starts from 0.0, runs over k in
 * ascending order, and every term is a rounded product followed by a rounded sum (no fused multiply-add), so the result equals the NumPy
 * loop bit for bit.  Beta is [K][ldn] (k-major, like the activation's weights).  A workgroup owns 64 rows of time and 64 columns; its slice of
 * Beta and its rows of S go to LDS once.  Columns nloc .. ldn - 1 of Off are not written.  T = 0 launches nothing. */
int pgl_covariate_offset(const double* S, long lds, const double* Beta, double* Off, long ldn, int T, int nloc, int K, void* hip_stream);

/* Psi[t * ldpsi + n] += Off[t * ldo + n], and Kappa[t * ldk + n] -= Omega[t * ldo2 + n] * Off[t * ldo + n] (a rounded product, then a rounded
 * difference), for t < T, n < nloc: the two elementwise steps a sweep under an offset adds (pgl_sweep_offset), and what a read-out of the
 * chain adds to its activation. */
int pgl_covariate_add_offset(double* Psi, long ldpsi, const double* Off, long ldo, int T, int nloc, void* hip_stream);
int pgl_covariate_reduce_kappa(double* Kappa, long ldk, const double* Omega, long ldo2, const double* Off, long ldo, int T, int nloc,
                               void* hip_stream);

/* ---- the sufficient statistics of beta_n | omega, W, b of ONE data set (covariates.py: covariate_stats_host) ----------------------------- */
/* For local column n, with psi_net[t] = Psi[t * ldn + n] + bias[n] (Psi: the activation alone -- no bias, no offset; bias NULL: 0),
 * w[t] = Omega[t * ldo + n], c[t] = Kappa[t * ldk + n] + w[t] * (Off[t * ldn + n] - psi_net[t]):
 *   Lambda[n * K (K + 1) / 2 + j (j + 1) / 2 + k] (+)= sum_t w[t] S[t][j] S[t][k]     (k <= j: the lower triangle, row by row)
 *   r[n * K + k]                                  (+)= sum_t S[t][k] c[t]
 * accumulate = 0: the sums start from zero, whatever Lambda and r hold; 1: a further data set is added.  The prior's Lambda0 and
 * Lambda0 mu0 are NOT in these sums: pgl_covariate_draw adds them.  T = 0 is allowed.
 * The (j, k) pairs are cut into 8 x 8 blocks of the triangle.  A workgroup owns PGL_COVARIATE_ROWS rows of time of 64 columns and ONE
 * block: a diagonal block (its 36 sums of Lambda and its 8 of r: 32 bytes read per cell) or a block below the diagonal (64 sums of Lambda:
 * Omega alone, 8 bytes per cell); lane = column, each of the 4 waves walks its 64 rows in time order, the block's columns of S come from LDS,
 * the waves' sums are added in wave order, and the workgroup leaves one partial per sum and column in work (pgl_covariate_work_bytes(nloc,
 * T, K) bytes, 8-byte aligned).  A second launch adds the workgroups' partials in time order.  No floating-point atomics: a column's sums
 * have the same bits whatever nloc, neuron0 or the shard.  K <= 8 is one diagonal block: every cell is read once. */
size_t pgl_covariate_work_bytes(int nloc, int T, int K);
int pgl_covariate_fold(const double* Psi, long ldn, const double* bias, const double* Omega, long ldo, const double* Kappa, long ldk,
                       const double* Off, const double* S, long lds, int T, int nloc, int K, double* Lambda, double* r, int accumulate, void* work,
                       void* hip_stream);

/* ---- the draw (covariates.py: covariate_draw_host) ------------------------------------------------------------------------------------------ */
/* Per neuron n < nloc: A = Lambda0 + Lambda[n] (Lambda0: [K][K] symmetric, its lower triangle is read), A = L L', y = L^-1 (h0 + r[n]),
 * Beta_out[n * K + .] = L^-T (y + z[n * K + .]).  One wavefront per neuron, the system in LDS.  Where a pivot is not positive (or not a
 * number) status[n] |= 1 and Beta_out[n] is left as it is; a status that is already non-zero stays (sticky).  That cannot happen with a
 * positive-definite Lambda0: the flag is there for a user's bad prior. */
int pgl_covariate_draw(const double* Lambda, const double* r, const double* Lambda0, const double* h0, const double* z, double* Beta_out,
                       int* status, int nloc, int K, void* hip_stream);

/* ---- the sweep under an offset ---------------------------------------------------------------------------------------------------------------- */
/* pgl_sweep (pyglm_hip.h) with one device pointer per data set in the HOST array offsets[ndatasets], each [T][ldn] doubles (ldn of
 * pgl_sweep_dims); NULL, or a NULL entry, means no offset.  pgl_sweep is this call with offsets = NULL.  With an offset two elementwise
 * launches are added per data set: Psi += Off between the activation and the Polya-gamma pass -- omega is drawn, and ll (Gaussian: the sum
 * of squared residuals) taken, at psi including the offset -- and Kappa -= Omega * Off behind that pass, and behind the omega_override
 * copy where there is one.  Without an offset exactly the launches of pgl_sweep are queued. */
int pgl_sweep_offset(const pgl_sweep_t* s, const double* const* offsets, uint64_t seed, uint64_t sweep, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
