/*
 * pyglm_hip_latents.h -- the entries of libpyglm_hip.so behind the latent common input (pgl_latents.hip): the sufficient statistics of
 * x_t | omega, W, b, beta for every time bin, and the draw of x_t.
 *
 * A sixth header beside pyglm_hip.h, pyglm_hip_dispersion.h, pyglm_hip_diagnostics.h, pyglm_hip_sbm.h and pyglm_hip_covariates.h; the
 * conventions of pyglm_hip.h hold here word for word (device pointers, the current HIP device, `hip_stream` a hipStream_t passed as void*,
 * 0 = ok, the message from pgl_last_error()); pyglm_hip.h stays the statement of ABI 11 and is not changed by what is declared here.
 *
 * This project's own step; it replaces no reference call site.  pyglm_amd/latents.py states the law in NumPy: a data set's S (T x K
 * doubles, rows lds >= K apart) is [S_obs | X], the Q latent columns starting at col0, 1 <= Q <= PGL_LATENT_MAX; neuron n's loadings are
 * C_n[q] = Beta[(col0 + q) * ldb + n] of the k-major covariate weights.  The loadings themselves are drawn by pgl_covariate_fold /
 * pgl_covariate_draw unchanged.
 */
#ifndef PYGLM_HIP_LATENTS_H
#define PYGLM_HIP_LATENTS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PGL_LATENT_MAX 8
#define PGL_LATENT_LDS_COLS 1024
#define PGL_PURPOSE_LATENT 6
int pgl_latent_max(void);

/* ---- the sufficient statistics of x_t of ONE data set (latents.py: latent_stats_host) -------------------------------------------------------- */
/* For time bin t < T, with psi_net[n] = Psi[t * ldn + n] + bias[n] (Psi: the activation alone -- no bias, no offset; bias NULL: 0),
 * w[n] = Omega[t * ldo + n], o[n] = sum_q S[t * lds + col0 + q] * C_n[q] (q ascending) and c[n] = Kappa[t * ldk + n] + w[n] * (o[n] -
 * psi_net[n]):
 *   Lambda[t * Q (Q + 1) / 2 + j (j + 1) / 2 + k] = sum_n w[n] C_n[j] C_n[k]          (k <= j: the lower triangle, row by row)
 *   r[t * Q + q]                                  = sum_n C_n[q] c[n]
 * over n < nloc.  The prior's identity is NOT in Lambda: pgl_latent_draw adds it.  One pass over Psi, Omega and Kappa: 24 bytes per cell.
 * One wavefront owns a time bin: lane l adds columns l, l + 64, l + 128, ... in ascending order, then the 64 lanes' sums join in a fixed
 * tree of __shfl_xor steps (distances 32, 16, 8, 4, 2, 1; the first steps halve the set of sums a lane carries, so the tree moves 63
 * values per bin at Q = 8, not 44 x 6).  No floating-point atomics: a bin's sums have the same bits whatever T, the bins that share its
 * workgroup and the launch geometry -- they depend on nloc alone.  Columns nloc and above are not read and add nothing.  A workgroup
 * stages the loadings and the bias in LDS once ((Q + 1) * 8 bytes per column) where nloc <= PGL_LATENT_LDS_COLS; above that every lane
 * reads its columns' loadings from Beta through the caches -- the same sums in the same order.  T = 0 launches nothing. */
int pgl_latent_fold(const double* Psi, long ldn, const double* bias, const double* Omega, long ldo, const double* Kappa, long ldk, const double* S,
                    long lds, int col0, const double* Beta, long ldb, int T, int nloc, int Q, double* Lambda, double* r, void* hip_stream);

/* ---- the draw (latents.py: latent_draw_host) ---------------------------------------------------------------------------------------------------- */
/* Per time bin t < T, one thread each: A = I + Lambda[t], A = L L', y = L^-1 r[t], S[t * lds + col0 + q] = (L^-T (y + z))[q] for q < Q --
 * and nothing else of S is written.  z = z_override[t * Q + q] where z_override is given (tests: the linear algebra apart from the
 * stream); NULL: z[q] is the q-th pgl_norm of the Philox stream (purpose PGL_PURPOSE_LATENT, key = seed, stream = sweep, element = elem0 +
 * t), one call of the generator per normal.  Where a pivot is not positive (or not a number) *status |= 1 and the bin's latents are left
 * as they are; a status that is already non-zero stays (sticky).  I + a positive semi-definite Lambda cannot produce that on finite input. */
int pgl_latent_draw(const double* Lambda, const double* r, const double* z_override, uint64_t seed, uint64_t sweep, uint64_t elem0, double* S,
                    long lds, int col0, int* status, int T, int Q, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
