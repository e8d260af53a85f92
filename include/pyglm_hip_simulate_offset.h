/*
 * pyglm_hip_simulate_offset.h -- the entries of libpyglm_hip.so behind free-running simulation of a model with external covariates or
 * latent common input: pgl_simulate with a time-parallel offset (pgl_generate.hip), the offset itself and the latents' prior paths
 * (pgl_simulate_offset.hip).
 *
 * An eighth header beside pyglm_hip.h and the six others; the conventions of pyglm_hip.h hold here word for word (device pointers, the
 * current HIP device, `hip_stream` a hipStream_t passed as void*, 0 = ok, the message from pgl_last_error()); pyglm_hip.h stays the
 * statement of ABI 11 and is not changed by what is declared here.
 *
 * This project's own step; it replaces no reference call site.  pyglm_amd/simulate.py states the law in NumPy (simulate_host(offset=),
 * simulate_offset_host, latent_prior_host):  psi_r[t][n] = ((Wm[n] . x_r[t]) + bias[n]) + o_r[t][n],  o_r = offset_host([S_obs | X_r], beta).
 */
#ifndef PYGLM_HIP_SIMULATE_OFFSET_H
#define PYGLM_HIP_SIMULATE_OFFSET_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PGL_PURPOSE_SIM_LATENT 7
#define PGL_SIM_LATENT_MAX 8

/* ---- pgl_simulate under an offset ---------------------------------------------------------------------------------------------------------- */
/* pgl_simulate (pyglm_hip.h) word for word, and the activation of replicate r (0 <= r < R) at bin t0 + k (0 <= k < Tc) of neuron n is
 *   psi = ((Wm[n, :] . x) + bias[n]) + Off[r * ldo_r + k * ldo_t + n]
 * -- one rounded sum, added last.  ldo_t >= N; ldo_r = 0: one offset shared by the replicates, else ldo_r >= (Tc - 1) * ldo_t + N.  Only
 * columns n < N of a row are read, and a workgroup reads the columns of its own neurons alone; Off is not written.  Off = NULL (ldo_t and
 * ldo_r are then ignored) queues exactly the launch of pgl_simulate. */
int pgl_simulate_offset(const double* Wm, const double* bias, const double* basis, int N, int B, int L, const int* kind, const double* par, int R,
                        long rep0, unsigned long long seed, double* ring, double* Y, long ldr, double* sum, double* sumsq, long t0, int Tc,
                        void* work, int* status, const double* Off, long ldo_t, long ldo_r, void* hip_stream);

/* ---- the offset of a chunk (simulate.py: simulate_offset_host) ----------------------------------------------------------------------------- */
/* Off[r * ldo_r + k * ldo_t + n] = sum_j S[k * lds + j] * Beta[j * ldn + n]  (j < K_obs, ascending)
 *                                 + sum_q X[r * ldx_r + k * Q + q] * Beta[(K_obs + q) * ldn + n]  (q < Q, ascending)
 * for r < R, k < Tc, n < N: from 0.0, a rounded product and a rounded sum per term (covariates.offset_host of [S_obs | X_r]; the prefix
 * over the observed columns is formed once per cell and continued per replicate).  Beta: the k-major weights [K_obs + Q][ldn].  K_obs >= 0,
 * 0 <= Q <= PGL_SIM_LATENT_MAX, 1 <= K_obs + Q <= 32; Q = 0 requires R = 1 and equals pgl_covariate_offset bit for bit.  ldx_r = 0: the
 * latents are shared (R = 1 is then required: a shared X makes a shared offset).  ldo_t >= N, lds >= K_obs; columns >= N are not written.
 * One workgroup owns 64 rows of 64 columns for every replicate. */
int pgl_simulate_offset_build(const double* S, long lds, const double* X, long ldx_r, const double* Beta, long ldn, double* Off, long ldo_t,
                              long ldo_r, int Tc, int N, int K_obs, int Q, int R, void* hip_stream);

/* ---- the latents' prior paths of a chunk (simulate.py: latent_prior_host) ------------------------------------------------------------------ */
/* X[r * ldx_r + k * Q + q] for r < R, k < Tc, q < Q: the stationary AR(1) path of factor q of replicate rep0 + r at bins t0 .. t0 + Tc - 1.
 *   z[r][k][q]  = z_override[(r * Tc + k) * Q + q] where z_override is given (tests: the recurrence apart from the stream); NULL: the
 *                 pgl_norm of call q of the Philox stream (purpose PGL_PURPOSE_SIM_LATENT, key = seed, stream = rep0 + r, element = t0 +
 *                 k; the element's low 32 bits enter the counter), both uniforms of the call
 *   x[k][q]     = z[k][q]                                                at k = 0 where has_carry = 0: the stationary start
 *               = fl(fl(phi[q] * x[k - 1][q]) + fl(s[q] * z[k][q]))      otherwise; x[-1] = carry[r * Q + q] (has_carry = 1)
 * uncontracted.  phi, s: Q doubles each on the HOST, 0 <= phi[q] < 1, 0 < s[q] <= 1 (the caller forms s = sqrt(1 - phi^2)).  carry [R][Q] is
 * read where has_carry = 1 and always receives x[Tc - 1].  1 <= Q <= PGL_SIM_LATENT_MAX, R >= 1, Tc >= 1, rep0 >= 0, ldx_r >= Tc * Q.
 * One workgroup per replicate: the normals of a tile of bins are drawn one thread each into LDS, one lane per factor then walks the tile in
 * time order.  A plain launch, no atomics; the bits of X do not depend on R or on how the bins are cut into calls. */
int pgl_latent_prior_paths(double* X, long ldx_r, int R, long rep0, uint64_t t0, int Tc, int Q, const double* phi, const double* s, double* carry,
                           int has_carry, const double* z_override, uint64_t seed, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
