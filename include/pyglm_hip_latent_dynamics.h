/*
 * pyglm_hip_latent_dynamics.h -- the entries of libpyglm_hip.so behind the temporal prior of the latent common input
 * (pgl_latent_dynamics.hip): an exact joint draw of a data set's X from the block-tridiagonal Gaussian an AR(1) prior makes of its T bins.
 *
 * A seventh header beside pyglm_hip.h and the five others; the conventions of pyglm_hip.h hold here word for word (device pointers, the
 * current HIP device, `hip_stream` a hipStream_t passed as void*, 0 = ok, the message from pgl_last_error()); pyglm_hip.h stays the
 * statement of ABI 11 and pyglm_hip_latents.h stays as it is: pgl_latent_fold produces Lambda and r for this draw unchanged.
 *
 * This project's own step; it replaces no reference call site.  pyglm_amd/latents.py states the law in NumPy (ar_prior_blocks,
 * ar_precision_dense, latent_ar_draw_host): per factor q, x_0 ~ N(0, 1), x_t = phi_q x_{t-1} + sqrt(1 - phi_q^2) eps_t.
 */
#ifndef PYGLM_HIP_LATENT_DYNAMICS_H
#define PYGLM_HIP_LATENT_DYNAMICS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the default segment length of pgl_latent_ar_draw (seg = 0) */
int pgl_latent_ar_seg(void);

/* bytes of device scratch one pgl_latent_ar_draw(T, Q, seg) needs, all levels together (seg = 0: the default); 0 on arguments the draw
 * refuses */
size_t pgl_latent_ar_scratch(int T, int Q, int seg);

/* ---- the draw (latents.py: latent_ar_draw_host states the law, not the elimination order) --------------------------------------------- */
/* X ~ N(J^-1 h, J^-1) of ONE data set, J the T Q x T Q block-tridiagonal matrix with
 *   J[t][t]     = Lambda[t] (the lower triangle pgl_latent_fold writes, Q (Q + 1) / 2 per bin) + diag(d_t),
 *                 d_t[q] = (1 + phi_q^2) / s_q, 1 / s_q at t = 0 and t = T - 1, exactly 1 where T = 1;  s_q = 1 - phi_q^2
 *   J[t + 1][t] = -diag(phi_q / s_q)
 *   h[t]        = r[t]
 * and phi (Q doubles on the HOST, 0 <= phi_q < 1) the AR(1) coefficients.  S[t * lds + col0 + q] = X[t][q] for q < Q and nothing else of
 * S is written.  z = z_override[t * Q + q] where given; NULL: the Philox stream of pgl_latent_draw (purpose PGL_PURPOSE_LATENT, key = seed,
 * stream = sweep, element = elem0 + t, call q), used wherever bin t is drawn.
 *
 * Segments and separators, recursively: a chain of n blocks is cut into runs of seg - 1 interior bins with one separator bin between
 * two runs (bins seg - 1, 2 seg - 1, ...); every run is eliminated by its own group of lanes in one launch, which leaves the separators'
 * own block-tridiagonal chain of floor(n / seg) blocks -- a separator's diagonal block and right-hand side are the sum of a partial from
 * the run on its left and one from the run on its right, added in that order (no floating-point atomics) --; that chain is reduced
 * likewise until it has fewer than 2 seg blocks, which one group factors serially; on the way back every run is drawn given its two
 * separators.  2 levels + 1 launches, queued on the stream with no host synchronisation; the level structure follows from T and seg alone,
 * and so do the bits of X together with Q, phi and the inputs -- not the grid, the CU count or other data sets.  seg >= T: one serial chain.
 *
 * A pivot that is not positive (or not a number) at any level sets *status |= 1 (sticky), and then S is NOT written at all: the draw
 * happens in scratch and the last launch copies into S only where the status word is still 0.  T = 0 launches nothing.  scratch: at least
 * pgl_latent_ar_scratch(T, Q, seg) bytes, 8-byte aligned, owned by the call until the stream has run it. */
int pgl_latent_ar_draw(const double* Lambda, const double* r, const double* phi, const double* z_override, uint64_t seed, uint64_t sweep,
                       uint64_t elem0, double* S, long lds, int col0, int* status, int T, int Q, int seg, void* scratch, size_t scratch_bytes,
                       void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
