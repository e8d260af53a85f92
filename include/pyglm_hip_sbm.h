/*
 * pyglm_hip_sbm.h -- the entries of libpyglm_hip.so behind the learned network priors (pgl_sbm.hip): the scan over the block assignments of a
 * stochastic block model, the block-to-block edge counts, and the label-invariant fold of a sampled partition.
 *
 * A fourth header beside pyglm_hip.h, pyglm_hip_dispersion.h and pyglm_hip_diagnostics.h; the conventions of pyglm_hip.h hold here word for
 * word (device pointers, the current HIP device, `hip_stream` a hipStream_t passed as void*, 0 = ok, the message from pgl_last_error());
 * pyglm_hip.h stays the statement of ABI 11 and is not changed by what is declared here.  The headers may be included together, in any order.
 */
#ifndef PYGLM_HIP_SBM_H
#define PYGLM_HIP_SBM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the scan over the block assignments (pyglm_amd/sbm.py: sbm_scan_host states the definition) ------------------------------------------ */
/* This project's own step; it replaces no reference call site (the reference leaves its block models as a TODO).  A is the gathered
 * adjacency, one byte per cell (non-zero = edge), row n the postsynaptic neuron, rows lda >= N bytes apart; z[n] in [0, K) the block of
 * neuron n; LP[k][l] = log P[k][l], LQ[k][l] = log(1 - P[k][l]) and logpi[k] finite doubles formed on the host (the device evaluates no
 * logarithm).  For n = 0 .. N - 1 in order, with the z of the moment and over the partners m != n:
 *   cnt[l] = #{m : z_m = l}    cin[l] = #{m : A[n][m], z_m = l}    cout[l] = #{m : A[m][n], z_m = l}            (exact integers)
 *   s = logpi[k];  for l = 0 .. K-1:  s += cin[l] * LP[k][l];  s += (cnt[l] - cin[l]) * LQ[k][l]
 *                  for l = 0 .. K-1:  s += cout[l] * LP[l][k]; s += (cnt[l] - cout[l]) * LQ[l][k];   lp[k] = s
 *   every product rounded, every sum rounded, in this order: no fused multiply-add
 *   e_k = exp(lp[k] - max lp);  c_k = e_0 + .. + e_k from the left;  u = the first uniform (words 0 and 1, ((x >> 11) + 0.5) / 2^53) of
 *   Philox4x32-10 call 0 with key = seed, counter = (PGL_PURPOSE_SBM << 24, n, sweep lo, sweep hi);  z_n = the smallest k with
 *   u * c_{K-1} < c_k, else K - 1.
 * lp_out (NULL, or [N][K] doubles) receives the lp every neuron saw at its turn.  work holds pgl_sbm_work_bytes(N) bytes: the transpose of A
 * (0 / 1 bytes, rows N apart: column n of A is then a contiguous read), written first, and behind it the word the pre-pass over z reports in.
 * The scan is ONE workgroup of 1024 threads; the entry waits for the stream once, to read that word.  N * K = 0 launches nothing.  Refused:
 * K outside 1 .. PGL_SBM_MAX_BLOCKS, N outside 0 .. PGL_SBM_MAX_N, lda < N, a NULL A, z, LP, LQ, logpi or work, and a z entry outside
 * [0, K) on entry (found by the pre-pass) -- PGL_ERR_ARG (1); z, lp_out and the transpose are not written then. */
#define PGL_SBM_MAX_BLOCKS 32
#define PGL_SBM_MAX_N 32768
#define PGL_PURPOSE_SBM 5
size_t pgl_sbm_work_bytes(int N);
int pgl_sbm_scan(const uint8_t* A, int* z, const double* LP, const double* LQ, const double* logpi, double* lp_out, void* work, int N, int K,
                 long lda, unsigned long long seed, unsigned long long sweep, void* hip_stream);

/* ---- block-to-block edge counts (sbm.py: block_counts_host) -------------------------------------------------------------------------------- */
/* M[k][l] = #{(n, m), n != m : A[n][m], z_n = k, z_m = l};  nk[k] = #{n : z_n = k};  diag[0] = #{n : A[n][n]}.  Parallel over the N^2 cells:
 * integer histograms per workgroup in LDS, then integer atomics to global memory -- exact whatever the launch geometry.  The three outputs
 * are overwritten.  A neuron whose z lies outside [0, K) is counted nowhere (nor are its cells off the diagonal).  Refused: K outside
 * 1 .. PGL_SBM_MAX_BLOCKS, N outside 0 .. PGL_SBM_MAX_N, lda < N, a NULL pointer. */
int pgl_sbm_block_counts(const uint8_t* A, const int* z, long long* M, long long* nk, long long* diag, int N, int K, long lda, void* hip_stream);

/* ---- the fold of one sampled partition (sbm.py: BlockStructure) ------------------------------------------------------------------------------ */
/* One thread per cell:  coassign[n][m] += (z_n == z_m);  rho_sum[n][m] += (n == m ? rho_self : P[z_n][z_m]) -- the prior as it was pushed;
 * one IEEE addition per cell and sample, so the bits do not depend on the launch geometry.  A cell with a z outside [0, K) is left as it is.
 * Refused: K outside 1 .. PGL_SBM_MAX_BLOCKS, N outside 0 .. PGL_SBM_MAX_N, a NULL pointer. */
int pgl_sbm_fold(const int* z, const double* P, double rho_self, uint32_t* coassign, double* rho_sum, int N, int K, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
