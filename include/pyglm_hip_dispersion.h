/*
 * pyglm_hip_dispersion.h -- the entries of libpyglm_hip.so that learn the negative-binomial dispersion xi (pgl_dispersion.hip).
 *
 * A second header beside pyglm_hip.h, whose conventions hold here word for word (device pointers, the current HIP device, `hip_stream` a
 * hipStream_t passed as void*, 0 = ok, the message from pgl_last_error()); pyglm_hip.h stays the statement of ABI 11 and is not changed by
 * what is declared here.  The two headers may be included together, in either order.
 */
#ifndef PYGLM_HIP_DISPERSION_H
#define PYGLM_HIP_DISPERSION_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the sufficient statistics of xi | y, psi (pgl_dispersion.hip): the CRT augmentation of Zhou & Carin -------------------------------- */
/* This project's own step; it replaces no reference call site.  With y ~ NB(xi, sigma(psi)) and xi ~ Gamma(e0, rate f0), the table counts
 * L_t | y_t, xi = sum_{i < y_t} Bernoulli(xi / (xi + i)) make xi | L, psi ~ Gamma(e0 + sum_t L_t, rate f0 + sum_t log(1 + e^psi_t)).  For local
 * column n, psi[t] = Psi[t * ldn + n] + bias[n] (bias NULL: 0), y[t] = Y[t * ldn + n]:
 *   count of a cell   m = min(floor(y), PGL_DISPERSION_MAX_COUNT) for y >= 1, else 0 (NaN and negative values count as none)
 *   table count       l = 1[m >= 1] + sum_{i = 1 .. m - 1} 1[ u_{i-1} * (xi[n] + i) < xi[n] ]
 *   u_k               the k-th uniform of the cell's own Philox stream: purpose 4, key = seed, stream = (sweep << 32) | (neuron0 + n),
 *                     element = elem0 + t; call j yields u_{2j} from words 0, 1 and u_{2j+1} from words 2, 3.  A cell with m <= 1 draws nothing
 *   L[n] (+)= sum_t l,   S[n] (+)= sum_t softplus(psi[t]),   softplus(x) = max(x, 0) + log1p(exp(-|x|))
 * (pyglm_amd/dispersion.py: dispersion_host states the definition).  xi is [nloc] on the device.  accumulate = 0: L and S start from zero,
 * whatever they hold; 1: a further data set is added.  T = 0 is allowed and launches nothing.  A workgroup owns PGL_DISPERSION_ROWS rows of
 * time of 64 columns and leaves one partial per column in work (pgl_dispersion_work_bytes(nloc, T) bytes, 8-byte aligned); a second launch
 * adds the workgroups' partials in time order.  A cell with m > PGL_DISPERSION_COOP is finished by the 64 lanes of its wave together: a
 * trial is addressed by its index, so who evaluates it changes nothing.  No floating-point atomics: S[n] has the same bits whatever nloc,
 * neuron0 or the shard; L is exact.  Psi is only read.  A refused argument returns PGL_ERR_ARG (1) and writes nothing. */
#define PGL_PURPOSE_DISPERSION 4
#define PGL_DISPERSION_ROWS 256
#define PGL_DISPERSION_COOP 128
#define PGL_DISPERSION_MAX_COUNT 16777216
size_t pgl_dispersion_work_bytes(int nloc, int T);
int pgl_dispersion_fold(const double* Psi, long ldn, const double* bias, const double* Y, int T, int nloc, const double* xi, uint64_t seed,
                        uint64_t sweep, uint64_t neuron0, uint64_t elem0, long long* L, double* S, int accumulate, void* work, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
