// Chain diagnostics for gfx950: dyadic batch means of the chain state, folded once per collected sample, and the conditional (Rao-Blackwell)
// edge probabilities of a sweep (pyglm_amd/diagnostics.py: batch_means_host and edge_conditional_host state the definitions; include/
// pyglm_hip_diagnostics.h the calls).  DESIGN.md section 17.
//
//   diag_fold_kernel              one thread per entry of the sections `what` names (edge | edge_rb | weight | bias), 256 per workgroup.  Sample
//                                 k touches levels 0 .. min(tz(k), levels - 1) -- a number every thread shares, so the loops over levels are
//                                 uniform.  The accumulators are [level][entry]: at every level a wave reads and writes 512 contiguous bytes
//                                 of each plane.  All loads of a thread are issued before the first dependent addition (the carry chain s_l =
//                                 pending_{l-1} + s_{l-1} would otherwise put one HBM latency per level in series), then the Welford steps run
//                                 in registers, then the stores.  HBM-bound: 40 bytes per touched level and entry (pending read or written, mean
//                                 and M2 read and written) plus the entry's value.
//   diag_edge_fill_kernel         p = a != 0 ? 1 : 0
//   diag_edge_conditional_kernel  one thread per (n, kk): p[n][perm[n][kk]] = sigma(logodds[n][kk]) where that is a number and perm in range
// No atomics, no LDS, no cross-lane traffic: an entry's bits cannot depend on nloc, the shard or the launch geometry.
#include "pgl_common.h"
#include "../../include/pyglm_hip_diagnostics.h"

namespace {

struct DiagFold {
    const int* a; const double* W; const double* b; const double* p;
    double* pending; double* mean; double* M2;
    long E, o_rb, o_w, o_b;      // entries; where the edge_rb, weight and bias sections begin (a section not in `what` is empty)
    int B, div32;                // div32: the weight section's index fits 32 bits (its edge comes by a 32-bit division)
    int nlev, last;              // levels touched: 0 .. nlev - 1; last: level nlev - 1 is tz(k) and keeps its sum as pending
    long long k;
};

// the value of entry i: its section's read of the chain state
__device__ __forceinline__ double diag_value(const DiagFold& f, long i) {
    if (i < f.o_rb) return f.a[i] != 0 ? 1.0 : 0.0;
    if (i < f.o_w) return f.p[i - f.o_rb];
    if (i < f.o_b) {
        const long j = i - f.o_w;
        const long e = f.div32 ? (long)((unsigned)j / (unsigned)f.B) : j / f.B;
        const double w = f.W[j];
        return f.a[e] != 0 ? w : 0.0;
    }
    return f.b[i - f.o_b];
}

__global__ __launch_bounds__(256) void diag_fold_kernel(DiagFold f) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= f.E) return;
    const int nlev = f.nlev;
    double pe[PGL_DIAG_MAX_LEVELS], me[PGL_DIAG_MAX_LEVELS], m2[PGL_DIAG_MAX_LEVELS];
#pragma unroll
    for (int l = 0; l < PGL_DIAG_MAX_LEVELS; ++l) {
        if (l < nlev) {
            const long at = (long)l * f.E + i;
            me[l] = f.mean[at];
            m2[l] = f.M2[at];
            pe[l] = l + 1 < nlev ? f.pending[at] : 0.0;       // (the levels below the last carry: they read their first half)
        }
    }
    double s = diag_value(f, i);      // (behind the planes' loads: the section's select waits for its operands, and those loads are then in flight)
#pragma unroll
    for (int l = 0; l < PGL_DIAG_MAX_LEVELS; ++l) {
        if (l < nlev) {
            const long at = (long)l * f.E + i;
            // Welford step k >> l of (mean, M2) with the batch mean s / 2^l (pgl_summary.hip: welford)
            const double v = s * (1.0 / (double)(1 << l)), kd = (double)(f.k >> l);
            const double d = v - me[l], m1 = me[l] + d / kd;
            f.mean[at] = m1;
            f.M2[at] = m2[l] + d * (v - m1);
            if (l + 1 < nlev) s = pe[l] + s;                  // the earlier half first
            else if (f.last) f.pending[at] = s;
        }
    }
}

__global__ __launch_bounds__(256) void diag_edge_fill_kernel(const int* __restrict__ a, double* __restrict__ p, long total) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i < total) p[i] = a[i] != 0 ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void diag_edge_conditional_kernel(const double* __restrict__ logodds, const int* __restrict__ perm,
                                                                    double* __restrict__ p, long total, int N) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const double lo = logodds[i];
    const int m = perm[i];
    if (lo == lo && m >= 0 && m < N) p[(i / N) * N + m] = 1.0 / (1.0 + exp(-lo));
}

constexpr unsigned DIAG_KNOWN = PGL_DIAG_EDGE | PGL_DIAG_EDGE_RB | PGL_DIAG_WEIGHT | PGL_DIAG_BIAS;
static_assert(DIAG_KNOWN == PGL_DIAG_ALL, "PGL_DIAG_ALL names every section");

inline bool diag_blocks_ok(long total) { return (total + 255) / 256 <= 2147483647L; }

}  // namespace

extern "C" long pgl_diag_entries(int N, int B, int nloc, unsigned int what) {
    if (N < 0 || B < 0 || nloc < 0 || (what & ~DIAG_KNOWN)) return -1;
    const long e = (long)nloc * N;
    long total = 0;
    if (what & PGL_DIAG_EDGE) total += e;
    if (what & PGL_DIAG_EDGE_RB) total += e;
    if (what & PGL_DIAG_WEIGHT) total += e * B;
    if (what & PGL_DIAG_BIAS) total += nloc;
    return total;
}

extern "C" size_t pgl_diag_bytes(long entries, int levels) {
    if (entries < 0 || levels < 1 || levels > PGL_DIAG_MAX_LEVELS) return 0;
    return (size_t)3 * (size_t)levels * (size_t)entries * sizeof(double);
}

extern "C" int pgl_diag_fold(const int* a, const double* W, const double* b, const double* p, double* pending, double* mean, double* M2, int N,
                             int B, int nloc, int levels, long long k, unsigned int what, void* hip_stream) {
    PGL_CHECK_ARG(levels >= 1 && levels <= PGL_DIAG_MAX_LEVELS && k >= 1);
    PGL_CHECK_ARG(N >= 0 && B >= 0 && nloc >= 0 && what != 0 && (what & ~DIAG_KNOWN) == 0);
    PGL_CHECK_ARG(!(what & PGL_DIAG_WEIGHT) || B >= 1);
    PGL_CHECK_ARG(pending && mean && M2);
    PGL_CHECK_ARG(!(what & (PGL_DIAG_EDGE | PGL_DIAG_WEIGHT)) || a);
    PGL_CHECK_ARG(!(what & PGL_DIAG_EDGE_RB) || p);
    PGL_CHECK_ARG(!(what & PGL_DIAG_WEIGHT) || W);
    PGL_CHECK_ARG(!(what & PGL_DIAG_BIAS) || b);
    const long e = (long)nloc * N;
    DiagFold f;
    f.a = a; f.W = W; f.b = b; f.p = p; f.pending = pending; f.mean = mean; f.M2 = M2;
    f.o_rb = (what & PGL_DIAG_EDGE) ? e : 0;
    f.o_w = f.o_rb + ((what & PGL_DIAG_EDGE_RB) ? e : 0);
    const long nw = (what & PGL_DIAG_WEIGHT) ? e * B : 0;
    f.o_b = f.o_w + nw;
    f.E = f.o_b + ((what & PGL_DIAG_BIAS) ? nloc : 0);
    PGL_CHECK_ARG(diag_blocks_ok(f.E));
    if (f.E == 0) return PGL_OK;
    f.B = B > 0 ? B : 1;
    f.div32 = nw <= 2147483647L;
    const int tz = __builtin_ctzll((unsigned long long)k);
    f.nlev = (tz < levels - 1 ? tz : levels - 1) + 1;
    f.last = f.nlev - 1 == tz;
    f.k = k;
    hipLaunchKernelGGL(diag_fold_kernel, dim3((unsigned)((f.E + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(hip_stream), f);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}

extern "C" int pgl_diag_edge_conditional(const double* logodds, const int* perm, const int* a, double* p, int nloc, int N, void* hip_stream) {
    PGL_CHECK_ARG(nloc >= 0 && N >= 0 && logodds && perm && a && p);
    const long total = (long)nloc * N;
    PGL_CHECK_ARG(diag_blocks_ok(total));
    if (total == 0) return PGL_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const dim3 grid((unsigned)((total + 255) / 256));
    hipLaunchKernelGGL(diag_edge_fill_kernel, grid, dim3(256), 0, st, a, p, total);
    PGL_CHECK_LAUNCH();
    hipLaunchKernelGGL(diag_edge_conditional_kernel, grid, dim3(256), 0, st, logodds, perm, p, total, N);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}
