// The sufficient statistics of the negative-binomial dispersion's conditional (Zhou & Carin's CRT augmentation): per neuron
//   L = sum_t l_t,  l_t = sum_{i < y_t} Bernoulli(xi / (xi + i)),      S = sum_t log(1 + e^psi_t),
// so that xi | L, psi ~ Gamma(e0 + L, rate f0 + S) (pyglm_amd/dispersion.py: dispersion_host states the definition; include/
// pyglm_hip_dispersion.h the call).  DESIGN.md section 16.
//
//   disp_fold_kernel    one workgroup = PGL_DISPERSION_ROWS rows of time of 64 columns; lane = column, so a wave reads 512 contiguous bytes of
//                       Psi and of Y per row.  Each of the 4 waves walks its DISP_WAVE_ROWS rows in time order, eight rows' loads in flight:
//                       the eight softplus terms come branch-free and join the lane's sum in row order; then the lanes whose rows hold a
//                       count of 2 or more take those cells one at a time (the loop runs as often as the busiest lane has such cells): a
//                       cell of up to PGL_DISPERSION_COOP trials is walked by its lane, two trials per Philox call; a larger one is left
//                       for the wave, which finishes such cells one after the other with all 64 lanes -- calls lane, lane + 64, ... of
//                       the cell's stream, then an integer butterfly.  A trial is addressed by its index, so the count is the
//                       definition's whoever evaluates it.  Behind the barrier wave 0 adds the four waves' sums in wave order and writes
//                       the workgroup's partial to `work`: [blocks][nloc] doubles, then [blocks][nloc] 64-bit integers.
//   disp_finish_kernel  one thread per column adds the workgroups' partials in time order and alone writes S and L.
// No floating-point atomics: every floating sum is formed by one thread in an order fixed by T, so a column's S has the same bits whatever
// nloc, neuron0 or the shard (the property pgl_summary_colsum documents); L adds integers only.
#include "pgl_common.h"
#include "pgl_rng.h"
#include "../../include/pyglm_hip_dispersion.h"

namespace {

constexpr int DISP_WAVES = 4;
constexpr int DISP_WAVE_ROWS = PGL_DISPERSION_ROWS / DISP_WAVES;     // rows of time one wave walks
constexpr int DISP_BATCH = 8;                                        // rows whose loads are in flight together
static_assert(PGL_DISPERSION_ROWS % DISP_WAVES == 0 && DISP_WAVE_ROWS % DISP_BATCH == 0, "a wave walks whole batches");
static_assert(PGL_DISPERSION_COOP % 64 == 0, "the cooperative threshold is a multiple of the wave");
static_assert(PGL_DISPERSION_MAX_COUNT <= (1 << 24), "call j of a cell's stream sits in 24 bits of counter word 0");

struct DispArgs {
    const double* Psi; long ldn; const double* bias; const double* Y;
    int T, nloc; const double* xi;
    uint32_t k0, k1, s1;                              // Philox key; counter word 3 (the sweep)
    uint64_t neuron0, elem0;
};

// count of a cell: floor(y) for y >= 1, capped; NaN and negative values compare false
__device__ __forceinline__ int disp_count(double y) {
    return y >= 1.0 ? (y >= (double)PGL_DISPERSION_MAX_COUNT ? PGL_DISPERSION_MAX_COUNT : (int)y) : 0;
}

// trials 2j + 1 and 2j + 2 of a cell of count m (call j of its stream: u_{2j}, u_{2j+1}) -> how many of them open a table
__device__ __forceinline__ int disp_call(const DispArgs& a, uint32_t elem, uint32_t s0, int j, int m, double xi) {
#pragma clang fp contract(off)                        // (xi + i) is rounded, then the product: what `u * (xi + i) < xi` says on the host
    uint32_t o0, o1, o2, o3;
    pgl_philox4x32_10((uint32_t)j | ((uint32_t)PGL_PURPOSE_DISPERSION << 24), elem, s0, a.s1, a.k0, a.k1, o0, o1, o2, o3);
    const int i = 2 * j + 1;
    const double u0 = pgl_u64_to_unit((uint64_t)o0 | ((uint64_t)o1 << 32)), u1 = pgl_u64_to_unit((uint64_t)o2 | ((uint64_t)o3 << 32));
    int c = (i < m && u0 * (xi + (double)i) < xi) ? 1 : 0;
    c += (i + 1 < m && u1 * (xi + (double)(i + 1)) < xi) ? 1 : 0;
    return c;
}

__global__ __launch_bounds__(256) void disp_fold_kernel(DispArgs a, double* __restrict__ partS, long long* __restrict__ partL) {
    __shared__ double redS[DISP_WAVES][64];
    __shared__ long long redL[DISP_WAVES][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.y * 64 + lane;
    const bool own = n < a.nloc;
    const int nc = own ? n : a.nloc - 1;                               // a lane past the last column reads that column and owns nothing
    const double bn = a.bias ? a.bias[nc] : 0.0, xi = a.xi[nc];
    const uint32_t s0 = (uint32_t)(a.neuron0 + (uint64_t)nc);          // counter word 2: the global neuron
    const double* pp = a.Psi + nc;
    const double* py = a.Y + nc;
    double s = 0.0;
    long long l = 0;
    const int u0 = blockIdx.x * PGL_DISPERSION_ROWS + wave * DISP_WAVE_ROWS, u1 = min(a.T, u0 + DISP_WAVE_ROWS);
    for (int u = u0; u < u1; u += DISP_BATCH) {                        // (u0, u1 are the wave's: every lane makes the same trips)
        double q[DISP_BATCH], y[DISP_BATCH];
#pragma unroll
        for (int k = 0; k < DISP_BATCH; ++k) {
            const bool in = u + k < u1;
            q[k] = in ? pp[(long)(u + k) * a.ldn] : 0.0;
            y[k] = in ? py[(long)(u + k) * a.ldn] : 0.0;
        }
        unsigned ev = 0;
#pragma unroll
        for (int k = 0; k < DISP_BATCH; ++k) {
            const bool in = u + k < u1;
            const double x = q[k] + bn;
            const double sp = (x > 0.0 ? x : 0.0) + log1p(exp(-fabs(x)));
            s += in ? sp : 0.0;                                        // (s >= 0: adding 0.0 leaves its bits)
            const int m = own ? disp_count(y[k]) : 0;
            l += m >= 1 ? 1 : 0;
            ev |= m >= 2 ? 1u << k : 0u;
        }
        unsigned big = 0;
        while (ev) {                                                   // this lane's cells of two or more, in time order
            const int k = __ffs(ev) - 1;
            ev &= ev - 1;
            double ye = y[0];
#pragma unroll
            for (int j = 1; j < DISP_BATCH; ++j) ye = k == j ? y[j] : ye;
            const int m = disp_count(ye);
            if (m > PGL_DISPERSION_COOP) { big |= 1u << k; continue; }
            const uint32_t elem = (uint32_t)(a.elem0 + (uint64_t)(u + k));
            int c = 0;
#pragma unroll 1
            for (int j = 0; 2 * j + 1 < m; ++j) c += disp_call(a, elem, s0, j, m, xi);
            l += c;
        }
        // the large cells of the wave, one after the other, every lane on each: the ballot is the same in all 64 lanes, so they leave together
        for (unsigned long long who = __ballot(big != 0); who; who = __ballot(big != 0)) {
            const int src = __ffsll(who) - 1;
            const unsigned bsrc = (unsigned)__shfl((int)big, src);
            const int k = __ffs(bsrc) - 1;
            double ye = y[0];
#pragma unroll
            for (int j = 1; j < DISP_BATCH; ++j) ye = k == j ? y[j] : ye;
            const int m = __shfl(disp_count(ye), src);
            const double xs = __shfl(xi, src);
            const uint32_t ss = (uint32_t)__shfl((int)s0, src);
            const uint32_t elem = (uint32_t)(a.elem0 + (uint64_t)(u + k));
            int c = 0;
#pragma unroll 1
            for (int j = lane; 2 * j + 1 < m; j += 64) c += disp_call(a, elem, ss, j, m, xs);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
            if (lane == src) { l += c; big &= big - 1; }
        }
    }
    redS[wave][lane] = s;
    redL[wave][lane] = l;
    __syncthreads();
    if (wave == 0 && own) {
        const long at = (long)blockIdx.x * a.nloc + n;
        partS[at] = ((redS[0][lane] + redS[1][lane]) + redS[2][lane]) + redS[3][lane];
        partL[at] = redL[0][lane] + redL[1][lane] + redL[2][lane] + redL[3][lane];
    }
}

__global__ __launch_bounds__(256) void disp_finish_kernel(const double* __restrict__ partS, const long long* __restrict__ partL, int nblk, int nloc,
                                                          long long* __restrict__ L, double* __restrict__ S, int accumulate) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= nloc) return;
    double s = 0.0;
    long long l = 0;
    for (int b = 0; b < nblk; ++b) {
        s += partS[(long)b * nloc + n];
        l += partL[(long)b * nloc + n];
    }
    S[n] = accumulate ? S[n] + s : s;
    L[n] = accumulate ? L[n] + l : l;
}

inline long disp_blocks(long T) { return (T + PGL_DISPERSION_ROWS - 1) / PGL_DISPERSION_ROWS; }

}  // namespace

extern "C" size_t pgl_dispersion_work_bytes(int nloc, int T) {
    if (nloc < 1 || T < 0) return 0;
    const size_t bytes = (size_t)disp_blocks(T) * (size_t)nloc * (sizeof(double) + sizeof(long long));
    return bytes < 16 ? 16 : bytes;
}

extern "C" int pgl_dispersion_fold(const double* Psi, long ldn, const double* bias, const double* Y, int T, int nloc, const double* xi, uint64_t seed,
                                   uint64_t sweep, uint64_t neuron0, uint64_t elem0, long long* L, double* S, int accumulate, void* work,
                                   void* hip_stream) {
    PGL_CHECK_ARG(nloc >= 1 && T >= 0 && ldn >= nloc && xi && L && S);
    PGL_CHECK_ARG(accumulate == 0 || accumulate == 1);
    PGL_CHECK_ARG(T == 0 || (Psi && Y && work && ((uintptr_t)work % 8) == 0));
    PGL_CHECK_ARG(((long)nloc + 63) / 64 <= 65535 && T <= 2147483647 - PGL_DISPERSION_ROWS);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (T == 0) {
        if (!accumulate && (hipMemsetAsync(L, 0, (size_t)nloc * sizeof(long long), st) != hipSuccess ||
                            hipMemsetAsync(S, 0, (size_t)nloc * sizeof(double), st) != hipSuccess)) {
            pgl_set_error("pgl_dispersion_fold: hipMemsetAsync failed");
            return PGL_ERR_HIP;
        }
        return PGL_OK;
    }
    DispArgs a;
    a.Psi = Psi; a.ldn = ldn; a.bias = bias; a.Y = Y; a.T = T; a.nloc = nloc; a.xi = xi;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.s1 = (uint32_t)sweep;
    a.neuron0 = neuron0; a.elem0 = elem0;
    const long nblk = disp_blocks(T);
    double* partS = static_cast<double*>(work);
    long long* partL = reinterpret_cast<long long*>(partS + nblk * nloc);
    hipLaunchKernelGGL(disp_fold_kernel, dim3((unsigned)nblk, (unsigned)((nloc + 63) / 64)), dim3(256), 0, st, a, partS, partL);
    PGL_CHECK_LAUNCH();
    hipLaunchKernelGGL(disp_finish_kernel, dim3((unsigned)((nloc + 255) / 256)), dim3(256), 0, st, partS, partL, (int)nblk, nloc, L, S, accumulate);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}
