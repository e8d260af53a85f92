// Learned network priors for gfx950: the scan over the block assignments of a stochastic block model, the block-to-block edge counts and the
// fold of a sampled partition (pyglm_amd/sbm.py: sbm_scan_host, block_counts_host and BlockStructure state the definitions; include/
// pyglm_hip_sbm.h the calls).  DESIGN.md section 18.
//
//   sbm_check_z_kernel      the pre-pass: one word that says whether a z entry lies outside [0, K)
//   sbm_transpose_kernel    AT[m][n] = A[n][m] != 0, 64 x 64 byte tiles through LDS: column n of A becomes a contiguous read
//   sbm_scan_kernel         ONE workgroup of 1024 threads walks n = 0 .. N - 1.  z lives in LDS, one byte per neuron; thread t owns the partners
//                           m = t, t + 1024, ...  A step's counts cin / cout are integer LDS atomics of the lanes that hold an edge (a sparse A
//                           issues few); cnt comes from the block sizes, which wave 0 keeps in registers.  The steps are pipelined so that ONE
//                           barrier separates them: while wave 0 decides z_n, every wave (wave 0 first) already counts step n + 1 over the
//                           partners m != n, n + 1 -- none of which the pending decision touches -- and wave 0 adds partner n under its new label
//                           once it is known.  Row n + 2 of A and of AT is loaded into registers right after row n + 1 was consumed: the L2
//                           latency runs beside wave 0's arithmetic, off the chain.  What bounds a step is wave 0: 4 K dependent fp64
//                           operations, the max, one exp, K dependent additions, and the barrier.
//   sbm_counts_kernel       grid-stride over the N^2 cells; per-workgroup integer histograms in LDS, then 64-bit integer atomics
//   sbm_fold_kernel         one thread per cell
// No floating-point atomics anywhere: the sums that are not integers are formed by one lane, in the order the header states.
#include "pgl_common.h"
#include "pgl_rng.h"
#include "../../include/pyglm_hip_sbm.h"

namespace {

constexpr int SBM_THREADS = 1024;
constexpr int SBM_PF = 4;                               // passes of the workgroup whose row bytes travel in registers (N <= 4096); later passes load at use
constexpr int SBM_PITCH = PGL_SBM_MAX_BLOCKS + 1;       // row pitch of the tables in LDS: lane k reads [k][l], a stride of 33 doubles
static_assert(PGL_SBM_MAX_BLOCKS <= 64, "one lane per block");
static_assert(PGL_SBM_MAX_BLOCKS <= 255, "z is kept as one byte per neuron");

inline size_t sbm_at_bytes(int N) { return (((size_t)N * (size_t)N) + 15) & ~(size_t)15; }

__global__ __launch_bounds__(256) void sbm_check_z_kernel(const int* __restrict__ z, int N, int K, int* __restrict__ flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N && (z[i] < 0 || z[i] >= K)) atomicOr(flag, 1);
}

__global__ __launch_bounds__(256) void sbm_transpose_kernel(const uint8_t* __restrict__ A, long lda, uint8_t* __restrict__ AT, int N) {
    __shared__ uint8_t tile[64][65];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;         // 64 x 4
    for (int i = ty; i < 64; i += 4) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < N && c < N) ? (uint8_t)(A[(size_t)r * (size_t)lda + c] != 0) : (uint8_t)0;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int r = c0 + i, c = r0 + tx;                          // AT[r][c] = A[c][r]
        if (r < N && c < N) AT[(size_t)r * (size_t)N + c] = tile[tx][i];
    }
}

struct SbmScan {
    const uint8_t* A; const uint8_t* AT; long lda;
    int* z; const double* LP; const double* LQ; const double* logpi; double* lp_out;
    int N, K;
    uint64_t seed, sweep;
};

// s + c * t with the product rounded and the sum rounded: never one fused operation
__device__ __forceinline__ double sbm_add_prod(double s, double c, double t) {
#pragma clang fp contract(off)
    const double p = c * t;
    return s + p;
}

// the bytes of row r that thread t owns in its first SBM_PF passes (0 beyond the row or the matrix)
__device__ __forceinline__ void sbm_load_rows(const SbmScan& g, int r, int t, uint8_t (&in)[SBM_PF], uint8_t (&out)[SBM_PF]) {
#pragma unroll
    for (int p = 0; p < SBM_PF; ++p) {
        const int m = t + p * SBM_THREADS;
        const bool ok = r < g.N && m < g.N;
        in[p] = ok ? g.A[(size_t)r * (size_t)g.lda + m] : (uint8_t)0;
        out[p] = ok ? g.AT[(size_t)r * (size_t)g.N + m] : (uint8_t)0;
    }
}

// the counts of step s over the partners m != s, m != skip, under the labels in zs:  C[0][l] = cin, C[1][l] = cout
__device__ __forceinline__ void sbm_count(const SbmScan& g, int s, int skip, int t, const uint8_t (&in)[SBM_PF], const uint8_t (&out)[SBM_PF],
                                          const uint8_t* zs, int (*C)[PGL_SBM_MAX_BLOCKS]) {
#pragma unroll
    for (int p = 0; p < SBM_PF; ++p) {
        const int m = t + p * SBM_THREADS;
        if (m < g.N && m != s && m != skip && (in[p] | out[p])) {
            const int l = zs[m];
            if (in[p]) atomicAdd(&C[0][l], 1);
            if (out[p]) atomicAdd(&C[1][l], 1);
        }
    }
    for (int m = t + SBM_PF * SBM_THREADS; m < g.N; m += SBM_THREADS) {      // N > 4096: loaded at use
        if (m == s || m == skip) continue;
        const uint8_t ai = g.A[(size_t)s * (size_t)g.lda + m], ao = g.AT[(size_t)s * (size_t)g.N + m];
        if (ai | ao) {
            const int l = zs[m];
            if (ai) atomicAdd(&C[0][l], 1);
            if (ao) atomicAdd(&C[1][l], 1);
        }
    }
}

__global__ __launch_bounds__(SBM_THREADS) void sbm_scan_kernel(SbmScan g) {
    __shared__ uint8_t zs[PGL_SBM_MAX_N];
    __shared__ double sLP[PGL_SBM_MAX_BLOCKS * SBM_PITCH], sLQ[PGL_SBM_MAX_BLOCKS * SBM_PITCH], slogpi[PGL_SBM_MAX_BLOCKS];
    __shared__ int C[2][2][PGL_SBM_MAX_BLOCKS];
    __shared__ int nk0[PGL_SBM_MAX_BLOCKS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int N = g.N, K = g.K;

    for (int i = t; i < K * K; i += SBM_THREADS) {
        sLP[(i / K) * SBM_PITCH + i % K] = g.LP[i];
        sLQ[(i / K) * SBM_PITCH + i % K] = g.LQ[i];
    }
    if (t < K) slogpi[t] = g.logpi[t];
    if (t < 2 * 2 * PGL_SBM_MAX_BLOCKS) (&C[0][0][0])[t] = 0;
    if (t < PGL_SBM_MAX_BLOCKS) nk0[t] = 0;
    __syncthreads();
    for (int m = t; m < N; m += SBM_THREADS) {
        const int zm = g.z[m];                       // in [0, K): the pre-pass has looked
        zs[m] = (uint8_t)zm;
        atomicAdd(&nk0[zm], 1);
    }
    __syncthreads();
    int nk = lane < K ? nk0[lane] : 0;               // block sizes: lane l of wave 0 keeps n_l from here on

    uint8_t rin[SBM_PF], rout[SBM_PF];
    sbm_load_rows(g, 0, t, rin, rout);
    sbm_count(g, 0, -1, t, rin, rout, zs, C[0]);     // step 0 in full
    sbm_load_rows(g, 1, t, rin, rout);
    // partner n of step n + 1, which wave 0 adds once z_n is known: A[n + 1][n] and A[n][n + 1]; loaded one step ahead
    uint8_t pin = 0, pout = 0;
    if (1 < N) { pin = g.A[(size_t)g.lda]; pout = g.AT[(size_t)N]; }
    __syncthreads();

    for (int n = 0; n < N; ++n) {
        const int s = n + 1;
        if (s < N) sbm_count(g, s, n, t, rin, rout, zs, C[s & 1]);
        sbm_load_rows(g, n + 2, t, rin, rout);
        if (wave == 0) {
            uint8_t pin_next = 0, pout_next = 0;
            if (n + 2 < N) {
                pin_next = g.A[(size_t)(n + 2) * (size_t)g.lda + (n + 1)];
                pout_next = g.AT[(size_t)(n + 2) * (size_t)N + (n + 1)];
            }
            // the uniform of this step: it depends on nothing the chain computes
            uint32_t o0, o1, o2, o3;
            pgl_philox4x32_10(PGL_PURPOSE_SBM << 24, (uint32_t)n, (uint32_t)g.sweep, (uint32_t)(g.sweep >> 32), (uint32_t)g.seed,
                              (uint32_t)(g.seed >> 32), o0, o1, o2, o3);
            const double u = pgl_u64_to_unit((uint64_t)o0 | ((uint64_t)o1 << 32));
            const int zold = zs[n];
            if (lane == zold) nk -= 1;               // cnt[l] over m != n
            int (*Cn)[PGL_SBM_MAX_BLOCKS] = C[n & 1];
            const int k = lane < K ? lane : 0;       // lanes beyond K repeat block 0 and take no part in the decision
            double sum = slogpi[k];
            for (int l = 0; l < K; ++l) {
                const int cnt = __shfl(nk, l), cin = Cn[0][l];
                sum = sbm_add_prod(sum, (double)cin, sLP[k * SBM_PITCH + l]);
                sum = sbm_add_prod(sum, (double)(cnt - cin), sLQ[k * SBM_PITCH + l]);
            }
            for (int l = 0; l < K; ++l) {
                const int cnt = __shfl(nk, l), cout = Cn[1][l];
                sum = sbm_add_prod(sum, (double)cout, sLP[l * SBM_PITCH + k]);
                sum = sbm_add_prod(sum, (double)(cnt - cout), sLQ[l * SBM_PITCH + k]);
            }
            if (g.lp_out && lane < K) g.lp_out[(size_t)n * K + lane] = sum;
            double mx = lane < K ? sum : -1.7976931348623157e308;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
            const double e = exp(sum - mx);
            double c = 0.0, ck = 0.0;
            for (int l = 0; l < K; ++l) {            // c_l = e_0 + .. + e_l from the left, the same on every lane
                c = c + __shfl(e, l);
                if (l == lane) ck = c;
            }
            const unsigned long long hit = __ballot(lane < K && u * c < ck);
            const int znew = hit ? __ffsll((long long)hit) - 1 : K - 1;
            if (lane == znew) nk += 1;
            if (lane == 0) zs[n] = (uint8_t)znew;
            if (lane < K) { Cn[0][lane] = 0; Cn[1][lane] = 0; }      // this buffer is counted into again at step n + 2, behind the next barrier
            if (lane == 0 && s < N) {
                if (pin) atomicAdd(&C[s & 1][0][znew], 1);
                if (pout) atomicAdd(&C[s & 1][1][znew], 1);
            }
            pin = pin_next; pout = pout_next;
        }
        __syncthreads();
    }
    for (int m = t; m < N; m += SBM_THREADS) g.z[m] = zs[m];
}

constexpr int SBM_COUNT_CELLS = 256 * 32;               // cells per workgroup and pass of the grid-stride loop

__global__ __launch_bounds__(256) void sbm_counts_kernel(const uint8_t* __restrict__ A, long lda, const int* __restrict__ z, unsigned long long* M,
                                                         unsigned long long* nk, unsigned long long* diag, int N, int K) {
    __shared__ unsigned int hM[PGL_SBM_MAX_BLOCKS * PGL_SBM_MAX_BLOCKS], hn[PGL_SBM_MAX_BLOCKS], hd;
    for (int i = threadIdx.x; i < K * K; i += 256) hM[i] = 0;
    if (threadIdx.x < PGL_SBM_MAX_BLOCKS) hn[threadIdx.x] = 0;
    if (threadIdx.x == 0) hd = 0;
    __syncthreads();
    const unsigned cells = (unsigned)N * (unsigned)N;   // N <= 32768: at most 2^30
    const unsigned stride = gridDim.x * 256u;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < cells; i += stride) {
        const unsigned n = i / (unsigned)N, m = i - n * (unsigned)N;
        if (A[(size_t)n * (size_t)lda + m] == 0) continue;
        if (n == m) { atomicAdd(&hd, 1u); continue; }
        const int zn = z[n], zm = z[m];
        if (zn >= 0 && zn < K && zm >= 0 && zm < K) atomicAdd(&hM[zn * K + zm], 1u);
    }
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < (unsigned)N; i += stride) {
        const int zi = z[i];
        if (zi >= 0 && zi < K) atomicAdd(&hn[zi], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < K * K; i += 256)
        if (hM[i]) atomicAdd(&M[i], (unsigned long long)hM[i]);
    if (threadIdx.x < K && hn[threadIdx.x]) atomicAdd(&nk[threadIdx.x], (unsigned long long)hn[threadIdx.x]);
    if (threadIdx.x == 0 && hd) atomicAdd(diag, (unsigned long long)hd);
}

__global__ __launch_bounds__(256) void sbm_fold_kernel(const int* __restrict__ z, const double* __restrict__ P, double rho_self,
                                                       uint32_t* __restrict__ coassign, double* __restrict__ rho_sum, int N, int K) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)N * (unsigned)N) return;
    const unsigned n = i / (unsigned)N, m = i - n * (unsigned)N;
    const int zn = z[n], zm = z[m];
    if (zn < 0 || zn >= K || zm < 0 || zm >= K) return;
    coassign[i] += zn == zm ? 1u : 0u;
    rho_sum[i] = rho_sum[i] + (n == m ? rho_self : P[zn * K + zm]);
}

inline bool sbm_dims_ok(int N, int K) { return K >= 1 && K <= PGL_SBM_MAX_BLOCKS && N >= 0 && N <= PGL_SBM_MAX_N; }

}  // namespace

extern "C" size_t pgl_sbm_work_bytes(int N) {
    if (N < 0 || N > PGL_SBM_MAX_N) return 0;
    return sbm_at_bytes(N) + 16;
}

extern "C" int pgl_sbm_scan(const uint8_t* A, int* z, const double* LP, const double* LQ, const double* logpi, double* lp_out, void* work, int N,
                            int K, long lda, unsigned long long seed, unsigned long long sweep, void* hip_stream) {
    PGL_CHECK_ARG(sbm_dims_ok(N, K) && lda >= N);
    PGL_CHECK_ARG(A && z && LP && LQ && logpi && work);
    if (N == 0) return PGL_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    uint8_t* AT = static_cast<uint8_t*>(work);
    int* flag = reinterpret_cast<int*>(AT + sbm_at_bytes(N));
    int bad = 0;
    if (hipMemsetAsync(flag, 0, sizeof(int), st) != hipSuccess) { pgl_set_error("pgl_sbm_scan: hipMemsetAsync failed"); return PGL_ERR_HIP; }
    hipLaunchKernelGGL(sbm_check_z_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, z, N, K, flag);
    PGL_CHECK_LAUNCH();
    if (hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        pgl_set_error("pgl_sbm_scan: reading the pre-pass's word failed: %s", hipGetErrorString(hipGetLastError()));
        return PGL_ERR_HIP;
    }
    if (bad) {
        pgl_set_error("pgl_sbm_scan: a z entry lies outside [0, %d)", K);
        return PGL_ERR_ARG;
    }
    const unsigned tiles = (unsigned)((N + 63) / 64);
    hipLaunchKernelGGL(sbm_transpose_kernel, dim3(tiles, tiles), dim3(256), 0, st, A, lda, AT, N);
    PGL_CHECK_LAUNCH();
    SbmScan g;
    g.A = A; g.AT = AT; g.lda = lda; g.z = z; g.LP = LP; g.LQ = LQ; g.logpi = logpi; g.lp_out = lp_out;
    g.N = N; g.K = K; g.seed = seed; g.sweep = sweep;
    hipLaunchKernelGGL(sbm_scan_kernel, dim3(1), dim3(SBM_THREADS), 0, st, g);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}

extern "C" int pgl_sbm_block_counts(const uint8_t* A, const int* z, long long* M, long long* nk, long long* diag, int N, int K, long lda,
                                    void* hip_stream) {
    PGL_CHECK_ARG(sbm_dims_ok(N, K) && lda >= N);
    PGL_CHECK_ARG(A && z && M && nk && diag);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (hipMemsetAsync(M, 0, sizeof(long long) * K * K, st) != hipSuccess || hipMemsetAsync(nk, 0, sizeof(long long) * K, st) != hipSuccess ||
        hipMemsetAsync(diag, 0, sizeof(long long), st) != hipSuccess) {
        pgl_set_error("pgl_sbm_block_counts: hipMemsetAsync failed");
        return PGL_ERR_HIP;
    }
    if (N == 0) return PGL_OK;
    const size_t cells = (size_t)N * (size_t)N;
    size_t blocks = (cells + SBM_COUNT_CELLS - 1) / SBM_COUNT_CELLS;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sbm_counts_kernel, dim3((unsigned)blocks), dim3(256), 0, st, A, lda, z, reinterpret_cast<unsigned long long*>(M),
                       reinterpret_cast<unsigned long long*>(nk), reinterpret_cast<unsigned long long*>(diag), N, K);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}

extern "C" int pgl_sbm_fold(const int* z, const double* P, double rho_self, uint32_t* coassign, double* rho_sum, int N, int K, void* hip_stream) {
    PGL_CHECK_ARG(sbm_dims_ok(N, K));
    PGL_CHECK_ARG(z && P && coassign && rho_sum);
    if (N == 0) return PGL_OK;
    const size_t cells = (size_t)N * (size_t)N;
    hipLaunchKernelGGL(sbm_fold_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(hip_stream), z, P, rho_self,
                       coassign, rho_sum, N, K);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}
