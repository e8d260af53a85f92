// External covariates (pyglm_amd/covariates.py states the law; include/pyglm_hip_covariates.h the calls):
// psi = X . vec(a * W) + b + o with o = S beta, S [T][K] shared by all neurons, and the Gibbs step beta_n | omega, W, b.
//
//   cov_offset_kernel       Off = S Beta.  One workgroup = 64 rows of time of 64 columns; its slice of Beta ([K][64]) and its rows of S go to
//                           LDS once, lane = column, the waves take the rows in turn.  A rounded product and a rounded sum per term, k
//                           ascending from 0.0: the host loop's bits.
//   cov_add_kernel          Psi += Off, and
//   cov_kappa_kernel        Kappa -= Omega * Off: the two elementwise steps of a sweep under an offset.
//   cov_fold_kernel<DIAG>   the likelihood parts of Lambda_n (lower triangle) and r_n.  The (j, k) pairs are cut into 8 x 8 blocks of the
//                           triangle; a workgroup owns PGL_COVARIATE_ROWS rows of time of 64 columns and ONE block.  A diagonal block holds
//                           36 sums of Lambda and 8 of r per lane (reads Omega, Kappa, Off, Psi: 32 bytes per cell); a block below the
//                           diagonal 64 sums of Lambda (reads Omega alone).  The block's 16 columns of S are staged in LDS (zero past T and K)
//                           and read as broadcasts; each of the 4 waves walks its 64 rows in time order, four rows' loads in flight; the
//                           waves then add their sums in wave order through LDS (which reuses the staging area) and the workgroup writes
//                           one partial per sum and column to `work`: [time block][sum][nloc].
//   cov_finish_kernel       one thread per (sum, column) adds the workgroups' partials in time order and alone writes Lambda and r.
//   cov_draw_kernel         one wavefront per neuron, the K x K system in LDS: Cholesky, forward solve, add z, backward solve.
// No floating-point atomics: every sum is formed by one thread in an order fixed by T, so a column's Lambda and r have the same bits
// whatever nloc, neuron0 or the shard.
#include "pgl_common.h"
#include "../../include/pyglm_hip_covariates.h"

namespace {

constexpr int COV_WAVES = 4;
constexpr int COV_WAVE_ROWS = PGL_COVARIATE_ROWS / COV_WAVES;       // rows of time one wave walks
constexpr int COV_BATCH = 4;                                        // rows whose loads are in flight together
constexpr int COV_BLK = 8;                                          // edge of a block of (j, k) pairs
constexpr int COV_TILE = 64;                                        // rows and columns of a workgroup of the offset kernel
static_assert(PGL_COVARIATE_ROWS % COV_WAVES == 0 && COV_WAVE_ROWS % COV_BATCH == 0, "a wave walks whole batches");
static_assert(PGL_COVARIATE_MAX % COV_BLK == 0 && PGL_COVARIATE_MAX <= 32, "the draw holds a 32 x 32 system per wave");

__global__ __launch_bounds__(256) void cov_offset_kernel(const double* __restrict__ S, long lds, const double* __restrict__ Beta, double* __restrict__ Off,
                                                         long ldn, int T, int nloc, int K) {
#pragma clang fp contract(off)                        // the product is rounded, then the sum: what offset_host does
    __shared__ double sB[PGL_COVARIATE_MAX][COV_TILE];
    __shared__ double sS[COV_TILE][PGL_COVARIATE_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)blockIdx.x * COV_TILE;
    const int col0 = blockIdx.y * COV_TILE;
    for (int e = tid; e < K * COV_TILE; e += 256) {
        const int k = e >> 6, n = col0 + (e & 63);
        sB[k][e & 63] = n < nloc ? Beta[(long)k * ldn + n] : 0.0;
    }
    for (int e = tid; e < COV_TILE * K; e += 256) {
        const int row = e / K, k = e - row * K;
        const long t = row0 + row;
        sS[row][k] = t < T ? S[t * lds + k] : 0.0;
    }
    __syncthreads();
    const int n = col0 + lane;
    for (int row = wave; row < COV_TILE; row += COV_WAVES) {
        const long t = row0 + row;
        if (t >= T) break;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) acc = acc + sS[row][k] * sB[k][lane];
        if (n < nloc) Off[t * ldn + n] = acc;
    }
}

__global__ __launch_bounds__(256) void cov_add_kernel(double* __restrict__ Psi, long ldpsi, const double* __restrict__ Off, long ldo, long cells, int nloc) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= cells) return;
    const long t = e / nloc, n = e - t * nloc;
    Psi[t * ldpsi + n] += Off[t * ldo + n];
}

__global__ __launch_bounds__(256) void cov_kappa_kernel(double* __restrict__ Kappa, long ldk, const double* __restrict__ Omega, long ldo2,
                                                        const double* __restrict__ Off, long ldo, long cells, int nloc) {
#pragma clang fp contract(off)                        // one product, one difference
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= cells) return;
    const long t = e / nloc, n = e - t * nloc;
    const double p = Omega[t * ldo2 + n] * Off[t * ldo + n];
    Kappa[t * ldk + n] = Kappa[t * ldk + n] - p;
}

struct CovArgs {
    const double *Psi, *bias, *Omega, *Kappa, *Off, *S;
    long ldn, ldo, ldk, lds;
    int T, nloc, K, nsum, nkind;                      // nsum = K (K + 1) / 2 + K; nkind: blocks of this launch's kind
};

// blockIdx.x = time block * nkind + block of this kind: the workgroups that read one tile of the data are neighbours in the launch order
template <bool DIAG>
__global__ __launch_bounds__(256) void cov_fold_kernel(CovArgs a, double* __restrict__ part) {
    constexpr int NL = DIAG ? COV_BLK * (COV_BLK + 1) / 2 : COV_BLK * COV_BLK;      // sums of Lambda a lane holds
    constexpr int NS = DIAG ? NL + COV_BLK : NL;                                    // ... and of r
    __shared__ double sm[PGL_COVARIATE_ROWS * 2 * COV_BLK];     // the block's columns of S, [row][j part | k part]; then the waves' sums [sum][lane]
    static_assert(NS * 64 <= PGL_COVARIATE_ROWS * 2 * COV_BLK, "the sums fit where S was staged");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kb = blockIdx.x % a.nkind, tb = blockIdx.x / a.nkind;
    int bj = kb, bk = kb;
    if (!DIAG) {                                      // kb = bj (bj - 1) / 2 + bk, bk < bj
        bj = 1;
        int rem = kb;
        while (rem >= bj) { rem -= bj; ++bj; }
        bk = rem;
    }
    const long row0 = (long)tb * PGL_COVARIATE_ROWS;
    for (int e = tid; e < PGL_COVARIATE_ROWS * 2 * COV_BLK; e += 256) {
        const int row = e >> 4, c = e & 15;
        const long t = row0 + row;
        const int col = c < COV_BLK ? bj * COV_BLK + c : bk * COV_BLK + c - COV_BLK;
        sm[e] = (t < a.T && col < a.K) ? a.S[t * a.lds + col] : 0.0;
    }
    __syncthreads();
    const int n = blockIdx.z * 64 + lane;
    const bool own = n < a.nloc;
    const int nc = own ? n : a.nloc - 1;              // a lane past the last column reads that column and owns nothing
    const double bn = (DIAG && a.bias) ? a.bias[nc] : 0.0;
    double acc[NL], racc[COV_BLK];
#pragma unroll
    for (int i = 0; i < NL; ++i) acc[i] = 0.0;
#pragma unroll
    for (int i = 0; i < COV_BLK; ++i) racc[i] = 0.0;
    const int u0 = wave * COV_WAVE_ROWS;
    for (int u = u0; u < u0 + COV_WAVE_ROWS; u += COV_BATCH) {
        if (row0 + u >= a.T) break;                   // (the wave's: every lane makes the same trips)
        double w[COV_BATCH], kp[COV_BATCH], of[COV_BATCH], ps[COV_BATCH];
#pragma unroll
        for (int q = 0; q < COV_BATCH; ++q) {
            const long t = row0 + u + q;
            const bool in = t < a.T;
            w[q] = in ? a.Omega[t * a.ldo + nc] : 0.0;
            if (DIAG) {
                kp[q] = in ? a.Kappa[t * a.ldk + nc] : 0.0;
                of[q] = in ? a.Off[t * a.ldn + nc] : 0.0;
                ps[q] = in ? a.Psi[t * a.ldn + nc] : 0.0;
            }
        }
#pragma unroll
        for (int q = 0; q < COV_BATCH; ++q) {
            const double* s = sm + (u + q) * 2 * COV_BLK;             // (a row past T holds zeros: it adds nothing)
            double sj[COV_BLK], sk[COV_BLK];
#pragma unroll
            for (int j = 0; j < COV_BLK; ++j) { sj[j] = s[j]; sk[j] = DIAG ? s[j] : s[COV_BLK + j]; }
#pragma unroll
            for (int j = 0; j < COV_BLK; ++j) {
                const double wj = w[q] * sj[j];
#pragma unroll
                for (int k = 0; k < COV_BLK; ++k) {
                    if (DIAG && k > j) continue;
                    const int i = DIAG ? j * (j + 1) / 2 + k : j * COV_BLK + k;
                    acc[i] += wj * sk[k];
                }
            }
            if (DIAG) {
                const double c = kp[q] + w[q] * (of[q] - (ps[q] + bn));
#pragma unroll
                for (int j = 0; j < COV_BLK; ++j) racc[j] += sj[j] * c;
            }
        }
    }
    __syncthreads();                                   // every wave is done with the staged S: its place takes the sums
    for (int v = 0; v < COV_WAVES; ++v) {              // wave 0 stores, waves 1, 2, 3 add in turn: the sums join in time order
        if (wave == v) {
#pragma unroll
            for (int i = 0; i < NL; ++i) sm[i * 64 + lane] = v ? sm[i * 64 + lane] + acc[i] : acc[i];
            if (DIAG) {
#pragma unroll
                for (int i = 0; i < COV_BLK; ++i) sm[(NL + i) * 64 + lane] = v ? sm[(NL + i) * 64 + lane] + racc[i] : racc[i];
            }
        }
        __syncthreads();
    }
    if (!own) return;
    const int P = a.K * (a.K + 1) / 2;
    for (int i = wave; i < NS; i += COV_WAVES) {       // sum i of the block -> its place among the nsum sums of a column
        int gid;
        if (i < NL) {
            int j, k;
            if (DIAG) { j = 0; while ((j + 1) * (j + 2) / 2 <= i) ++j; k = i - j * (j + 1) / 2; }
            else { j = i / COV_BLK; k = i % COV_BLK; }
            const int J = bj * COV_BLK + j, Kc = bk * COV_BLK + k;
            if (J >= a.K || Kc >= a.K) continue;
            gid = J * (J + 1) / 2 + Kc;
        } else {
            const int J = bj * COV_BLK + (i - NL);
            if (J >= a.K) continue;
            gid = P + J;
        }
        part[((long)tb * a.nsum + gid) * a.nloc + n] = sm[i * 64 + lane];
    }
}

__global__ __launch_bounds__(256) void cov_finish_kernel(const double* __restrict__ part, int nblk, int nloc, int K, double* __restrict__ Lambda,
                                                         double* __restrict__ r, int accumulate) {
    const int P = K * (K + 1) / 2, nsum = P + K;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)nsum * nloc) return;
    const int gid = (int)(e / nloc), n = (int)(e - (long)gid * nloc);
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[((long)b * nsum + gid) * nloc + n];
    double* out = gid < P ? Lambda + (long)n * P + gid : r + (long)n * K + (gid - P);
    *out = accumulate ? *out + s : s;
}

__global__ __launch_bounds__(256) void cov_draw_kernel(const double* __restrict__ Lambda, const double* __restrict__ r, const double* __restrict__ Lambda0,
                                                       const double* __restrict__ h0, const double* __restrict__ z, double* __restrict__ Beta,
                                                       int* __restrict__ status, int nloc, int K) {
    constexpr int LD = PGL_COVARIATE_MAX + 1;
    __shared__ double sA[COV_WAVES][PGL_COVARIATE_MAX * LD];
    __shared__ double sx[COV_WAVES][PGL_COVARIATE_MAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * COV_WAVES + wave;
    const bool own = n < nloc;
    const int nc = own ? n : nloc - 1;                 // a wave past the last neuron works on that neuron and writes nothing: every wave
    double* A = sA[wave];                              // makes the same trips to the barriers
    double* x = sx[wave];
    const int P = K * (K + 1) / 2;
    for (int e = lane; e < K * K; e += 64) {
        const int j = e / K, k = e - j * K;
        if (k <= j) A[j * LD + k] = Lambda0[j * K + k] + Lambda[(long)nc * P + j * (j + 1) / 2 + k];
    }
    if (lane < K) x[lane] = h0[lane] + r[(long)nc * K + lane];
    __syncthreads();
    bool bad = false;
    for (int j = 0; j < K; ++j) {                      // A = L L', column by column; lane = row
        double d = A[j * LD + j];
        if (!(d > 0.0)) { bad = true; d = 1.0; }       // (goes on, so that the barriers are met; nothing of it is written)
        const double l = sqrt(d);
        __syncthreads();
        if (lane >= j && lane < K) A[lane * LD + j] = lane == j ? l : A[lane * LD + j] / l;
        __syncthreads();
        if (lane > j && lane < K) {
            const double lij = A[lane * LD + j];
            for (int k = j + 1; k <= lane; ++k) A[lane * LD + k] -= lij * A[k * LD + j];
        }
        __syncthreads();
    }
    for (int j = 0; j < K; ++j) {                      // y = L^-1 (h0 + r)
        const double yj = x[j] / A[j * LD + j];
        __syncthreads();
        if (lane == j) x[j] = yj;
        else if (lane > j && lane < K) x[lane] -= A[lane * LD + j] * yj;
        __syncthreads();
    }
    if (lane < K) x[lane] += z[(long)nc * K + lane];
    __syncthreads();
    for (int j = K - 1; j >= 0; --j) {                 // beta = L^-T (y + z)
        const double xj = x[j] / A[j * LD + j];
        __syncthreads();
        if (lane == j) x[j] = xj;
        else if (lane < j) x[lane] -= A[j * LD + lane] * xj;
        __syncthreads();
    }
    if (!own) return;
    if (bad) { if (lane == 0) status[n] |= 1; return; }
    if (lane < K) Beta[(long)n * K + lane] = x[lane];
}

inline long cov_blocks(long T) { return (T + PGL_COVARIATE_ROWS - 1) / PGL_COVARIATE_ROWS; }
inline bool cov_grid_ok(long blocks) { return blocks >= 0 && blocks <= 2147483647L; }

}  // namespace

extern "C" int pgl_covariate_max(void) { return PGL_COVARIATE_MAX; }

extern "C" int pgl_covariate_offset(const double* S, long lds, const double* Beta, double* Off, long ldn, int T, int nloc, int K, void* hip_stream) {
    PGL_CHECK_ARG(K >= 1 && K <= PGL_COVARIATE_MAX && nloc >= 1 && T >= 0 && lds >= K && ldn >= nloc && Beta);
    PGL_CHECK_ARG(T == 0 || (S && Off));
    PGL_CHECK_ARG(((long)nloc + COV_TILE - 1) / COV_TILE <= 65535);
    if (T == 0) return PGL_OK;
    hipLaunchKernelGGL(cov_offset_kernel, dim3((unsigned)(((long)T + COV_TILE - 1) / COV_TILE), (unsigned)((nloc + COV_TILE - 1) / COV_TILE)), dim3(256), 0,
                       static_cast<hipStream_t>(hip_stream), S, lds, Beta, Off, ldn, T, nloc, K);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}

extern "C" int pgl_covariate_add_offset(double* Psi, long ldpsi, const double* Off, long ldo, int T, int nloc, void* hip_stream) {
    PGL_CHECK_ARG(nloc >= 1 && T >= 0 && ldpsi >= nloc && ldo >= nloc && (T == 0 || (Psi && Off)));
    const long cells = (long)T * nloc;
    PGL_CHECK_ARG(cov_grid_ok((cells + 255) / 256));
    if (T == 0) return PGL_OK;
    hipLaunchKernelGGL(cov_add_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(hip_stream), Psi, ldpsi, Off, ldo,
                       cells, nloc);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}

extern "C" int pgl_covariate_reduce_kappa(double* Kappa, long ldk, const double* Omega, long ldo2, const double* Off, long ldo, int T, int nloc,
                                          void* hip_stream) {
    PGL_CHECK_ARG(nloc >= 1 && T >= 0 && ldk >= nloc && ldo2 >= nloc && ldo >= nloc && (T == 0 || (Kappa && Omega && Off)));
    const long cells = (long)T * nloc;
    PGL_CHECK_ARG(cov_grid_ok((cells + 255) / 256));
    if (T == 0) return PGL_OK;
    hipLaunchKernelGGL(cov_kappa_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(hip_stream), Kappa, ldk, Omega,
                       ldo2, Off, ldo, cells, nloc);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}

extern "C" size_t pgl_covariate_work_bytes(int nloc, int T, int K) {
    if (nloc < 1 || T < 0 || K < 1 || K > PGL_COVARIATE_MAX) return 0;
    const size_t bytes = (size_t)cov_blocks(T) * (size_t)(K * (K + 1) / 2 + K) * (size_t)nloc * sizeof(double);
    return bytes < 16 ? 16 : bytes;
}

extern "C" int pgl_covariate_fold(const double* Psi, long ldn, const double* bias, const double* Omega, long ldo, const double* Kappa, long ldk,
                                  const double* Off, const double* S, long lds, int T, int nloc, int K, double* Lambda, double* r, int accumulate,
                                  void* work, void* hip_stream) {
    PGL_CHECK_ARG(K >= 1 && K <= PGL_COVARIATE_MAX && nloc >= 1 && T >= 0 && ldn >= nloc && ldo >= nloc && ldk >= nloc && lds >= K && Lambda && r);
    PGL_CHECK_ARG(accumulate == 0 || accumulate == 1);
    PGL_CHECK_ARG(T == 0 || (Psi && Omega && Kappa && Off && S && work && ((uintptr_t)work % 8) == 0));
    const int P = K * (K + 1) / 2, nsum = P + K, KB = (K + COV_BLK - 1) / COV_BLK;
    const long nblk = cov_blocks(T);
    PGL_CHECK_ARG(((long)nloc + 63) / 64 <= 65535 && cov_grid_ok(nblk * (KB * (KB + 1) / 2)) && cov_grid_ok(((long)nsum * nloc + 255) / 256));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (T == 0) {
        if (!accumulate && (hipMemsetAsync(Lambda, 0, (size_t)nloc * P * sizeof(double), st) != hipSuccess ||
                            hipMemsetAsync(r, 0, (size_t)nloc * K * sizeof(double), st) != hipSuccess)) {
            pgl_set_error("pgl_covariate_fold: hipMemsetAsync failed");
            return PGL_ERR_HIP;
        }
        return PGL_OK;
    }
    CovArgs a;
    a.Psi = Psi; a.bias = bias; a.Omega = Omega; a.Kappa = Kappa; a.Off = Off; a.S = S;
    a.ldn = ldn; a.ldo = ldo; a.ldk = ldk; a.lds = lds; a.T = T; a.nloc = nloc; a.K = K; a.nsum = nsum;
    double* part = static_cast<double*>(work);
    const unsigned gz = (unsigned)((nloc + 63) / 64);
    a.nkind = KB;
    hipLaunchKernelGGL(cov_fold_kernel<true>, dim3((unsigned)(nblk * KB), 1, gz), dim3(256), 0, st, a, part);
    PGL_CHECK_LAUNCH();
    if (KB > 1) {
        a.nkind = KB * (KB - 1) / 2;
        hipLaunchKernelGGL(cov_fold_kernel<false>, dim3((unsigned)(nblk * a.nkind), 1, gz), dim3(256), 0, st, a, part);
        PGL_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(cov_finish_kernel, dim3((unsigned)(((long)nsum * nloc + 255) / 256)), dim3(256), 0, st, part, (int)nblk, nloc, K, Lambda, r,
                       accumulate);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}

extern "C" int pgl_covariate_draw(const double* Lambda, const double* r, const double* Lambda0, const double* h0, const double* z, double* Beta_out,
                                  int* status, int nloc, int K, void* hip_stream) {
    PGL_CHECK_ARG(K >= 1 && K <= PGL_COVARIATE_MAX && nloc >= 1 && Lambda && r && Lambda0 && h0 && z && Beta_out && status);
    hipLaunchKernelGGL(cov_draw_kernel, dim3((unsigned)((nloc + COV_WAVES - 1) / COV_WAVES)), dim3(256), 0, static_cast<hipStream_t>(hip_stream), Lambda, r,
                       Lambda0, h0, z, Beta_out, status, nloc, K);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}
