// Lagged cross products of spike trains: S[r][l][i][j] (+)= sum_u Y_r[u - l][i] * Y_r[u][j]  ("neuron i leads neuron j by l bins"), the pairwise
// statistic of the posterior predictive check (pyglm_amd/simulate.py: correlogram).  DESIGN.md section 12.
//
// PGL_LAG_I8 -- the counts themselves on the integer matrix cores, exact:
//   lag_convert_kernel  the prev + rows rows of Y as int8, time-contiguous per neuron: Q[r][n][F + u], u = -prev .. rows - 1 (u = 0 the first new
//                       row), zero everywhere else -- F = lag_front(K) bytes in front (a multiple of 64, > K - 1), the rows up to a multiple of 64
//                       and the neurons up to a multiple of 16 behind.  A value that is no integer of [-127, 127] sets status = {3, row, replicate,
//                       neuron} (first writer wins).
//   lag_product_kernel  one workgroup = one 16 x 16 block of neuron pairs, 64 lags (4 waves x 16 lags) and a span of time of one replicate.  Per slab
//                       of LAG_TT bins it stages 16 rows of the "current" operand (neuron j, bytes u .. u + LAG_TT) and 16 rows of the "past" operand
//                       (neuron i, bytes u - L0 - 64 .. u - L0 + LAG_TT: one staged tile serves all 64 lags).  v_mfma_i32_16x16x64_i8 contracts
//                       64 bins: lane (n, g) holds bytes 16 g .. 16 g + 15 of neuron n for both operands.  The past operand of lag l0 + s is the
//                       current window moved back by l0 + s bytes: the lane reads the 32 bytes from 16 bytes before its window of lag l0 with TWO
//                       ALIGNED ds_read_b128 and forms the 16 shifted fragments in registers, 4 v_alignbyte_b32 each (none for s = 0) -- no
//                       misaligned LDS read, and 3 LDS reads feed 16 MFMAs.  Which operand carries the shift is immaterial to the sum; shifting
//                       the past one makes "u >= 0" the loop bound and "u - l >= -prev" the zero padding, so no product needs a mask.
//                       The int32 sums of a workgroup cover at most LAG_FLUSH = 65 536 bins (127^2 * 65 536 < 2^30); they are added to S as doubles:
//                       every partial sum is an integer below 2^53, so the additions are exact in any order, and time may be split over workgroups
//                       (atomic adds) whenever the pairs alone do not fill the chip.  The kernel reads status first and leaves S alone if it is set.
// PGL_LAG_F64 -- any real Y: the window is copied to `work` with an even row length and 16 zero rows behind, and lag l is one PGL_GEMM_PLAIN
//                       contraction (pgl_gemm.hip) of the rows u - l against the rows u, batched over the replicates.
#include "pgl_common.h"

typedef int v4i __attribute__((ext_vector_type(4)));

namespace {

constexpr int LAG_TT = 512;               // bins per staged slab
constexpr int LAG_WG_LAGS = 64;           // lags per workgroup (4 waves x 16)
constexpr int LAG_FLUSH = 65536;          // bins per int32 accumulation at most
constexpr int LAG_CS = LAG_TT + 16;       // LDS row strides: one 16-byte slot of padding, so that the 16 rows of a fragment read fall in 16 slots
constexpr int LAG_PS = LAG_TT + 64 + 16;

inline int lag_front(int K) { return ((K - 1) / LAG_WG_LAGS + 1) * LAG_WG_LAGS; }
inline long lag_row_bytes(int K, int rows) { return lag_front(K) + ((long)rows + 63) / 64 * 64; }
inline int lag_np16(int N) { return (N + 15) / 16 * 16; }

__global__ __launch_bounds__(256) void lag_convert_kernel(const double* __restrict__ Y, long ldy, long strideY, int rows, int prev, int N, int Np, int F,
                                                          long Tq, int8_t* __restrict__ Q, int* __restrict__ status) {
    __shared__ int8_t tile[64][68];
    const int r = blockIdx.z, n0 = blockIdx.y * 64;
    const long c0 = (long)blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const double* Yr = Y + (long)r * strideY;
    const int n = n0 + tx;
    for (int t = ty; t < 64; t += 4) {
        const long u = c0 + t - F;
        int8_t q = 0;
        if (n < N && u >= -(long)prev && u < rows) {
            const double v = Yr[u * ldy + n];
            const bool ok = v >= -127.0 && v <= 127.0 && (double)(int)v == v;
            if (ok) q = (int8_t)(int)v;
            else if (atomicCAS(status, 0, 3) == 0) { status[1] = (int)u; status[2] = r; status[3] = n; }
        }
        tile[tx][t] = q;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * 16; idx += 256) {
        const int nn = idx >> 4, dw = idx & 15;
        if (n0 + nn < Np)
            *reinterpret_cast<int*>(Q + ((long)r * Np + n0 + nn) * Tq + c0 + 4 * dw) = *reinterpret_cast<const int*>(&tile[nn][4 * dw]);
    }
}

__global__ __launch_bounds__(256) void lag_zero_kernel(double* __restrict__ S, long strideS, long len, const int* __restrict__ status) {
    if (status[0] == 3) return;
    double* Sr = S + (long)blockIdx.y * strideS;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < len; i += (long)gridDim.x * 256) Sr[i] = 0.0;
}

struct LagArgs {
    const int8_t* Q; long Tq; int Np, F;
    int rows64, span;                // bins (padded to 64), bins per time split (a multiple of 64, <= LAG_FLUSH)
    int N, K, ntile, nlg;
    double* S; long strideS;
    int accumulate, atomic;
    const int* status;
};

// fragment of lag l0 + S_ from the 32-byte window w (bytes 16 - S_ .. 31 - S_)
template <int S_>
__device__ __forceinline__ v4i lag_shift(const int (&w)[8]) {
    constexpr int o = 16 - S_, q = o >> 2, sh = o & 3;
    v4i f;
    if constexpr (sh == 0) {
        f = v4i{w[q], w[q + 1], w[q + 2], w[q + 3]};
    } else {
        f[0] = (int)__builtin_amdgcn_alignbyte((unsigned)w[q + 1], (unsigned)w[q], sh);
        f[1] = (int)__builtin_amdgcn_alignbyte((unsigned)w[q + 2], (unsigned)w[q + 1], sh);
        f[2] = (int)__builtin_amdgcn_alignbyte((unsigned)w[q + 3], (unsigned)w[q + 2], sh);
        f[3] = (int)__builtin_amdgcn_alignbyte((unsigned)w[q + 4], (unsigned)w[q + 3], sh);
    }
    return f;
}

template <int S_>
__device__ __forceinline__ void lag_steps(v4i (&acc)[16], const int (&w)[8], const v4i& c) {
    if constexpr (S_ < 16) {
        acc[S_] = __builtin_amdgcn_mfma_i32_16x16x64_i8(lag_shift<S_>(w), c, acc[S_], 0, 0, 0);
        lag_steps<S_ + 1>(acc, w, c);
    }
}

__global__ __launch_bounds__(256) void lag_product_kernel(LagArgs a) {
    if (a.status[0] == 3) return;
    __shared__ __attribute__((aligned(16))) int8_t Cs[16 * LAG_CS];
    __shared__ __attribute__((aligned(16))) int8_t Ps[16 * LAG_PS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g = lane >> 4;
    int b = blockIdx.x;
    const int tj = b % a.ntile; b /= a.ntile;
    const int ti = b % a.ntile; b /= a.ntile;
    const int L0 = b * LAG_WG_LAGS, l0 = L0 + 16 * wave;
    const int r = blockIdx.z;
    const int ua = blockIdx.y * a.span, ub = min(a.rows64, ua + a.span);
    if (ua >= ub) return;
    const bool live = l0 < a.K;                                    // a wave whose 16 lags are all >= K only helps staging
    const int8_t* Qc = a.Q + ((long)r * a.Np + tj * 16) * a.Tq + a.F;              // byte u of neuron row 0 of the tile
    const int8_t* Qp = a.Q + ((long)r * a.Np + ti * 16) * a.Tq + a.F - L0 - 64;
    v4i acc[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) acc[s] = v4i{0, 0, 0, 0};
    for (int u0 = ua; u0 < ub; u0 += LAG_TT) {
        const int len = min(LAG_TT, ub - u0);                      // a multiple of 64
        const int cv = len >> 4, pv = (len + 64) >> 4;             // 16-byte vectors per row
        __syncthreads();
        for (int idx = tid; idx < 16 * cv; idx += 256) {
            const int row = idx / cv, v = idx - row * cv;
            *reinterpret_cast<v4i*>(Cs + row * LAG_CS + 16 * v) = *reinterpret_cast<const v4i*>(Qc + (long)row * a.Tq + u0 + 16 * v);
        }
        for (int idx = tid; idx < 16 * pv; idx += 256) {
            const int row = idx / pv, v = idx - row * pv;
            *reinterpret_cast<v4i*>(Ps + row * LAG_PS + 16 * v) = *reinterpret_cast<const v4i*>(Qp + (long)row * a.Tq + u0 + 16 * v);
        }
        __syncthreads();
        if (!live) continue;
        const int8_t* cp = Cs + n * LAG_CS + 16 * g;
        const int8_t* pp = Ps + n * LAG_PS + 16 * g + 48 - 16 * wave;       // 16 bytes before the window of lag l0
        for (int ks = 0; ks < len; ks += 64) {
            const v4i c = *reinterpret_cast<const v4i*>(cp + ks);
            const v4i w0 = *reinterpret_cast<const v4i*>(pp + ks);
            const v4i w1 = *reinterpret_cast<const v4i*>(pp + ks + 16);
            const int w[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
            lag_steps<0>(acc, w, c);
        }
    }
    if (!live) return;
    // i32 C/D fragment: row = 4 * (lane >> 4) + reg, col = lane & 15
    const int j = tj * 16 + n;
    double* Sr = a.S + (long)r * a.strideS;
    // four lags at a time: their 16 read-modify-write loads are in flight together (S is the traffic of a fold: DESIGN.md section 12)
#pragma unroll
    for (int s0 = 0; s0 < 16; s0 += 4) {
        double old[4][4];
        bool ok[4][4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int l = l0 + s0 + s, i = ti * 16 + 4 * g + q;
                ok[s][q] = l < a.K && i < a.N && j < a.N;
                old[s][q] = (ok[s][q] && !a.atomic && a.accumulate) ? Sr[((long)l * a.N + i) * a.N + j] : 0.0;
            }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (!ok[s][q]) continue;
                const int l = l0 + s0 + s, i = ti * 16 + 4 * g + q;
                double* p = Sr + ((long)l * a.N + i) * a.N + j;
                const int v = acc[s0 + s][q];
                if (a.atomic) {
                    if (v != 0) unsafeAtomicAdd(p, (double)v);
                } else {
                    *p = old[s][q] + (double)v;
                }
            }
    }
}

__global__ __launch_bounds__(256) void lag_pack_kernel(const double* __restrict__ Y, long ldy, long strideY, int nrows, int N, double* __restrict__ W,
                                                       int ldw, int rowsW) {
    const long total = (long)rowsW * ldw;
    const double* Yr = Y + (long)blockIdx.y * strideY;
    double* Wr = W + (long)blockIdx.y * total;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long q = i / ldw;
        const int c = (int)(i - q * ldw);
        Wr[i] = (q < nrows && c < N) ? Yr[q * ldy + c] : 0.0;
    }
}

int lag_i8(const double* Y, long ldy, long strideY, int rows, int prev, int N, int K, int R, double* S, long strideS, int accumulate, void* work,
           int* status, hipStream_t st) {
    const int F = lag_front(K), Np = lag_np16(N);
    const long Tq = lag_row_bytes(K, rows);
    int8_t* Q = static_cast<int8_t*>(work);
    hipLaunchKernelGGL(lag_convert_kernel, dim3((unsigned)(Tq / 64), (unsigned)((Np + 63) / 64), (unsigned)R), dim3(256), 0, st, Y, ldy, strideY, rows,
                       prev, N, Np, F, Tq, Q, status);
    PGL_CHECK_LAUNCH();
    LagArgs a{};
    a.Q = Q; a.Tq = Tq; a.Np = Np; a.F = F;
    a.rows64 = (int)(Tq - F);
    a.N = N; a.K = K; a.ntile = Np / 16; a.nlg = (K + LAG_WG_LAGS - 1) / LAG_WG_LAGS;
    a.S = S; a.strideS = strideS; a.accumulate = accumulate; a.status = status;
    // time is split over workgroups until there are two per compute unit, and always so that no int32 sum covers more than LAG_FLUSH bins
    const long blocks = (long)a.ntile * a.ntile * a.nlg * R;
    const long want = (2L * pgl_device_cus(pgl_device()) + blocks - 1) / blocks;
    const long slabs = (a.rows64 + LAG_TT - 1) / LAG_TT;
    long nsplit = want < slabs ? want : slabs;
    const long need = ((long)a.rows64 + LAG_FLUSH - 1) / LAG_FLUSH;
    if (nsplit < need) nsplit = need;
    if (nsplit < 1) nsplit = 1;
    a.span = (int)((((long)a.rows64 + nsplit - 1) / nsplit + 63) / 64 * 64);
    nsplit = (a.rows64 + a.span - 1) / a.span;
    PGL_CHECK_ARG(a.span <= LAG_FLUSH && nsplit <= 65535 && blocks / R <= 0x7fffffffL && R <= 65535);
    a.atomic = nsplit > 1;
    if (a.atomic && !accumulate) {
        const long len = (long)K * N * N;
        hipLaunchKernelGGL(lag_zero_kernel, dim3((unsigned)((len + 255) / 256 < 4096 ? (len + 255) / 256 : 4096), (unsigned)R), dim3(256), 0, st, S, strideS, len,
                           status);
        PGL_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(lag_product_kernel, dim3((unsigned)(blocks / R), (unsigned)nsplit, (unsigned)R), dim3(256), 0, st, a);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}

int lag_f64(const double* Y, long ldy, long strideY, int rows, int prev, int N, int K, int R, double* S, long strideS, int accumulate, void* work,
            hipStream_t st) {
    const int ldw = (N + 1) & ~1, rowsW = prev + rows + 16;
    double* W = static_cast<double*>(work);
    const long total = (long)rowsW * ldw;
    hipLaunchKernelGGL(lag_pack_kernel, dim3((unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192), (unsigned)R), dim3(256), 0, st,
                       Y - (long)prev * ldy, ldy, strideY, prev + rows, N, W, ldw, rowsW);
    PGL_CHECK_LAUNCH();
    for (int l = 0; l < K; ++l) {
        const int u0 = l > prev ? l - prev : 0;                    // the first new row whose partner u - l exists
        double* Sl = S + (long)l * N * N;
        if (u0 >= rows) {
            if (!accumulate && hipMemset2DAsync(Sl, (size_t)strideS * 8, 0, (size_t)N * N * 8, (size_t)R, st) != hipSuccess) {
                pgl_set_error("pgl_lagged_products: hipMemset2DAsync failed");
                return PGL_ERR_HIP;
            }
            continue;
        }
        PglGemmArgs g{};
        g.A = W + (long)(prev + u0 - l) * ldw; g.lda = ldw; g.strideA = total;
        g.B = W + (long)(prev + u0) * ldw; g.ldb = ldw; g.strideB = total;      // its last rows, up to a multiple of 16, are the zero rows
        g.C = Sl; g.ldc = N; g.strideC = strideS;
        g.M = N; g.N = N; g.K = (rows - u0 + 15) & ~15;
        g.a_cols = ldw; g.b_cols = ldw;
        g.nbatch = R; g.alpha = 1.0; g.beta = accumulate ? 1.0 : 0.0; g.tri = 0;
        if (int rc = pgl_launch_gemm(PGL_GEMM_PLAIN, g, st)) return rc;
    }
    return PGL_OK;
}

}  // namespace

size_t pgl_lagged_work_bytes(int N, int K, int R, int rows) {
    if (N <= 0 || K <= 0 || K > PGL_LAG_MAX || R <= 0 || rows <= 0) return 0;
    const size_t i8 = (size_t)R * lag_np16(N) * (size_t)lag_row_bytes(K, rows);
    const size_t f64 = (size_t)R * ((size_t)K - 1 + rows + 16) * (size_t)((N + 1) & ~1) * 8;
    return ((i8 > f64 ? i8 : f64) + 15) & ~(size_t)15;
}

int pgl_lagged_products(const double* Y, long ldy, long strideY, int rows, int prev, int N, int K, int R, double* S, long strideS, int accumulate,
                        int mode, void* work, int* status, void* hip_stream) {
    PGL_CHECK_ARG(Y && S && work && status && rows > 0 && N > 0 && R > 0 && K >= 1 && K <= PGL_LAG_MAX && prev >= 0 && prev <= K - 1);
    PGL_CHECK_ARG(ldy >= N && strideS >= (long)K * N * N && (mode == PGL_LAG_I8 || mode == PGL_LAG_F64) && ((uintptr_t)work % 16) == 0);
    PGL_CHECK_ARG((long)prev + rows + 16 + 2L * PGL_LAG_MAX < 0x7fffffffL);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (mode == PGL_LAG_I8) return lag_i8(Y, ldy, strideY, rows, prev, N, K, R, S, strideS, accumulate, work, status, st);
    return lag_f64(Y, ldy, strideY, rows, prev, N, K, R, S, strideS, accumulate, work, st);
}
