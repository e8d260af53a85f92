// Latent common input (pyglm_amd/latents.py states the law; include/pyglm_hip_latents.h the calls): a data set's
// S = [S_obs | X] carries Q latent columns whose values are sampled, x_t | omega, W, b, beta for every time bin t.
//
//   lat_fold_kernel<Q, LDS>  Lambda_t (lower triangle) and r_t.  Where the covariate fold reduces over time per neuron (lane = column), this
//                            one reduces over NEURONS per time bin: the contiguous axis of Psi, Omega and Kappa.  One wavefront owns a bin;
//                            lane l walks columns l, l + 64, ... in ascending order, LAT_UNROLL columns' loads in flight, and holds the
//                            bin's Q (Q + 1) / 2 + Q sums in registers.  The loadings C_n and the bias come from LDS, staged once per
//                            workgroup as [q][column] (LDS = true: nloc <= PGL_LATENT_LDS_COLS), or from Beta and bias through the caches
//                            (LDS = false) -- the same operations in the same order.  The workgroup's 4 waves take bins in a grid stride.
//   lat_tree                 joins the 64 lanes' sums in a fixed order: __shfl_xor at distances 32, 16, 8, 4, 2, 1.  While a lane holds more
//                            than one sum a step HALVES what it holds -- the lane keeps one half of the sums and hands the other half to
//                            its partner, which keeps that one -- so 63 values cross lanes per bin at Q = 8 instead of 44 x 6; lane i ends
//                            with sum i and writes it.
//   lat_draw_kernel<Q>       one thread per bin, the Q x Q system in registers: Cholesky of I + Lambda_t, forward solve, add z (the Philox
//                            stream, or z_override), backward solve; the bin's Q latent cells of S are all it writes.
// No floating-point atomics: a bin's sums depend on nloc alone -- not on T, on the bins that share its workgroup or on the launch geometry.
#include "pgl_common.h"
#include "pgl_rng.h"
#include "../../include/pyglm_hip_latents.h"

namespace {

constexpr int LAT_WAVES = 4;
constexpr int LAT_UNROLL = 4;                                       // columns of a lane whose loads are in flight together, at most
constexpr int LAT_STEP = 64 * LAT_UNROLL;                           // the staged columns are padded to a multiple of this
static_assert(PGL_LATENT_LDS_COLS % LAT_STEP == 0, "the staged columns are whole trips");
static_assert((PGL_LATENT_MAX + 1) * PGL_LATENT_LDS_COLS * 8 * 2 <= 160 * 1024, "two workgroups' loadings fit a CU's LDS");

struct LatArgs {
    const double *Psi, *bias, *Omega, *Kappa, *S, *Beta;
    long ldn, ldo, ldk, lds, ldb;
    int col0, T, nloc, npad;                                        // npad: nloc rounded up to whole trips (the staged columns)
    double *Lambda, *r;
};

// a[0 .. NS) of every lane -> the sums over the 64 lanes; returns in `idx` which sum this lane's a[0] holds afterwards (idx >= NS: none) and
// whether the lane is the one that writes it.  Lower lane + upper lane at every step.
template <int NS, int H, int MASK>                                  // one halving step: slots [0, 2 H) are held, [0, H) stay
__device__ __forceinline__ void lat_tree_halve(double (&a)[NS], int lane) {
    if constexpr (H >= 1) {
        const bool up = (lane & MASK) != 0;
#pragma unroll
        for (int i = 0; i < (H < NS ? H : NS); ++i) {
            if (i + H < NS) {
                double lo = a[i], hi = a[i + H];
                asm volatile("" : "+v"(lo), "+v"(hi));            // (values, not addresses, are selected: the sums stay in registers)
                const double keep = up ? hi : lo;
                const double send = up ? lo : hi;
                a[i] = keep + __shfl_xor(send, MASK);
            } else {
                a[i] = a[i] + __shfl_xor(a[i], MASK);              // (the upper lanes' result stands for a sum that does not exist)
            }
        }
        lat_tree_halve<NS, H / 2, MASK / 2>(a, lane);
    }
}

template <int NS>
__device__ __forceinline__ bool lat_tree(double (&a)[NS], int lane, int& idx) {
    constexpr int K = NS <= 1 ? 0 : NS <= 2 ? 1 : NS <= 4 ? 2 : NS <= 8 ? 3 : NS <= 16 ? 4 : NS <= 32 ? 5 : 6;
    static_assert(NS >= 1 && NS <= 64, "a lane ends with at most one sum");
    lat_tree_halve<NS, (1 << K) / 2, 32>(a, lane);
#pragma unroll
    for (int mask = 32 >> K; mask > 0; mask >>= 1) a[0] = a[0] + __shfl_xor(a[0], mask);
    idx = lane >> (6 - K);
    return (lane & ((1 << (6 - K)) - 1)) == 0 && idx < NS;
}

template <int Q, bool LDS>
__global__ __launch_bounds__(256) void lat_fold_kernel(LatArgs a) {
    constexpr int P = Q * (Q + 1) / 2, NS = P + Q;
    constexpr int U = Q <= 4 ? LAT_UNROLL : 2;                      // (4 columns of 44 sums' operands do not fit the registers: 2 from Q = 5 on)
    extern __shared__ __attribute__((aligned(16))) double sm[];     // [Q + 1][npad]: the loadings, then the bias; zero from nloc on
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (LDS) {
        for (int e = tid; e < (Q + 1) * a.npad; e += 256) {
            const int q = e / a.npad, n = e - q * a.npad;
            double v = 0.0;
            if (n < a.nloc) v = q < Q ? a.Beta[(long)(a.col0 + q) * a.ldb + n] : (a.bias ? a.bias[n] : 0.0);
            sm[e] = v;
        }
        __syncthreads();
    }
    for (long t = (long)blockIdx.x * LAT_WAVES + wave; t < a.T; t += (long)gridDim.x * LAT_WAVES) {      // (the wave's: every lane makes the same trips)
        double x[Q], acc[NS];
#pragma unroll
        for (int q = 0; q < Q; ++q) x[q] = a.S[t * a.lds + a.col0 + q];
#pragma unroll
        for (int i = 0; i < NS; ++i) acc[i] = 0.0;
        const double* om = a.Omega + t * a.ldo;
        const double* kp = a.Kappa + t * a.ldk;
        const double* ps = a.Psi + t * a.ldn;
        for (int n0 = 0; n0 < a.nloc; n0 += 64 * U) {
            double w[U], kk[U], pp[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int n = n0 + u * 64 + lane;
                const bool in = n < a.nloc;                         // a column past the last one is not read and adds exact zeros
                w[u] = in ? om[n] : 0.0;
                kk[u] = in ? kp[n] : 0.0;
                pp[u] = in ? ps[n] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int n = n0 + u * 64 + lane;
                double c[Q], bn;
                if (LDS) {
#pragma unroll
                    for (int q = 0; q < Q; ++q) c[q] = sm[q * a.npad + n];
                    bn = sm[Q * a.npad + n];
                } else {
                    const bool in = n < a.nloc;
#pragma unroll
                    for (int q = 0; q < Q; ++q) c[q] = in ? a.Beta[(long)(a.col0 + q) * a.ldb + n] : 0.0;
                    bn = (in && a.bias) ? a.bias[n] : 0.0;
                }
                double o = 0.0;
#pragma unroll
                for (int q = 0; q < Q; ++q) o += x[q] * c[q];
                const double cc = kk[u] + w[u] * (o - (pp[u] + bn));
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    const double wj = w[u] * c[j];
#pragma unroll
                    for (int k = 0; k < Q; ++k) {
                        if (k > j) continue;                        // (a fixed trip count: the loop unrolls and the sums stay in registers)
                        acc[j * (j + 1) / 2 + k] += wj * c[k];
                    }
                }
#pragma unroll
                for (int q = 0; q < Q; ++q) acc[P + q] += c[q] * cc;
            }
        }
        int idx;
        if (lat_tree<NS>(acc, lane, idx)) {
            if (idx < P) a.Lambda[t * P + idx] = acc[0];
            else a.r[t * Q + (idx - P)] = acc[0];
        }
    }
}

template <int Q>
__global__ __launch_bounds__(256) void lat_draw_kernel(const double* __restrict__ Lambda, const double* __restrict__ r, const double* __restrict__ zo,
                                                       uint64_t seed, uint64_t sweep, uint64_t elem0, double* __restrict__ S, long lds, int col0,
                                                       int* __restrict__ status, int T) {
    constexpr int P = Q * (Q + 1) / 2;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    double A[P], x[Q];                                              // A: the lower triangle row by row, entry (j, k) at j (j + 1) / 2 + k
#pragma unroll
    for (int i = 0; i < P; ++i) A[i] = Lambda[t * P + i];
#pragma unroll
    for (int j = 0; j < Q; ++j) { A[j * (j + 1) / 2 + j] += 1.0; x[j] = r[t * Q + j]; }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < Q; ++j) {                                   // A = L L', row by row
#pragma unroll
        for (int k = 0; k <= j; ++k) {
            double s = A[j * (j + 1) / 2 + k];
#pragma unroll
            for (int m = 0; m < k; ++m) s -= A[j * (j + 1) / 2 + m] * A[k * (k + 1) / 2 + m];
            if (k == j) {
                if (!(s > 0.0)) { bad = true; s = 1.0; }
                A[j * (j + 1) / 2 + j] = sqrt(s);
            } else {
                A[j * (j + 1) / 2 + k] = s / A[k * (k + 1) / 2 + k];
            }
        }
    }
    if (bad) { atomicOr(status, 1); return; }
#pragma unroll
    for (int j = 0; j < Q; ++j) {                                   // y = L^-1 r
        double s = x[j];
#pragma unroll
        for (int m = 0; m < j; ++m) s -= A[j * (j + 1) / 2 + m] * x[m];
        x[j] = s / A[j * (j + 1) / 2 + j];
    }
    if (zo) {
#pragma unroll
        for (int q = 0; q < Q; ++q) x[q] += zo[t * Q + q];
    } else {
        PglPhilox g;
        pgl_rng_init(g, seed, sweep, elem0 + (uint64_t)t, PGL_PURPOSE_LATENT);
#pragma unroll
        for (int q = 0; q < Q; ++q) x[q] += pgl_norm(g);            // call q of the generator: both of its uniforms
    }
#pragma unroll
    for (int j = Q - 1; j >= 0; --j) {                              // x = L^-T (y + z)
        double s = x[j];
#pragma unroll
        for (int m = j + 1; m < Q; ++m) s -= A[m * (m + 1) / 2 + j] * x[m];
        x[j] = s / A[j * (j + 1) / 2 + j];
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) S[t * lds + col0 + q] = x[q];
}

PglPerDeviceSize lat_lds_have[PGL_LATENT_MAX];

template <int Q>
int lat_fold_launch(const LatArgs& a, hipStream_t st) {
    const int cus = pgl_device_cus(pgl_device());
    const long want = ((long)a.T + LAT_WAVES - 1) / LAT_WAVES;
    if (a.nloc <= PGL_LATENT_LDS_COLS) {
        const size_t bytes = (size_t)(Q + 1) * a.npad * sizeof(double);
        const int rc = pgl_grow_dynamic_lds(reinterpret_cast<const void*>(&lat_fold_kernel<Q, true>), bytes, lat_lds_have[Q - 1]);
        if (rc != PGL_OK) return rc;
        long per_cu = (160 * 1024) / (long)bytes;
        per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
        const long grid = want < per_cu * cus ? want : per_cu * cus;
        hipLaunchKernelGGL((lat_fold_kernel<Q, true>), dim3((unsigned)grid), dim3(256), bytes, st, a);
    } else {
        const long grid = want < 8L * cus ? want : 8L * cus;
        hipLaunchKernelGGL((lat_fold_kernel<Q, false>), dim3((unsigned)grid), dim3(256), 0, st, a);
    }
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}

}  // namespace

extern "C" int pgl_latent_max(void) { return PGL_LATENT_MAX; }

extern "C" int pgl_latent_fold(const double* Psi, long ldn, const double* bias, const double* Omega, long ldo, const double* Kappa, long ldk,
                               const double* S, long lds, int col0, const double* Beta, long ldb, int T, int nloc, int Q, double* Lambda, double* r,
                               void* hip_stream) {
    PGL_CHECK_ARG(Q >= 1 && Q <= PGL_LATENT_MAX && nloc >= 1 && T >= 0 && col0 >= 0);
    PGL_CHECK_ARG(ldn >= nloc && ldo >= nloc && ldk >= nloc && ldb >= nloc && lds >= (long)col0 + Q && Beta && Lambda && r);
    PGL_CHECK_ARG(T == 0 || (Psi && Omega && Kappa && S));
    PGL_CHECK_ARG((long)nloc + LAT_STEP <= 2147483647L);
    if (T == 0) return PGL_OK;
    LatArgs a;
    a.Psi = Psi; a.bias = bias; a.Omega = Omega; a.Kappa = Kappa; a.S = S; a.Beta = Beta;
    a.ldn = ldn; a.ldo = ldo; a.ldk = ldk; a.lds = lds; a.ldb = ldb;
    a.col0 = col0; a.T = T; a.nloc = nloc; a.npad = (nloc + LAT_STEP - 1) / LAT_STEP * LAT_STEP;
    a.Lambda = Lambda; a.r = r;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    switch (Q) {
        case 1: return lat_fold_launch<1>(a, st);
        case 2: return lat_fold_launch<2>(a, st);
        case 3: return lat_fold_launch<3>(a, st);
        case 4: return lat_fold_launch<4>(a, st);
        case 5: return lat_fold_launch<5>(a, st);
        case 6: return lat_fold_launch<6>(a, st);
        case 7: return lat_fold_launch<7>(a, st);
        default: return lat_fold_launch<8>(a, st);
    }
}

extern "C" int pgl_latent_draw(const double* Lambda, const double* r, const double* z_override, uint64_t seed, uint64_t sweep, uint64_t elem0,
                               double* S, long lds, int col0, int* status, int T, int Q, void* hip_stream) {
    PGL_CHECK_ARG(Q >= 1 && Q <= PGL_LATENT_MAX && T >= 0 && col0 >= 0 && lds >= (long)col0 + Q && status);
    PGL_CHECK_ARG(T == 0 || (Lambda && r && S));
    if (T == 0) return PGL_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const dim3 grid((unsigned)(((long)T + 255) / 256)), block(256);
#define PGL_LAT_DRAW(q) \
    case q: hipLaunchKernelGGL(lat_draw_kernel<q>, grid, block, 0, st, Lambda, r, z_override, seed, sweep, elem0, S, lds, col0, status, T); break
    switch (Q) {
        PGL_LAT_DRAW(1); PGL_LAT_DRAW(2); PGL_LAT_DRAW(3); PGL_LAT_DRAW(4); PGL_LAT_DRAW(5); PGL_LAT_DRAW(6); PGL_LAT_DRAW(7);
        default: hipLaunchKernelGGL(lat_draw_kernel<8>, grid, block, 0, st, Lambda, r, z_override, seed, sweep, elem0, S, lds, col0, status, T);
    }
#undef PGL_LAT_DRAW
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}
