// What free-running simulation of a model with covariates or latent common input needs beside pgl_simulate_offset (pgl_generate.hip):
// the chunk's offset and the latents' prior paths (pyglm_amd/simulate.py states the law; include/pyglm_hip_simulate_offset.h the calls;
// DESIGN.md section 22).
//
//   sim_offset_kernel      Off[r][k][n] = offset_host([S_obs | X_r], beta)[k][n].  cov_offset_kernel's scheme (pgl_covariates.hip): one workgroup =
//                          64 rows of time of 64 columns, its slice of Beta ([K][64]) and its rows of S_obs in LDS, lane = column, the waves
//                          take the rows in turn.  The prefix over the K_obs observed columns is formed once per cell; every replicate
//                          continues it with its Q latent terms (X[r][k][:] is the same address in every lane: a broadcast load).  A rounded
//                          product and a rounded sum per term, ascending from 0.0: the host loop's bits.
//   sim_paths_kernel       X[r][k][q], the stationary AR(1) prior paths.  One workgroup per replicate walks the chunk in tiles of
//                          PATH_TILE bins: every thread draws normals of the tile into LDS (one Philox call per normal, or z_override), then
//                          lane q < Q walks the tile in time order in LDS -- the serial walk is what defines the bits --, then the workgroup
//                          stores the tile.  No atomics; nothing depends on R or on where the bins are cut into calls.
#include "pgl_common.h"
#include "pgl_rng.h"
#include "../../include/pyglm_hip_covariates.h"
#include "../../include/pyglm_hip_simulate_offset.h"

namespace {

constexpr int OFFB_TILE = 64;                                       // rows and columns of a workgroup of the offset kernel
constexpr int OFFB_WAVES = 4;
constexpr int PATH_TILE = 512;                                      // bins of a tile of the path kernel: 32 KiB of LDS at Q = 8
static_assert(PGL_SIM_LATENT_MAX <= PGL_COVARIATE_MAX, "the latent columns are columns of Beta");

__global__ __launch_bounds__(256) void sim_offset_kernel(const double* __restrict__ S, long lds, const double* __restrict__ X, long ldx_r,
                                                         const double* __restrict__ Beta, long ldn, double* __restrict__ Off, long ldo_t, long ldo_r,
                                                         int Tc, int N, int K_obs, int Q, int R) {
#pragma clang fp contract(off)                        // the product is rounded, then the sum: what offset_host does
    __shared__ double sB[PGL_COVARIATE_MAX][OFFB_TILE];
    __shared__ double sS[OFFB_TILE][PGL_COVARIATE_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)blockIdx.x * OFFB_TILE;
    const int col0 = blockIdx.y * OFFB_TILE;
    const int K = K_obs + Q;
    for (int e = tid; e < K * OFFB_TILE; e += 256) {
        const int k = e >> 6, n = col0 + (e & 63);
        sB[k][e & 63] = n < N ? Beta[(long)k * ldn + n] : 0.0;
    }
    for (int e = tid; e < OFFB_TILE * K_obs; e += 256) {
        const int row = e / K_obs, k = e - row * K_obs;
        const long t = row0 + row;
        sS[row][k] = t < Tc ? S[t * lds + k] : 0.0;
    }
    __syncthreads();
    const int n = col0 + lane;
    for (int row = wave; row < OFFB_TILE; row += OFFB_WAVES) {
        const long t = row0 + row;
        if (t >= Tc) break;
        double pre = 0.0;
        for (int k = 0; k < K_obs; ++k) pre = pre + sS[row][k] * sB[k][lane];
        for (int r = 0; r < R; ++r) {
            const double* x = Q ? X + (long)r * ldx_r + t * Q : nullptr;
            double acc = pre;
            for (int q = 0; q < Q; ++q) acc = acc + x[q] * sB[K_obs + q][lane];
            if (n < N) Off[(long)r * ldo_r + t * ldo_t + n] = acc;
        }
    }
}

struct PathArgs {
    double* X; long ldx_r;
    double* carry; const double* zo;
    double phi[PGL_SIM_LATENT_MAX], s[PGL_SIM_LATENT_MAX];
    uint64_t t0, seed; long rep0;
    int Tc, Q, has_carry;
};

__global__ __launch_bounds__(256) void sim_paths_kernel(PathArgs a) {
#pragma clang fp contract(off)                        // fl(fl(phi x) + fl(s z)): no fused multiply-add
    __shared__ double zs[PATH_TILE * PGL_SIM_LATENT_MAX];
    const int r = blockIdx.x, tid = threadIdx.x, Q = a.Q;
    double* Xr = a.X + (long)r * a.ldx_r;
    double prev = 0.0, phi = 0.0, sq = 0.0;
    bool have = a.has_carry != 0;
    if (tid < Q) {
        phi = a.phi[tid]; sq = a.s[tid];
        if (have) prev = a.carry[(long)r * Q + tid];
    }
    for (int k0 = 0; k0 < a.Tc; k0 += PATH_TILE) {
        const int rows = min(PATH_TILE, a.Tc - k0), cells = rows * Q;
        for (int e = tid; e < cells; e += 256) {                     // the normals of the tile, one thread each
            const int k = k0 + e / Q, q = e % Q;
            double z;
            if (a.zo) {
                z = a.zo[((long)r * a.Tc + k) * Q + q];
            } else {
                PglPhilox g;
                pgl_rng_init(g, a.seed, (uint64_t)(a.rep0 + r), a.t0 + (uint64_t)k, PGL_PURPOSE_SIM_LATENT);
                g.j = (uint32_t)q;                                   // call q of the (replicate, bin) stream: both of its uniforms
                z = pgl_norm(g);
            }
            zs[e] = z;
        }
        __syncthreads();
        if (tid < Q) {                                               // one lane per series, in time order
            for (int u = 0; u < rows; ++u) {
                const double z = zs[u * Q + tid];
                const double pa = phi * prev, pb = sq * z;        // (plain operators: the pragma above governs them, not a header's inlined body)
                const double x = have ? pa + pb : z;
                have = true;
                zs[u * Q + tid] = x;
                prev = x;
            }
        }
        __syncthreads();
        for (int e = tid; e < cells; e += 256) Xr[(long)k0 * Q + e] = zs[e];
        __syncthreads();                                             // the tile is stored before the next one's normals take its place
    }
    if (tid < Q) a.carry[(long)r * Q + tid] = prev;
}

}  // namespace

extern "C" int pgl_simulate_offset_build(const double* S, long lds, const double* X, long ldx_r, const double* Beta, long ldn, double* Off, long ldo_t,
                                         long ldo_r, int Tc, int N, int K_obs, int Q, int R, void* hip_stream) {
    PGL_CHECK_ARG(K_obs >= 0 && Q >= 0 && Q <= PGL_SIM_LATENT_MAX && K_obs + Q >= 1 && K_obs + Q <= PGL_COVARIATE_MAX);
    PGL_CHECK_ARG(Tc >= 1 && N >= 1 && R >= 1 && Beta && Off && ldn >= N && ldo_t >= N);
    PGL_CHECK_ARG(K_obs == 0 || (S && lds >= K_obs));
    PGL_CHECK_ARG(Q > 0 ? (X != nullptr) : (R == 1));
    PGL_CHECK_ARG(R == 1 ? ldx_r >= 0 : (ldx_r >= (long)Tc * Q && ldo_r >= (long)(Tc - 1) * ldo_t + N));
    PGL_CHECK_ARG(((long)N + OFFB_TILE - 1) / OFFB_TILE <= 65535);
    hipLaunchKernelGGL(sim_offset_kernel, dim3((unsigned)((Tc + OFFB_TILE - 1) / OFFB_TILE), (unsigned)((N + OFFB_TILE - 1) / OFFB_TILE)), dim3(256), 0,
                       static_cast<hipStream_t>(hip_stream), S, lds, X, ldx_r, Beta, ldn, Off, ldo_t, ldo_r, Tc, N, K_obs, Q, R);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}

extern "C" int pgl_latent_prior_paths(double* X, long ldx_r, int R, long rep0, uint64_t t0, int Tc, int Q, const double* phi, const double* s,
                                      double* carry, int has_carry, const double* z_override, uint64_t seed, void* hip_stream) {
    PGL_CHECK_ARG(X && phi && s && carry);
    PGL_CHECK_ARG(Q >= 1 && Q <= PGL_SIM_LATENT_MAX && R >= 1 && Tc >= 1 && rep0 >= 0 && rep0 + R <= (1L << 31) - 1);
    PGL_CHECK_ARG(has_carry == 0 || has_carry == 1);
    PGL_CHECK_ARG(ldx_r >= (long)Tc * Q);
    PathArgs a{};
    for (int q = 0; q < Q; ++q) {
        PGL_CHECK_ARG(phi[q] >= 0.0 && phi[q] < 1.0 && s[q] > 0.0 && s[q] <= 1.0);
        a.phi[q] = phi[q]; a.s[q] = s[q];
    }
    a.X = X; a.ldx_r = ldx_r; a.carry = carry; a.zo = z_override; a.t0 = t0; a.seed = seed; a.rep0 = rep0; a.Tc = Tc; a.Q = Q; a.has_carry = has_carry;
    hipLaunchKernelGGL(sim_paths_kernel, dim3((unsigned)R), dim3(256), 0, static_cast<hipStream_t>(hip_stream), a);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}
