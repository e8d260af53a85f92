// Forward simulation of the population model (reference pyglm/models.py:98-151, generate): Tc bins per launch, serial in t.
//
// Per bin t:  x_t[m, :] = sum_l Y[t-1-l, m] basis[l, :]   (the basis-filtered history of presynaptic neuron m)
//             psi_t[n]  = Wm[n, :] . x_t + bias[n]          (Wm = the stored W as N x N*B, not a*W, as the reference)
//             y_t[n]    = u < 1 / (1 + exp(-psi))  (Bernoulli)   or   psi + s * g  (Gaussian, s = sqrt(eta) formed by the caller)
// with u / g the caller's host draws for the bin (NumPy's legacy stream, row-major (Tc, N)), so the trajectory is the host loop's.
//
// Decomposition: workgroup k owns neurons [k*npw, (k+1)*npw) for both roles -- it computes their psi (one wave per neuron, or lanes in
// groups of lpn per neuron when a workgroup owns more neurons than it has waves) and keeps their history: the ring of the last L rows of
// Y (row t mod L = Y[t]) is read and written by the owning workgroup only, and carries the state from one launch to the next.  After
// drawing y_t a workgroup writes its slice of x_{t+1} into one of two exchange buffers (by the parity of t+1) and the grid meets at
// ONE barrier per bin; every workgroup then reads the whole x_{t+1}.  Two buffers suffice: x_{t+2} goes into the buffer x_t came from,
// and no workgroup writes it before every workgroup has passed the barrier of bin t+1, i.e. finished reading x_t.
//
// The barrier is XCD-hierarchical (workgroups labelled by blockIdx % 8: the label only picks which counter a workgroup arrives at, so
// placement changes speed, never results): agent-scope release fence, relaxed arrival on the label's counter; the last arriver of a
// label (acquire + release) arrives at the top counter; the last of those (acquire + release) stores the generation; every workgroup
// polls the generation relaxed with s_sleep and takes ONE agent-scope acquire.  Counters are monotonic within the launch (epoch =
// barrier index + 1) and zeroed by a memset ahead of every launch.  Every spin is bounded: a barrier that has not completed after
// `spin_ticks` of the wall clock, or that sees another workgroup's failure, sets the status word {1, bin} and the kernel exits.
// Residency: the grid is <= one workgroup per CU and launched cooperatively (the runtime checks it).  A model with N*N*B <=
// PGL_GEN_ONE_WG_MAX runs as ONE workgroup: no grid barrier, the bins are separated by the workgroup barrier alone.
#include "pgl_common.h"
#include "../../include/pyglm_hip.h"
#include <algorithm>

namespace {

constexpr int GEN_THREADS = 256;
constexpr int GEN_WAVES = GEN_THREADS / 64;
constexpr long PGL_GEN_ONE_WG_MAX = 1L << 14;      // N*N*B of the one-workgroup variant
constexpr int GEN_XLDS_MAX = 8192;                  // N*B up to which x_t is staged in LDS (64 KiB)
constexpr int GEN_BAR_BYTES = 1024;                 // barrier block at the head of the work buffer: 10 words, one per 64-byte line
constexpr int BAR_STRIDE = 16;                      // words between counters
constexpr int BAR_TOP = 8, BAR_GEN = 9;
constexpr size_t GEN_RING_LDS_MAX = 32 * 1024;       // the workgroup's ring in LDS up to this size
constexpr size_t GEN_BASIS_LDS_MAX = 16 * 1024;      // the basis in LDS up to this size
constexpr int GEN_KR = 80;                          // elements of Wm per lane held in registers

struct GenArgs {
    const double* Wm; const double* bias; const double* basis;
    const double* U; double* ring; double* Y;
    double* xbuf;            // [2][N*B]
    unsigned* bar;           // barrier words
    int* status;             // [2]: code, bin
    long t0; int Tc, N, B, L, obs; double scale;
    int npw, lpn, lpp;       // neurons per workgroup; lanes per neuron in the dot products, per (neuron, basis function) in the
                             // history sums (powers of 2, <= 64)
    int ring_off, basis_off; // byte offsets of the ring / the basis in LDS (0: read from global memory)
    unsigned long long spin_ticks;
};

__device__ __forceinline__ void fail(int* status, long bin) {
    int expect = 0;
    if (__hip_atomic_compare_exchange_strong(status, &expect, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_store(status + 1, (int)bin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// every wave of the workgroup calls this; returns false (uniformly) if the barrier failed
__device__ bool grid_sync(const GenArgs& g, unsigned epoch, long bin, int* ok_lds) {
    if (gridDim.x == 1) {                                              // one workgroup: x is in LDS, and a ring in global memory was
        __syncthreads();                                               // drained before the history sums
        return true;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // every storing wave drains its stores of x
    __syncthreads();
    if (threadIdx.x == 0) {
        const int G = gridDim.x, lab = blockIdx.x & 7, nlab = G < 8 ? G : 8;
        const unsigned lsize = (unsigned)((G - lab + 7) / 8);
        unsigned* bar = g.bar;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned a = __hip_atomic_fetch_add(bar + lab * BAR_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a + 1 == lsize * epoch) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned b = __hip_atomic_fetch_add(bar + BAR_TOP * BAR_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b + 1 == (unsigned)nlab * epoch) {
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(bar + BAR_GEN * BAR_STRIDE, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        int ok = 1;
        const unsigned long long start = wall_clock64();
        for (unsigned spins = 0; __hip_atomic_load(bar + BAR_GEN * BAR_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < epoch; ++spins) {
            if ((spins & 63) == 63 &&
                (__hip_atomic_load(g.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 || wall_clock64() - start > g.spin_ticks)) {
                fail(g.status, bin);
                ok = 0;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        *ok_lds = ok;
    }
    __syncthreads();
    return *ok_lds != 0;
}

// x_{tl+1}[m, :] for the workgroup's neurons m, from ring rows tl, tl-1, ..., tl-L+1 (rows of negative times are the ring's zeros) into
// out[m*B + b] (the exchange buffer, or x_t in LDS when one workgroup runs the model).  Each (m, b) is a sum over L, split over lpp lanes
// and added up by shuffles.  The ring (and the basis) are read from LDS when they fit there (rl / sb non-null), else from global memory.
__device__ void own_history(const GenArgs& g, long tl, int n_lo, int nown, const double* rl, const double* sb, double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lpp = g.lpp, gpw = 64 / lpp, grp = lane / lpp, gl = lane % lpp;
    const int P = nown * g.B, L = g.L;
    int r_top = (int)(tl % L);
    if (r_top < 0) r_top += L;
    for (int r0 = 0; r0 < P; r0 += GEN_WAVES * gpw) {                 // wave-uniform trip count
        const int p = r0 + wave * gpw + grp;
        double acc = 0.0;
        if (p < P) {
            const int ml = p / g.B, b = p % g.B;
            for (int l = gl; l < L; l += lpp) {
                int row = r_top - l;
                if (row < 0) row += L;
                const double y = rl ? rl[row * nown + ml] : g.ring[(long)row * g.N + n_lo + ml];
                acc = fma(y, sb ? sb[l * g.B + b] : g.basis[l * g.B + b], acc);
            }
        }
        for (int off = lpp >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (p < P && gl == 0) out[(n_lo + p / g.B) * g.B + p % g.B] = acc;
    }
}

// KR > 0: every lane keeps its <= KR elements of its neuron's row of Wm in registers for the whole launch (the workgroup's rows are read
// from memory once per launch, not once per bin); KR = 0: the rows stream from memory every bin.  XLDS: x_t is read from LDS.
template <bool XLDS, int KR>
__global__ __launch_bounds__(GEN_THREADS) void generate_kernel(GenArgs g) {
    // dynamic LDS: [16 B: barrier verdict][x_t: N*B (XLDS)][ring: L x npw (ring_off > 0)][basis: L x B (basis_off > 0)], 16-byte aligned
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* ok_lds = reinterpret_cast<int*>(smem);
    double* xs = reinterpret_cast<double*>(smem + 16);
    double* rl = g.ring_off ? reinterpret_cast<double*>(smem + g.ring_off) : nullptr;
    double* sb = g.basis_off ? reinterpret_cast<double*>(smem + g.basis_off) : nullptr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_lo = blockIdx.x * g.npw;
    const int nown = min(g.N, n_lo + g.npw) - n_lo;
    const int NB = g.N * g.B, L = g.L;
    const int lpn = g.lpn, gpw = 64 / lpn, grp = lane / lpn, gl = lane % lpn;
    const bool direct = XLDS && gridDim.x == 1;                      // one workgroup: x goes straight into LDS, no exchange buffer
    unsigned epoch = 0;

    if (rl)
        for (int e = threadIdx.x; e < L * nown; e += GEN_THREADS) rl[e] = g.ring[(long)(e / nown) * g.N + n_lo + e % nown];
    if (sb)
        for (int e = threadIdx.x; e < L * g.B; e += GEN_THREADS) sb[e] = g.basis[e];
    double wr[KR > 0 ? KR : 1];
    if (KR > 0) {                                                    // (the host picks KR only with one neuron per wave)
        const int i = wave * gpw + grp;
        const double* w = g.Wm + (long)(n_lo + (i < nown ? i : 0)) * NB;
#pragma unroll
        for (int q = 0; q < (KR > 0 ? KR : 1); ++q) wr[q] = (i < nown && gl + q * 64 < NB) ? w[gl + q * 64] : 0.0;
        for (int j = NB + threadIdx.x; j < KR * 64; j += GEN_THREADS) xs[j] = 0.0;
    }
    __syncthreads();

    // one round of neurons per wave (every lane keeps its neuron): its bias and the next bin's draw are loaded ahead of time
    const bool one_round = nown <= GEN_WAVES * gpw;
    const int i1 = wave * gpw + grp;
    const bool mine1 = one_round && i1 < nown && gl == 0;
    const double bias1 = mine1 ? g.bias[n_lo + i1] : 0.0;
    double v_next = mine1 ? g.U[n_lo + i1] : 0.0;
    own_history(g, g.t0 - 1, n_lo, nown, rl, sb, direct ? xs : g.xbuf + (g.t0 & 1) * (long)NB);      // x_{t0} from the ring
    if (!grid_sync(g, ++epoch, g.t0, ok_lds)) return;
    for (int k = 0; k < g.Tc; ++k) {
        const long t = g.t0 + k;
        const double* x = g.xbuf + (t & 1) * (long)NB;
        if (XLDS && !direct) {
            int j = threadIdx.x;
            for (; j + 7 * GEN_THREADS < NB; j += 8 * GEN_THREADS) {
                double v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = x[j + q * GEN_THREADS];
#pragma unroll
                for (int q = 0; q < 8; ++q) xs[j + q * GEN_THREADS] = v[q];
            }
            for (; j < NB; j += GEN_THREADS) xs[j] = x[j];
            __syncthreads();
        }
        for (int r0 = 0; r0 < nown; r0 += GEN_WAVES * gpw) {         // wave-uniform trip count: the shuffles below see every lane
            const int i = r0 + wave * gpw + grp;
            const bool mine = i < nown && gl == 0;
            const double v = one_round ? v_next : mine ? g.U[(long)k * g.N + n_lo + i] : 0.0;     // issued ahead of the dot product
            if (mine1 && k + 1 < g.Tc) v_next = g.U[(long)(k + 1) * g.N + n_lo + i1];
            double acc = 0.0;
            if (i < nown) {
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
                if (KR > 0) {                                        // lpn = 64; xs is zero beyond N*B up to KR*64
#pragma unroll
                    for (int q = 0; q < (KR > 0 ? KR : 1); q += 4) {
                        a0 = fma(wr[q], xs[gl + q * 64], a0);
                        if (q + 1 < KR) a1 = fma(wr[q + 1], xs[gl + (q + 1) * 64], a1);
                        if (q + 2 < KR) a2 = fma(wr[q + 2], xs[gl + (q + 2) * 64], a2);
                        if (q + 3 < KR) a3 = fma(wr[q + 3], xs[gl + (q + 3) * 64], a3);
                    }
                } else {
                    const double* w = g.Wm + (long)(n_lo + i) * NB;
                    int j = gl;
                    for (; j + 7 * lpn < NB; j += 8 * lpn) {
                        double wv[8], xv[8];
#pragma unroll
                        for (int q = 0; q < 8; ++q) wv[q] = w[j + q * lpn];
#pragma unroll
                        for (int q = 0; q < 8; ++q) xv[q] = XLDS ? xs[j + q * lpn] : x[j + q * lpn];
                        a0 = fma(wv[0], xv[0], a0); a1 = fma(wv[1], xv[1], a1); a2 = fma(wv[2], xv[2], a2); a3 = fma(wv[3], xv[3], a3);
                        a0 = fma(wv[4], xv[4], a0); a1 = fma(wv[5], xv[5], a1); a2 = fma(wv[6], xv[6], a2); a3 = fma(wv[7], xv[7], a3);
                    }
                    for (; j < NB; j += lpn) a0 = fma(w[j], XLDS ? xs[j] : x[j], a0);
                }
                acc = (a0 + a1) + (a2 + a3);
            }
            for (int off = lpn >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
            if (mine) {
                const int n = n_lo + i;
                const double psi = acc + (one_round ? bias1 : g.bias[n]);
                double y;
                if (g.obs == 0) y = v < 1.0 / (1.0 + exp(-psi)) ? 1.0 : 0.0;
                else y = __dadd_rn(psi, __dmul_rn(g.scale, v));
                g.Y[(long)k * g.N + n] = y;
                const int row = (int)(t % L);
                if (rl) rl[row * nown + i] = y;
                else g.ring[(long)row * g.N + n] = y;
            }
        }
        if (k + 1 == g.Tc) break;
        if (!rl) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (a ring in global memory: this bin's row before it is read)
        __syncthreads();                                              // this bin's ring row is complete, and x_t is no longer read
        own_history(g, t, n_lo, nown, rl, sb, direct ? xs : g.xbuf + ((t + 1) & 1) * (long)NB);
        if (!grid_sync(g, ++epoch, t + 1, ok_lds)) return;
    }
    if (rl) {                                                         // the ring goes back for the next launch
        __syncthreads();
        for (int e = threadIdx.x; e < L * nown; e += GEN_THREADS) g.ring[(long)(e / nown) * g.N + n_lo + e % nown] = rl[e];
    }
}

struct GenGeometry { int G, npw, lpn, lpp; };

GenGeometry geometry(int N, int B) {
    GenGeometry q;
    if ((long)N * N * B <= PGL_GEN_ONE_WG_MAX) q.G = 1;
    else q.G = std::min(pgl_device_cus(pgl_device()), (N + 3) / 4);
    q.npw = (N + q.G - 1) / q.G;
    q.G = (N + q.npw - 1) / q.npw;                                     // no workgroup without neurons
    int per_wave = (q.npw + GEN_WAVES - 1) / GEN_WAVES, gpw = 1;
    while (gpw < per_wave && gpw < 64) gpw *= 2;
    q.lpn = 64 / gpw;
    // lanes per (neuron, basis function) sum of the history: as many as leave every pair of the workgroup a group in one round
    const int pairs = q.npw * B;
    q.lpp = 64;
    while (q.lpp > 1 && pairs * q.lpp > GEN_THREADS) q.lpp /= 2;
    return q;
}

template <bool XLDS, int KR>
int launch(const GenArgs& a, int G, size_t lds, hipStream_t st) {
    static PglPerDeviceSize lds_set;
    int rc = pgl_grow_dynamic_lds(reinterpret_cast<const void*>(&generate_kernel<XLDS, KR>), lds, lds_set);
    if (rc) return rc;
    void* args[] = {const_cast<GenArgs*>(&a)};
    hipError_t e = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(&generate_kernel<XLDS, KR>), dim3(G), dim3(GEN_THREADS), args, lds, st);
    if (e != hipSuccess) { pgl_set_error("pgl_generate: cooperative launch of %d workgroups: %s", G, hipGetErrorString(e)); return PGL_ERR_HIP; }
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}

}  // namespace

extern "C" size_t pgl_generate_work_bytes(int N, int B) {
    if (N <= 0 || B <= 0) return 0;
    return GEN_BAR_BYTES + 2 * (size_t)N * B * sizeof(double);
}

extern "C" int pgl_generate(const double* Wm, const double* bias, const double* basis, int N, int B, int L, int obs, double noise_scale,
                            const double* U, double* ring, double* Y, long t0, int Tc, void* work, int* status, void* hip_stream) {
    PGL_CHECK_ARG(Wm && bias && basis && U && ring && Y && work && status);
    PGL_CHECK_ARG(N > 0 && B > 0 && L > 0 && Tc > 0 && t0 >= 0 && (obs == 0 || obs == 1));
    PGL_CHECK_ARG((long)N * B <= (1L << 30) && (long)L * N <= (1L << 31) - 1);
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    const GenGeometry q = geometry(N, B);
    const int dev = pgl_device();
    static std::atomic<long long> tick_khz[PGL_MAX_DEVICES];
    long long khz = tick_khz[dev & (PGL_MAX_DEVICES - 1)].load(std::memory_order_relaxed);
    if (khz <= 0) {
        int r = 0;
        if (hipDeviceGetAttribute(&r, hipDeviceAttributeWallClockRate, dev) != hipSuccess || r <= 0) r = 100000;
        khz = r;
        tick_khz[dev & (PGL_MAX_DEVICES - 1)].store(khz, std::memory_order_relaxed);
    }
    const int NB = N * B;
    const bool xlds = NB <= GEN_XLDS_MAX;
    auto al16 = [](size_t x) { return (x + 15) / 16 * 16; };
    // registers for the rows of Wm: one neuron per wave (npw <= 4, 64 lanes per neuron) and at most GEN_KR elements per lane; x_t is then
    // read as GEN_KR * 64 elements of which those beyond N*B are zero
    const bool regs = xlds && q.npw <= GEN_WAVES && q.lpn == 64 && NB <= GEN_KR * 64;
    size_t lds = 16 + (xlds ? al16((size_t)(regs ? GEN_KR * 64 : NB) * sizeof(double)) : 0);
    GenArgs a{};
    if ((size_t)L * q.npw * sizeof(double) <= GEN_RING_LDS_MAX) { a.ring_off = (int)lds; lds += al16((size_t)L * q.npw * sizeof(double)); }
    if ((size_t)L * B * sizeof(double) <= GEN_BASIS_LDS_MAX) { a.basis_off = (int)lds; lds += al16((size_t)L * B * sizeof(double)); }
    a.Wm = Wm; a.bias = bias; a.basis = basis; a.U = U; a.ring = ring; a.Y = Y;
    a.bar = static_cast<unsigned*>(work);
    a.xbuf = reinterpret_cast<double*>(static_cast<char*>(work) + GEN_BAR_BYTES);
    a.status = status;
    a.t0 = t0; a.Tc = Tc; a.N = N; a.B = B; a.L = L; a.obs = obs; a.scale = noise_scale;
    a.npw = q.npw; a.lpn = q.lpn; a.lpp = q.lpp;
    a.spin_ticks = (unsigned long long)khz * 2000ULL;                 // 2 s of the wall clock per barrier
    hipError_t e = hipMemsetAsync(work, 0, GEN_BAR_BYTES, st);
    if (e != hipSuccess) { pgl_set_error("pgl_generate: hipMemsetAsync: %s", hipGetErrorString(e)); return PGL_ERR_HIP; }
    if (regs) return launch<true, GEN_KR>(a, q.G, lds, st);
    if (xlds) return launch<true, 0>(a, q.G, lds, st);
    return launch<false, 0>(a, q.G, lds, st);
}
