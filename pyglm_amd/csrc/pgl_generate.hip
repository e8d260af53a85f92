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
//
// Two kernels run this scheme, built from ONE set of pieces (history, row_dot, stage_x, wg_begin / wg_end, grid_sync; geometry, plan and
// launch on the host), so the orders of addition that fix a trajectory's bits exist once: generate_kernel, one trajectory on the caller's
// draws (pgl_generate), and simulate_kernel, R trajectories of the fitted model on the device's own stream (pgl_simulate, THE LAW below).
// A kernel owns its bin loop and its draw.  For simulate_kernel a workgroup owns its neurons for EVERY replicate -- their ring rows
// [R][L][N], their draws, their running sums of y and y^2, added by the owning lane in time order and carried in `sum` / `sumsq` from
// launch to launch: no atomics -- and all R replicates meet at the ONE grid barrier per bin: the exchange buffer is [2][R][N*B].  Within a
// bin the replicates are independent: with the rows of Wm in registers (N*B <= GEN_KR * 64) x_{r+1} is fetched into registers while the
// dot products of x_r run out of LDS (two LDS buffers, one workgroup barrier per replicate).
// simulate_kernel also runs under a time-parallel offset (pgl_simulate_offset, include/pyglm_hip_simulate_offset.h: the covariates' and latents'
// S beta of a model that has them), a template parameter that leaves the instances without an offset as they are.
// A third kernel, conditional_kernel (pgl_conditional_simulate), is the one-workgroup form of the scheme run once per replicate on the free
// neurons of a model whose other neurons are clamped to a recording: the same pieces, and no grid barrier at all.
#include "pgl_common.h"
#include "pgl_rng.h"
#include "../../include/pyglm_hip.h"
#include "../../include/pyglm_hip_simulate_offset.h"
#include <algorithm>
#include <type_traits>

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

// ---- the pieces of a bin, written once: generate_kernel and simulate_kernel are built from these ----

typedef __attribute__((address_space(3))) const double* LdsPtr;

// x_{tl+1}[r][m, :] of the workgroup's neurons m for R replicates into out[r][m*B + b] (an exchange buffer, or x_t in LDS when ONE workgroup
// runs generate), from ring rows tl, tl-1, ..., tl-L+1 (rows of negative times are the ring's zeros).  Each (m, b) is a sum over L, split
// over lpp lanes -- lane gl adds l = gl, gl + lpp, ... in that order in ONE fma chain -- and added up by shuffles; the (replicate, neuron,
// basis function) triples are spread over the workgroup together.  The order is set by the geometry alone, not by R: a path does not
// depend on how many replicates share the launch.  ring0 / rs / rr: the workgroup's first ring row, the stride between rows and between
// replicates -- in LDS or in global memory, like bas0 (the instances keep the loads of either address space apart)
template <typename RingPtr, typename BasisPtr>
__device__ __forceinline__ void history_from(const GenArgs& g, int R, long tl, int n_lo, int nown, RingPtr ring0, int rs, long rr, BasisPtr bas0,
                                             double* out) {
    int lane = threadIdx.x & 63;
    // the lane's split and the starting values of the per-load indices below depend on the lane alone: formed here on every call, they
    // would otherwise be hoisted out of the caller's bin loop and stay in registers across its dot products (9 VGPRs, and one wave per
    // SIMD of register-limited occupancy, in generate_kernel<false, 0>)
    asm volatile("" : "+v"(lane));
    const int wave = threadIdx.x >> 6;
    const int lpp = g.lpp, gpw = 64 / lpp, grp = lane / lpp, gl = lane % lpp;
    const int P = nown * g.B, L = g.L, items = R * P;
    const long NB = (long)g.N * g.B;
    int r_top = (int)(tl % L);
    if (r_top < 0) r_top += L;
    for (int i0 = 0; i0 < items; i0 += GEN_WAVES * gpw) {               // wave-uniform trip count
        const int it = i0 + wave * gpw + grp;
        const bool on = it < items;
        const int r = on ? it / P : 0, p = on ? it % P : 0, ml = p / g.B, b = p % g.B;
        const long ro = r * rr + ml;
        double acc = 0.0;
        if (on) {
            int l = gl;
            for (; l + 3 * lpp < L; l += 4 * lpp) {                   // four loads in flight; the additions stay one chain in l
                double y[4], w[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int row = r_top - (l + q * lpp);
                    if (row < 0) row += L;
                    y[q] = ring0[ro + (long)row * rs];
                    w[q] = bas0[(l + q * lpp) * g.B + b];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) acc = fma(y[q], w[q], acc);
            }
            for (; l < L; l += lpp) {
                int row = r_top - l;
                if (row < 0) row += L;
                acc = fma(ring0[ro + (long)row * rs], bas0[l * g.B + b], acc);
            }
        }
        for (int off = lpp >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (on && gl == 0) out[(long)r * NB + (n_lo + ml) * g.B + b] = acc;
    }
}

// rl / sb: the rings [R][L][nown] / the basis in LDS, or null: read from global memory
__device__ void history(const GenArgs& g, int R, long tl, int n_lo, int nown, const double* rl, const double* sb, double* out) {
    if (rl && sb)
        history_from(g, R, tl, n_lo, nown, (LdsPtr)rl, nown, (long)g.L * nown, (LdsPtr)sb, out);
    else if (rl)
        history_from(g, R, tl, n_lo, nown, (LdsPtr)rl, nown, (long)g.L * nown, g.basis, out);
    else
        history_from(g, R, tl, n_lo, nown, (const double*)(g.ring + n_lo), g.N, (long)g.L * g.N, sb ? sb : g.basis, out);
}

// Wm[n, :] . x for the neuron of the lane's group of lpn lanes (`on`: the group has one), the sum in every lane of the group.  KR > 0: the
// row is wr[], lpn = 64 and x is readable (as zeros) beyond N*B up to KR*64; KR = 0: the row streams from w, eight loads in flight.  Four
// partial sums by the element's index mod 4*lpn, folded (a0 + a1) + (a2 + a3), then the shuffle ladder: this order is psi's bits.
template <int KR>
__device__ __forceinline__ double row_dot(const double (&wr)[KR > 0 ? KR : 1], const double* w, const double* x, int NB, int gl, int lpn, bool on) {
    double acc = 0.0;
    if (on) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (KR > 0) {
#pragma unroll
            for (int q = 0; q < (KR > 0 ? KR : 1); q += 4) {
                a0 = fma(wr[q], x[gl + q * 64], a0);
                if (q + 1 < KR) a1 = fma(wr[q + 1], x[gl + (q + 1) * 64], a1);
                if (q + 2 < KR) a2 = fma(wr[q + 2], x[gl + (q + 2) * 64], a2);
                if (q + 3 < KR) a3 = fma(wr[q + 3], x[gl + (q + 3) * 64], a3);
            }
        } else {
            int j = gl;
            for (; j + 7 * lpn < NB; j += 8 * lpn) {
                double wv[8], xv[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) wv[q] = w[j + q * lpn];
#pragma unroll
                for (int q = 0; q < 8; ++q) xv[q] = x[j + q * lpn];
                a0 = fma(wv[0], xv[0], a0); a1 = fma(wv[1], xv[1], a1); a2 = fma(wv[2], xv[2], a2); a3 = fma(wv[3], xv[3], a3);
                a0 = fma(wv[4], xv[4], a0); a1 = fma(wv[5], xv[5], a1); a2 = fma(wv[6], xv[6], a2); a3 = fma(wv[7], xv[7], a3);
            }
            for (; j < NB; j += lpn) a0 = fma(w[j], x[j], a0);
        }
        acc = (a0 + a1) + (a2 + a3);
    }
    for (int off = lpn >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    return acc;
}

// x (N*B doubles of an exchange buffer) into LDS by the whole workgroup, eight loads in flight; the caller places the barrier
__device__ __forceinline__ void stage_x(double* xs, const double* x, int NB) {
    int j = threadIdx.x;
    for (; j + 7 * GEN_THREADS < NB; j += 8 * GEN_THREADS) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = x[j + q * GEN_THREADS];
#pragma unroll
        for (int q = 0; q < 8; ++q) xs[j + q * GEN_THREADS] = v[q];
    }
    for (; j < NB; j += GEN_THREADS) xs[j] = x[j];
}

// what a thread keeps for the launch: the workgroup's dynamic LDS as the host laid it out, its neurons, the thread's place in the dot products
struct Wg {
    char* smem;              // [16 B: barrier verdict][x][rings: R x L x npw (ring_off > 0)][basis: L x B (basis_off > 0)][a kernel's own], 16-byte aligned
    int* ok_lds; double* xs; double* rl; double* sb;
    int n_lo, nown, NB;      // the workgroup owns neurons [n_lo, n_lo + nown)
    int gpw, grp, gl;        // groups of lpn lanes per wave, the lane's group, the lane within it
    // one round of neurons per wave (every lane keeps its neuron i1): its bias is loaded once
    bool one_round, mine1; int i1; double bias1;
};

// the rings of R replicates between global memory ([R][L][N]) and the workgroup's LDS ([R][L][nown])
template <bool IN>
__device__ __forceinline__ void ring_copy(const GenArgs& g, int R, const Wg& w) {
    const long ringN = (long)g.L * g.N, ringW = (long)g.L * w.nown;
    for (long e = threadIdx.x; e < R * ringW; e += GEN_THREADS) {
        const long r = e / ringW, q = e % ringW;
        double* glob = g.ring + r * ringN + (q / w.nown) * g.N + w.n_lo + q % w.nown;
        if (IN) w.rl[e] = *glob;
        else *glob = w.rl[e];
    }
}

// the prologue: the LDS pointers, the thread's place, rings and basis into LDS where the host gave them room.  The caller places the barrier.
// owner: which block of npw neurons the workgroup owns (blockIdx.x on a grid that splits the neurons; 0 where a workgroup owns them all)
__device__ __forceinline__ Wg wg_begin(const GenArgs& g, int R, int owner) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Wg w;
    w.smem = smem;
    w.ok_lds = reinterpret_cast<int*>(smem);
    w.xs = reinterpret_cast<double*>(smem + 16);
    w.rl = g.ring_off ? reinterpret_cast<double*>(smem + g.ring_off) : nullptr;
    w.sb = g.basis_off ? reinterpret_cast<double*>(smem + g.basis_off) : nullptr;
    w.n_lo = owner * g.npw;
    w.nown = min(g.N, w.n_lo + g.npw) - w.n_lo;
    w.NB = g.N * g.B;
    w.gpw = 64 / g.lpn; w.grp = lane / g.lpn; w.gl = lane % g.lpn;
    w.one_round = w.nown <= GEN_WAVES * w.gpw;
    w.i1 = wave * w.gpw + w.grp;
    w.mine1 = w.one_round && w.i1 < w.nown && w.gl == 0;
    w.bias1 = w.mine1 ? g.bias[w.n_lo + w.i1] : 0.0;
    if (w.rl) ring_copy<true>(g, R, w);
    if (w.sb)
        for (int e = threadIdx.x; e < g.L * g.B; e += GEN_THREADS) w.sb[e] = g.basis[e];
    return w;
}

// the lane's elements of its neuron's row of Wm into registers for the launch (KR > 0; the host picks KR only with one neuron per wave)
template <int KR>
__device__ __forceinline__ void load_row(const GenArgs& g, const Wg& w, double (&wr)[KR > 0 ? KR : 1]) {
    if (KR > 0) {
        const double* row = g.Wm + (long)(w.n_lo + (w.i1 < w.nown ? w.i1 : 0)) * w.NB;
#pragma unroll
        for (int q = 0; q < (KR > 0 ? KR : 1); ++q) {               // (every load is issued, from an element of the row that exists: no branches)
            const int j = w.gl + q * 64;
            const double v = row[j < w.NB ? j : 0];
            wr[q] = (w.i1 < w.nown && j < w.NB) ? v : 0.0;
        }
    }
}

// the epilogue: rings in LDS go back for the next launch
__device__ __forceinline__ void wg_end(const GenArgs& g, int R, const Wg& w) {
    if (w.rl) {
        __syncthreads();
        ring_copy<false>(g, R, w);
    }
}

// One trajectory on the caller's draws U.  KR > 0: every lane keeps its <= KR elements of its neuron's row of Wm in registers for the whole
// launch (the workgroup's rows are read from memory once per launch, not once per bin); KR = 0: the rows stream from memory every bin.
// XLDS: x_t is read from LDS.
template <bool XLDS, int KR>
__global__ __launch_bounds__(GEN_THREADS) void generate_kernel(GenArgs g) {
    const Wg w = wg_begin(g, 1, blockIdx.x);                         // LDS x: N*B, or KR*64 of which those beyond N*B are zero
    double wr[KR > 0 ? KR : 1];
    load_row<KR>(g, w, wr);
    const int wave = threadIdx.x >> 6, L = g.L;
    const bool direct = XLDS && gridDim.x == 1;                      // one workgroup: x goes straight into LDS, no exchange buffer
    unsigned epoch = 0;
    if (KR > 0)
        for (int j = w.NB + threadIdx.x; j < KR * 64; j += GEN_THREADS) w.xs[j] = 0.0;
    __syncthreads();

    double v_next = w.mine1 ? g.U[w.n_lo + w.i1] : 0.0;              // with one round per wave the next bin's draw is loaded ahead of time
    history(g, 1, g.t0 - 1, w.n_lo, w.nown, w.rl, w.sb, direct ? w.xs : g.xbuf + (g.t0 & 1) * (long)w.NB);      // x_{t0} from the ring
    if (!grid_sync(g, ++epoch, g.t0, w.ok_lds)) return;
    for (int k = 0; k < g.Tc; ++k) {
        const long t = g.t0 + k;
        const double* x = g.xbuf + (t & 1) * (long)w.NB;
        if (XLDS && !direct) {
            stage_x(w.xs, x, w.NB);
            __syncthreads();
        }
        for (int r0 = 0; r0 < w.nown; r0 += GEN_WAVES * w.gpw) {     // wave-uniform trip count: the shuffles of row_dot see every lane
            const int i = r0 + wave * w.gpw + w.grp;
            const bool mine = i < w.nown && w.gl == 0;
            const double v = w.one_round ? v_next : mine ? g.U[(long)k * g.N + w.n_lo + i] : 0.0;     // issued ahead of the dot product
            if (w.mine1 && k + 1 < g.Tc) v_next = g.U[(long)(k + 1) * g.N + w.n_lo + w.i1];
            const double acc = row_dot<KR>(wr, g.Wm + (long)(w.n_lo + (i < w.nown ? i : 0)) * w.NB, XLDS ? w.xs : x, w.NB, w.gl, g.lpn, i < w.nown);
            if (mine) {
                const int n = w.n_lo + i;
                const double psi = acc + (w.one_round ? w.bias1 : g.bias[n]);
                double y;
                if (g.obs == 0) y = v < 1.0 / (1.0 + exp(-psi)) ? 1.0 : 0.0;
                else y = __dadd_rn(psi, __dmul_rn(g.scale, v));
                g.Y[(long)k * g.N + n] = y;
                const int row = (int)(t % L);
                if (w.rl) w.rl[row * w.nown + i] = y;
                else g.ring[(long)row * g.N + n] = y;
            }
        }
        if (k + 1 == g.Tc) break;
        if (!w.rl) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // (a ring in global memory: this bin's row before it is read)
        __syncthreads();                                              // this bin's ring row is complete, and x_t is no longer read
        history(g, 1, t, w.n_lo, w.nown, w.rl, w.sb, direct ? w.xs : g.xbuf + ((t + 1) & 1) * (long)w.NB);
        if (!grid_sync(g, ++epoch, t + 1, w.ok_lds)) return;
    }
    wg_end(g, 1, w);
}

// =====================================================================================================================================
// pgl_simulate: R replicate trajectories of the FITTED model per launch -- posterior predictive simulation.
//
// THE LAW (pyglm_amd/simulate.py holds the separately written NumPy version of exactly this; the two are checked against each other).
//   activation   psi_t[r, n] = Wm[n, :] . x_t[r] + bias[n],   Wm = a*W (the activation of `means` and log_likelihood(), NOT generate()'s
//                stored W),  x_t[r][m, :] = sum_l Y_r[t-1-l, m] basis[l, :]  as in generate_kernel
//   model        kind[n] in {0 Bernoulli, 1 Gaussian, 2 negative binomial, 3 binomial}, par[n] = (unused, sqrt(eta_n), xi_n, n_n): every
//                neuron draws from its OWN regression's model
//   stream       Philox4x32-10, key = seed, purpose = PGL_PURPOSE_SIM, stream = (replicate << 32) | global neuron, element = global
//                time bin t, call index j = 0, 1, ...; one lane owns one draw (pgl_unif).  u1, u2 = the two uniforms of call j = 0.
//                Path r is a function of (seed, r, parameters, initial history): not of R, the chunking or the launch geometry.
//   Bernoulli    y = u1 < 1 / (1 + exp(-psi))
//   Gaussian     y = psi + par * (sqrt(-2 log u1) * cos(2 pi u2))
//   binomial     n = par <= PGL_SIM_BINOMIAL_MAX_N (64; the host refuses a larger n).  pp = 1 / (1 + exp(|psi|)) = min(p, 1 - p), q = 1 - pp,
//                s = pp / q;  f = q^n by n multiplications;  c = f, k = 0;  while u1 >= c and k < n:  f = f * (n - k) / (k + 1) * s, k += 1,
//                c = c + f.   y = k, mirrored to n - k when psi > 0 (p > 1/2)
//   neg. binom.  xi = par, p = 1 / (1 + exp(-psi)), softplus = max(psi, 0) + log1p(exp(-|psi|));  f = exp(-xi * softplus) = (1 - p)^xi;
//                c = f, k = 0;  while u1 >= c and k < PGL_SIM_NEGBIN_CAP (65 535):  f = f * p * (k + xi) / (k + 1), k += 1, c = c + f.   y = k.
//                A walk that reaches the cap sets the status word {2, bin, replicate, neuron}: an exploding count model ends as an error.
//   Every fp64 operation of the walks is evaluated left to right as written, uncontracted, on both sides.
constexpr int SIM_NEGBIN_CAP = 65535;
constexpr int SIM_PF = GEN_KR * 64 / GEN_THREADS;     // doubles of x per thread in the register-staged copy
constexpr size_t SIM_RING_LDS_MAX = 64 * 1024;
constexpr size_t SIM_LDS_BYTES = 160 * 1024;          // LDS of a gfx950 CU: the launch's whole request stays below it
constexpr int SIM_PSI_MAX = 1024;                     // activations (replicate, neuron) of a workgroup held in LDS between the two phases of a bin

struct SimArgs {
    GenArgs g;               // Wm, bias, basis, ring ([R][L][N]), xbuf ([2][R][N*B]), bar, status ([4]), t0, Tc, N, B, L, npw, lpn, lpp, offsets, spin_ticks
    const int* kind; const double* par;
    double* Y; long ldr;     // [R][Tc][N], replicate stride ldr; or null
    double* sum; double* sumsq;
    int R; long rep0; unsigned long long seed;
    int psi_off;             // byte offset of the activation table in LDS
};

// pgl_simulate_offset: the same block with the offset behind it, so that the kernels without an offset keep the argument block they had
struct SimOffArgs {
    SimArgs s;
    const double* Off; long ldo_t, ldo_r;     // [R][Tc][ldo_t], replicate stride ldo_r (0: shared by the replicates)
};
template <bool OFF> using SimArgsOf = typename std::conditional<OFF, SimOffArgs, SimArgs>::type;
__device__ __forceinline__ const SimArgs& sim_args(const SimArgs& a) { return a; }
__device__ __forceinline__ const SimArgs& sim_args(const SimOffArgs& a) { return a.s; }
constexpr int SIM_OFF_PAIRS = SIM_PSI_MAX / GEN_THREADS;   // (replicate, neuron) pairs of a group a thread draws at most

__device__ __forceinline__ void sim_cap_fail(int* status, long bin, long rep, int n) {
    int expect = 0;
    if (__hip_atomic_compare_exchange_strong(status, &expect, 2, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        __hip_atomic_store(status + 1, (int)bin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(status + 2, (int)rep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(status + 3, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one draw of neuron's model at activation psi (THE LAW above); every loop is bounded
__device__ double sim_draw(int kind, double par, double psi, PglPhilox& rng, bool& capped) {
#pragma clang fp contract(off)
    const double u1 = pgl_unif(rng);
    if (kind == 0) return u1 < 1.0 / (1.0 + exp(-psi)) ? 1.0 : 0.0;
    if (kind == 1) {
        const double u2 = pgl_unif(rng);
        const double gauss = sqrt(-2.0 * log(u1)) * cos(2.0 * PGL_PI * u2);
        return __dadd_rn(psi, __dmul_rn(par, gauss));
    }
    if (kind == 3) {
        int n = (int)par;
        n = n < 0 ? 0 : n > PGL_SIM_BINOMIAL_MAX_N ? PGL_SIM_BINOMIAL_MAX_N : n;
        const double pp = 1.0 / (1.0 + exp(fabs(psi)));
        const double q = 1.0 - pp, s = pp / q;
        double f = 1.0;
        for (int i = 0; i < n; ++i) f = f * q;
        double c = f;
        int k = 0;
        while (u1 >= c && k < n) {
            f = f * (double)(n - k) / (double)(k + 1) * s;
            ++k;
            c = c + f;
        }
        return (double)(psi > 0.0 ? n - k : k);
    }
    const double xi = par;
    const double p = 1.0 / (1.0 + exp(-psi));
    const double softplus = (psi > 0.0 ? psi : 0.0) + log1p(exp(-fabs(psi)));
    double f = exp(-xi * softplus), c = f;
    int k = 0;
    while (u1 >= c && k < SIM_NEGBIN_CAP) {
        f = f * p * ((double)k + xi) / (double)(k + 1);
        ++k;
        c = c + f;
    }
    if (k >= SIM_NEGBIN_CAP) capped = true;
    return (double)k;
}

// R trajectories on the device's Philox stream.  KR > 0: the rows of Wm in registers and x_r double-buffered in LDS; KR = 0, XLDS: x_r staged
// in LDS one replicate at a time; else x_r read from the exchange buffer.  A bin runs in two phases per group of replicates: the dot
// products, one replicate after the other, leave psi[r][n] in an LDS table; then the draws of ALL (replicate, neuron) pairs of the group run
// side by side, one lane each.  The pair a thread takes first is the same in every bin: its model and its running sums stay in registers for
// the whole launch.
// OFF: psi = (Wm . x + bias) + Off[r][k][n], one rounded sum added last in the draw phase; a thread loads the offsets of the group's pairs it
// will draw BEFORE the group's dot products, so that they arrive behind them.  OFF = false is the kernel without any of it.
template <bool XLDS, int KR, bool OFF>
__global__ __launch_bounds__(GEN_THREADS) void simulate_kernel(SimArgsOf<OFF> sa) {
    const SimArgs& s = sim_args(sa);
    const GenArgs& g = s.g;
    const int R = s.R;
    const Wg w = wg_begin(g, R, blockIdx.x);                         // LDS x: 2 * KR * 64 (KR > 0) or N*B (XLDS); after the basis, psi: SIM_PSI_MAX
    double wr[KR > 0 ? KR : 1];
    load_row<KR>(g, w, wr);
    double* xs = w.xs;
    double* psi_l = reinterpret_cast<double*>(w.smem + s.psi_off);
    const int wave = threadIdx.x >> 6;
    const int n_lo = w.n_lo, nown = w.nown, N = g.N, NB = w.NB, L = g.L;
    const long ringN = (long)L * N, ringW = (long)L * nown;
    const int RB = SIM_PSI_MAX / g.npw;                              // replicates per group (the host checks npw <= SIM_PSI_MAX)
    unsigned epoch = 0;
    __syncthreads();

    // the thread's pair in the first group of replicates
    const bool own1 = (int)threadIdx.x < min(RB, R) * nown;
    const int r1 = own1 ? threadIdx.x / nown : 0, n1 = n_lo + (own1 ? threadIdx.x % nown : 0);
    const int kind1 = own1 ? s.kind[n1] : 0;
    const double par1 = own1 ? s.par[n1] : 0.0;
    double sum1 = own1 ? s.sum[(long)r1 * N + n1] : 0.0, sq1 = own1 ? s.sumsq[(long)r1 * N + n1] : 0.0;
    history(g, R, g.t0 - 1, n_lo, nown, w.rl, w.sb, g.xbuf + (g.t0 & 1) * (long)R * NB);             // x_{t0} from the rings
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!grid_sync(g, ++epoch, g.t0, w.ok_lds)) return;
    for (int k = 0; k < g.Tc; ++k) {
        const long t = g.t0 + k;
        const double* xt = g.xbuf + (t & 1) * (long)R * NB;
        const int row = (int)(t % L);
        int capped = 0;
        double pf[KR > 0 ? SIM_PF : 1];
        if (KR > 0) {                                                // x_0 into the first buffer
#pragma unroll
            for (int q = 0; q < SIM_PF; ++q) { const int j = threadIdx.x + q * GEN_THREADS; pf[q] = j < NB ? xt[j] : 0.0; }
#pragma unroll
            for (int q = 0; q < SIM_PF; ++q) xs[threadIdx.x + q * GEN_THREADS] = pf[q];
            __syncthreads();
        }
        for (int rb = 0; rb < R; rb += RB) {
            const int rn = min(RB, R - rb);
            [[maybe_unused]] double off[OFF ? SIM_OFF_PAIRS : 1];
            if constexpr (OFF) {                                      // (rn * nown <= SIM_PSI_MAX = SIM_OFF_PAIRS * GEN_THREADS)
#pragma unroll
                for (int q = 0; q < SIM_OFF_PAIRS; ++q) {
                    const int it = threadIdx.x + q * GEN_THREADS;
                    const bool in = it < rn * nown;
                    const int r = rb + (in ? it / nown : 0), i = in ? it % nown : 0;
                    off[q] = in ? sa.Off[(long)r * sa.ldo_r + (long)k * sa.ldo_t + n_lo + i] : 0.0;
                }
            }
            for (int r = rb; r < rb + rn; ++r) {
                const double* x = xt + (long)r * NB;
                const double* xc = xs;                               // what the dot products read x_r from, when from LDS
                if (KR > 0) {
                    xc = xs + (r & 1) * (KR * 64);
                    if (r + 1 < R) {                                 // x_{r+1} on its way while the dot products of x_r run
#pragma unroll
                        for (int q = 0; q < SIM_PF; ++q) { const int j = threadIdx.x + q * GEN_THREADS; pf[q] = j < NB ? x[NB + j] : 0.0; }
                    }
                } else if (XLDS) {
                    stage_x(xs, x, NB);
                    __syncthreads();
                }
                for (int r0 = 0; r0 < nown; r0 += GEN_WAVES * w.gpw) { // wave-uniform trip count: the shuffles of row_dot see every lane
                    const int i = r0 + wave * w.gpw + w.grp;
                    const double acc = row_dot<KR>(wr, g.Wm + (long)(n_lo + (i < nown ? i : 0)) * NB, XLDS ? xc : x, NB, w.gl, g.lpn, i < nown);
                    if (i < nown && w.gl == 0) psi_l[(r - rb) * nown + i] = acc + (w.one_round ? w.bias1 : g.bias[n_lo + i]);
                }
                if (KR > 0) {
                    if (r + 1 < R) {
                        double* xn = xs + ((r + 1) & 1) * (KR * 64);
#pragma unroll
                        for (int q = 0; q < SIM_PF; ++q) xn[threadIdx.x + q * GEN_THREADS] = pf[q];
                    }
                    __syncthreads();                                  // x_{r+1} is complete, and x_r is no longer read
                } else if (XLDS) {
                    __syncthreads();                                  // x_r is no longer read
                }
            }
            __syncthreads();                                          // the group's activations are in the table
            for (int it = threadIdx.x; it < rn * nown; it += GEN_THREADS) {
                const bool first = rb == 0 && it == (int)threadIdx.x;  // the pair whose model and sums the thread keeps
                const int r = rb + it / nown, i = it % nown, n = n_lo + i;
                PglPhilox rng;
                pgl_rng_init(rng, s.seed, ((uint64_t)(s.rep0 + r) << 32) | (uint32_t)n, (uint64_t)t, PGL_PURPOSE_SIM);
                bool cap = false;
                double psi = psi_l[it];
                if constexpr (OFF) {
                    const int q = (it - (int)threadIdx.x) / GEN_THREADS;
                    psi = __dadd_rn(psi, q == 0 ? off[0] : q == 1 ? off[1] : q == 2 ? off[2] : off[3]);
                }
                const double y = sim_draw(first ? kind1 : s.kind[n], first ? par1 : s.par[n], psi, rng, cap);
                if (cap) { sim_cap_fail(g.status, t, s.rep0 + r, n); capped = 1; }
                if (s.Y) s.Y[(long)r * s.ldr + (long)k * N + n] = y;
                if (w.rl) w.rl[r * ringW + (long)row * nown + i] = y;
                else g.ring[r * ringN + (long)row * N + n] = y;
                if (first) {
                    sum1 = __dadd_rn(sum1, y);
                    sq1 = __dadd_rn(sq1, __dmul_rn(y, y));
                } else {
                    s.sum[(long)r * N + n] = __dadd_rn(s.sum[(long)r * N + n], y);
                    s.sumsq[(long)r * N + n] = __dadd_rn(s.sumsq[(long)r * N + n], __dmul_rn(y, y));
                }
            }
            if (rb + RB < R) __syncthreads();                         // the table is free for the next group
        }
        if (!w.rl) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // (rings in global memory: this bin's rows before they are read)
        if (__syncthreads_or(capped)) return;                         // a capped walk ends the launch: the status word names it
        if (k + 1 == g.Tc) break;
        history(g, R, t, n_lo, nown, w.rl, w.sb, g.xbuf + ((t + 1) & 1) * (long)R * NB);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (!grid_sync(g, ++epoch, t + 1, w.ok_lds)) return;
    }
    if (own1) { s.sum[(long)r1 * N + n1] = sum1; s.sumsq[(long)r1 * N + n1] = sq1; }
    wg_end(g, R, w);
}

// =====================================================================================================================================
// pgl_conditional_simulate: R replicate trajectories of F FREE neurons of the fitted model, the other neurons clamped to a recording.
//
// The law is stated once, in the docstring of conditional_host in pyglm_amd/simulate.py ("THE CONDITIONAL LAW"); in short
//   psi_r[t, j] = base[t, j] + Wff[j, :] . x_r[t],   x_r[t][k, :] = sum_l y_r[t-1-l, k] basis[l, :]   over the free neurons k alone,
// base -- the bias and everything the clamped neurons contribute, parallel in time -- being an INPUT, and y_r[t, j] sim_draw's draw of the
// free neuron's own model on the stream of pgl_simulate: stream = (replicate << 32) | neuron[j], the GLOBAL index, element = t.
//
// Only the F x (F*B) block is serial in t and the replicates do not interact: workgroup r walks the bins of replicate r by itself, in a plain
// launch -- no exchange buffer, no grid barrier, nothing a workgroup waits for but its own two barriers per bin (x_t complete; the ring row
// of y_t complete and x_t no longer read).  It is the one-workgroup form of the scheme above on an F-neuron model, from the same pieces:
// history writes x_t straight into LDS, row_dot folds it with the row of Wff in the order that is psi's bits, sim_draw draws.  The lanes
// split as lane_split decides for a workgroup that owns F neurons; F <= PGL_COND_MAX_FREE = GEN_THREADS makes that ONE round: lane 0 of a
// group keeps its neuron, its model and its running sums for the whole launch.  Residency by size (the host's plan): the ring [L][F] and the
// basis in LDS or in global memory as for pgl_simulate; Wff in LDS when it fits behind them, else streamed from L2.
struct CondArgs {
    GenArgs g;               // Wm = Wff, bias = base (only read by wg_begin), basis, ring ([R][L][F]), status ([4]), t0, Tc, N = npw = F, B, L, lpn, lpp, offsets
    const double* base; long ldb;            // [Tc][ldb], row k = bin t0 + k
    const int* kind; const double* par;      // [F], of the free neurons
    const int* neuron;                       // [F] global indices
    double* Y; long ldr;                     // [R][Tc][F], replicate stride ldr; or null
    double* Psi; long ldp;                   // likewise
    double* sum; double* sumsq;              // [R][F]
    long rep0; unsigned long long seed;
    int wff_off;                             // byte offset of Wff in LDS (0: streamed)
};

__global__ __launch_bounds__(GEN_THREADS) void conditional_kernel(CondArgs c) {
    const int r = blockIdx.x;
    GenArgs g = c.g;
    g.ring += (long)r * g.L * g.N;                                   // the workgroup's replicate is the whole "model" of the pieces
    const Wg w = wg_begin(g, 1, 0);                                   // LDS x: F*B
    const int F = g.N, NB = w.NB, L = g.L;
    const double* wff = g.Wm;
    if (c.wff_off) {
        double* wl = reinterpret_cast<double*>(w.smem + c.wff_off);
        for (int e = threadIdx.x; e < F * NB; e += GEN_THREADS) wl[e] = g.Wm[e];
        wff = wl;
    }
    const int j = w.i1;                                              // the host checks F <= GEN_WAVES * gpw: one round
    const bool mine = w.mine1;
    const double* row = wff + (long)(j < F ? j : 0) * NB;
    const int n = mine ? c.neuron[j] : 0, kind = mine ? c.kind[j] : 0;
    const double par = mine ? c.par[j] : 0.0;
    double sum1 = mine ? c.sum[(long)r * F + j] : 0.0, sq1 = mine ? c.sumsq[(long)r * F + j] : 0.0;
    const double wr[1] = {0.0};
    __syncthreads();
    for (int k = 0; k < g.Tc; ++k) {
        const long t = g.t0 + k;
        history(g, 1, t - 1, 0, F, w.rl, w.sb, w.xs);                // x_t from the ring
        __syncthreads();
        const double bt = mine ? c.base[(long)k * c.ldb + j] : 0.0;  // issued ahead of the dot product
        const double acc = row_dot<0>(wr, row, w.xs, NB, w.gl, g.lpn, j < F);
        int capped = 0;
        if (mine) {
            const double psi = bt + acc;
            PglPhilox rng;
            pgl_rng_init(rng, c.seed, ((uint64_t)(c.rep0 + r) << 32) | (uint32_t)n, (uint64_t)t, PGL_PURPOSE_SIM);
            bool cap = false;
            const double y = sim_draw(kind, par, psi, rng, cap);
            if (cap) { sim_cap_fail(g.status, t, c.rep0 + r, n); capped = 1; }
            if (c.Y) c.Y[(long)r * c.ldr + (long)k * F + j] = y;
            if (c.Psi) c.Psi[(long)r * c.ldp + (long)k * F + j] = psi;
            const int rw = (int)(t % L);
            if (w.rl) w.rl[rw * F + j] = y;
            else g.ring[(long)rw * F + j] = y;
            sum1 = __dadd_rn(sum1, y);
            sq1 = __dadd_rn(sq1, __dmul_rn(y, y));
        }
        if (!w.rl) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // (a ring in global memory: this bin's row before it is read)
        if (__syncthreads_or(capped)) return;                         // a capped walk ends THIS workgroup: the status word names it
    }
    if (mine) { c.sum[(long)r * F + j] = sum1; c.sumsq[(long)r * F + j] = sq1; }
    wg_end(g, 1, w);
}

struct GenGeometry { int G, npw, lpn, lpp; };

// the lanes of a workgroup that owns q.npw neurons: lpn per neuron in the dot products, lpp per (neuron, basis function) in the history sums
void lane_split(GenGeometry& q, int B) {
    int per_wave = (q.npw + GEN_WAVES - 1) / GEN_WAVES, gpw = 1;
    while (gpw < per_wave && gpw < 64) gpw *= 2;
    q.lpn = 64 / gpw;
    // lanes per (neuron, basis function) sum of the history: as many as leave every pair of the workgroup a group in one round
    const int pairs = q.npw * B;
    q.lpp = 64;
    while (q.lpp > 1 && pairs * q.lpp > GEN_THREADS) q.lpp /= 2;
}

GenGeometry geometry(int N, int B) {
    GenGeometry q;
    if ((long)N * N * B <= PGL_GEN_ONE_WG_MAX) q.G = 1;
    else q.G = std::min(pgl_device_cus(pgl_device()), (N + 3) / 4);
    q.npw = (N + q.G - 1) / q.G;
    q.G = (N + q.npw - 1) / q.npw;                                     // no workgroup without neurons
    lane_split(q, B);
    return q;
}

long long wall_clock_khz(int dev) {
    static std::atomic<long long> tick_khz[PGL_MAX_DEVICES];
    long long khz = tick_khz[dev & (PGL_MAX_DEVICES - 1)].load(std::memory_order_relaxed);
    if (khz <= 0) {
        int r = 0;
        if (hipDeviceGetAttribute(&r, hipDeviceAttributeWallClockRate, dev) != hipSuccess || r <= 0) r = 100000;
        khz = r;
        tick_khz[dev & (PGL_MAX_DEVICES - 1)].store(khz, std::memory_order_relaxed);
    }
    return khz;
}

// zero the barrier block, give the kernel its dynamic LDS, launch it cooperatively
template <auto Kernel, typename Args>
int launch(const char* entry, const Args& a, void* work, int G, size_t lds, hipStream_t st) {
    static PglPerDeviceSize lds_set;
    hipError_t e = hipMemsetAsync(work, 0, GEN_BAR_BYTES, st);
    if (e != hipSuccess) { pgl_set_error("%s: hipMemsetAsync: %s", entry, hipGetErrorString(e)); return PGL_ERR_HIP; }
    int rc = pgl_grow_dynamic_lds(reinterpret_cast<const void*>(Kernel), lds, lds_set);
    if (rc) return rc;
    void* args[] = {const_cast<Args*>(&a)};
    e = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(Kernel), dim3(G), dim3(GEN_THREADS), args, lds, st);
    if (e != hipSuccess) { pgl_set_error("%s: cooperative launch of %d workgroups: %s", entry, G, hipGetErrorString(e)); return PGL_ERR_HIP; }
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}

// the launch's geometry, which kernel instance runs it and its dynamic LDS
struct GenPlan { GenGeometry q; bool xlds, regs; size_t lds; };

// what an entry point asks of the LDS layout: row_regs, its kernel has an instance that keeps the rows of Wm in registers, and x is
// double-buffered there with x_double; the rings go into LDS when they are at most ring_cap and the whole request -- with the basis and the
// `extra` bytes the kernel appends -- stays within lds_cap
struct LdsPolicy { bool row_regs, x_double; size_t ring_cap, lds_cap, extra; };
// (pgl_generate: the ring's, the basis' and x's own caps keep the request at about 112 KiB, far below a CU's LDS: no test of the total)
constexpr LdsPolicy GEN_LDS_POLICY = {true, false, GEN_RING_LDS_MAX, SIZE_MAX, 0};
// (pgl_simulate: the rings go into LDS when they, the basis and the activation table still fit the CU's 160 KiB beside x)
constexpr LdsPolicy SIM_LDS_POLICY = {true, true, SIM_RING_LDS_MAX, SIM_LDS_BYTES, SIM_PSI_MAX * sizeof(double)};

// (pgl_conditional_simulate: the same caps on ring and basis, below the CU's LDS as a whole; Wff takes what is left, decided by the entry point)
constexpr LdsPolicy COND_LDS_POLICY = {false, false, SIM_RING_LDS_MAX, SIM_LDS_BYTES, 0};

// The plan of a launch of R trajectories per workgroup on the geometry q, and the head of its argument block (what is not set here is the
// entry point's own).  x in LDS is N*B doubles, or with the rows of Wm in registers GEN_KR * 64 (twice that when the kernel double-buffers x).
int plan(const GenGeometry& q, int N, int B, int L, int R, const LdsPolicy& pol, const double* Wm, const double* bias, const double* basis, double* ring, long t0,
         int Tc, void* work, int* status, GenArgs& a, GenPlan& p) {
    PGL_CHECK_ARG((long)N * B <= (1L << 30) && (long)L * N <= (1L << 31) - 1);
    const int NB = N * B;
    auto al16 = [](size_t x) { return (x + 15) / 16 * 16; };
    p.q = q;
    p.xlds = NB <= GEN_XLDS_MAX;
    // registers for the rows of Wm: one neuron per wave (npw <= 4, 64 lanes per neuron) and at most GEN_KR elements per lane
    p.regs = pol.row_regs && p.xlds && q.npw <= GEN_WAVES && q.lpn == 64 && NB <= GEN_KR * 64;
    size_t lds = 16 + (p.regs ? (pol.x_double ? 2 : 1) * (size_t)GEN_KR * 64 * sizeof(double) : p.xlds ? al16((size_t)NB * sizeof(double)) : 0);
    const size_t ring_bytes = (size_t)R * L * q.npw * sizeof(double), basis_bytes = (size_t)L * B * sizeof(double);
    const bool basis_lds = basis_bytes <= GEN_BASIS_LDS_MAX;
    if (ring_bytes <= pol.ring_cap && lds + al16(ring_bytes) + (basis_lds ? al16(basis_bytes) : 0) + pol.extra <= pol.lds_cap) {
        a.ring_off = (int)lds;
        lds += al16(ring_bytes);
    }
    if (basis_lds) { a.basis_off = (int)lds; lds += al16(basis_bytes); }
    p.lds = lds;
    a.Wm = Wm; a.bias = bias; a.basis = basis; a.ring = ring;
    a.bar = static_cast<unsigned*>(work);                            // (work null: a kernel without exchange buffers and grid barrier)
    a.xbuf = work ? reinterpret_cast<double*>(static_cast<char*>(work) + GEN_BAR_BYTES) : nullptr;
    a.status = status;
    a.t0 = t0; a.Tc = Tc; a.N = N; a.B = B; a.L = L;
    a.npw = q.npw; a.lpn = q.lpn; a.lpp = q.lpp;
    a.spin_ticks = (unsigned long long)wall_clock_khz(pgl_device()) * 2000ULL;        // 2 s of the wall clock per barrier
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
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    GenArgs a{};
    GenPlan p;
    int rc = plan(geometry(N, B), N, B, L, 1, GEN_LDS_POLICY, Wm, bias, basis, ring, t0, Tc, work, status, a, p);
    if (rc) return rc;
    a.U = U; a.Y = Y; a.obs = obs; a.scale = noise_scale;
    if (p.regs) return launch<generate_kernel<true, GEN_KR>>("pgl_generate", a, work, p.q.G, p.lds, st);
    if (p.xlds) return launch<generate_kernel<true, 0>>("pgl_generate", a, work, p.q.G, p.lds, st);
    return launch<generate_kernel<false, 0>>("pgl_generate", a, work, p.q.G, p.lds, st);
}

extern "C" size_t pgl_simulate_work_bytes(int N, int B, int R) {
    if (N <= 0 || B <= 0 || R <= 0) return 0;
    return GEN_BAR_BYTES + 2 * (size_t)R * N * B * sizeof(double);
}

namespace {
static_assert(SIM_OFF_PAIRS == 4, "the draw phase selects among four offsets");

// pgl_simulate and pgl_simulate_offset: Off null queues the kernels without an offset
int simulate_entry(const char* entry, const double* Wm, const double* bias, const double* basis, int N, int B, int L, const int* kind, const double* par,
                   int R, long rep0, unsigned long long seed, double* ring, double* Y, long ldr, double* sum, double* sumsq, long t0, int Tc,
                   void* work, int* status, const double* Off, long ldo_t, long ldo_r, void* hip_stream) {
    PGL_CHECK_ARG(Wm && bias && basis && kind && par && ring && sum && sumsq && work && status);
    PGL_CHECK_ARG(N > 0 && B > 0 && L > 0 && R > 0 && Tc > 0 && t0 >= 0 && rep0 >= 0);
    PGL_CHECK_ARG(t0 + Tc <= (1L << 31) - 1 && rep0 + R <= (1L << 31) - 1);           // the status word and the Philox counter hold them in 32 bits
    PGL_CHECK_ARG(!Y || ldr >= (long)Tc * N);
    PGL_CHECK_ARG(!Off || (ldo_t >= N && (ldo_r == 0 || ldo_r >= (long)(Tc - 1) * ldo_t + N)));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    SimArgs s{};
    GenPlan p;
    int rc = plan(geometry(N, B), N, B, L, R, SIM_LDS_POLICY, Wm, bias, basis, ring, t0, Tc, work, status, s.g, p);
    if (rc) return rc;
    PGL_CHECK_ARG((long)R * p.q.npw * B <= (1L << 30) && (long)R * L * p.q.npw <= (1L << 30) && p.q.npw <= SIM_PSI_MAX);
    s.psi_off = (int)p.lds;                                          // the activation table at the end
    p.lds += SIM_PSI_MAX * sizeof(double);
    s.kind = kind; s.par = par; s.Y = Y; s.ldr = ldr; s.sum = sum; s.sumsq = sumsq; s.R = R; s.rep0 = rep0; s.seed = seed;
    if (Off) {
        SimOffArgs o{};
        o.s = s; o.Off = Off; o.ldo_t = ldo_t; o.ldo_r = ldo_r;
        if (p.regs) return launch<simulate_kernel<true, GEN_KR, true>>(entry, o, work, p.q.G, p.lds, st);
        if (p.xlds) return launch<simulate_kernel<true, 0, true>>(entry, o, work, p.q.G, p.lds, st);
        return launch<simulate_kernel<false, 0, true>>(entry, o, work, p.q.G, p.lds, st);
    }
    if (p.regs) return launch<simulate_kernel<true, GEN_KR, false>>(entry, s, work, p.q.G, p.lds, st);
    if (p.xlds) return launch<simulate_kernel<true, 0, false>>(entry, s, work, p.q.G, p.lds, st);
    return launch<simulate_kernel<false, 0, false>>(entry, s, work, p.q.G, p.lds, st);
}
}  // namespace

extern "C" int pgl_simulate(const double* Wm, const double* bias, const double* basis, int N, int B, int L, const int* kind, const double* par,
                            int R, long rep0, unsigned long long seed, double* ring, double* Y, long ldr, double* sum, double* sumsq, long t0,
                            int Tc, void* work, int* status, void* hip_stream) {
    return simulate_entry("pgl_simulate", Wm, bias, basis, N, B, L, kind, par, R, rep0, seed, ring, Y, ldr, sum, sumsq, t0, Tc, work, status,
                          nullptr, 0, 0, hip_stream);
}

extern "C" int pgl_simulate_offset(const double* Wm, const double* bias, const double* basis, int N, int B, int L, const int* kind, const double* par,
                                   int R, long rep0, unsigned long long seed, double* ring, double* Y, long ldr, double* sum, double* sumsq,
                                   long t0, int Tc, void* work, int* status, const double* Off, long ldo_t, long ldo_r, void* hip_stream) {
    return simulate_entry("pgl_simulate_offset", Wm, bias, basis, N, B, L, kind, par, R, rep0, seed, ring, Y, ldr, sum, sumsq, t0, Tc, work, status,
                          Off, ldo_t, ldo_r, hip_stream);
}

extern "C" int pgl_conditional_max_free(void) { return PGL_COND_MAX_FREE; }

extern "C" int pgl_conditional_simulate(const double* Wff, const double* base, long ldb, const double* basis, int F, int B, int L, const int* kind,
                                        const double* par, const int* neuron, int R, long rep0, unsigned long long seed, double* ring, double* Y,
                                        long ldr, double* Psi, long ldp, double* sum, double* sumsq, long t0, int Tc, int* status,
                                        void* hip_stream) {
    static PglPerDeviceSize lds_set;
    PGL_CHECK_ARG(Wff && base && basis && kind && par && neuron && ring && sum && sumsq && status);
    PGL_CHECK_ARG(F > 0 && F <= PGL_COND_MAX_FREE && B > 0 && L > 0 && R > 0 && Tc > 0 && t0 >= 0 && rep0 >= 0);
    PGL_CHECK_ARG((long)F * B <= GEN_XLDS_MAX);                                      // x_t lives in LDS
    PGL_CHECK_ARG(t0 + Tc <= (1L << 31) - 1 && rep0 + R <= (1L << 31) - 1);           // the status word and the Philox counter hold them in 32 bits
    PGL_CHECK_ARG(ldb >= F && (!Y || ldr >= (long)Tc * F) && (!Psi || ldp >= (long)Tc * F));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    CondArgs c{};
    GenPlan p;
    GenGeometry q;
    q.G = R; q.npw = F;
    lane_split(q, B);
    PGL_CHECK_ARG(F <= GEN_WAVES * (64 / q.lpn));                                    // one round of neurons
    int rc = plan(q, F, B, L, 1, COND_LDS_POLICY, Wff, base, basis, ring, t0, Tc, nullptr, status, c.g, p);
    if (rc) return rc;
    const size_t wff_bytes = ((size_t)F * F * B * sizeof(double) + 15) / 16 * 16;
    if (p.lds + wff_bytes <= SIM_LDS_BYTES) {                         // Wff behind x, the ring and the basis, when it fits
        c.wff_off = (int)p.lds;
        p.lds += wff_bytes;
    }
    c.base = base; c.ldb = ldb; c.kind = kind; c.par = par; c.neuron = neuron; c.Y = Y; c.ldr = ldr; c.Psi = Psi; c.ldp = ldp;
    c.sum = sum; c.sumsq = sumsq; c.rep0 = rep0; c.seed = seed;
    rc = pgl_grow_dynamic_lds(reinterpret_cast<const void*>(conditional_kernel), p.lds, lds_set);
    if (rc) return rc;
    hipLaunchKernelGGL(conditional_kernel, dim3(R), dim3(GEN_THREADS), p.lds, st, c);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}
