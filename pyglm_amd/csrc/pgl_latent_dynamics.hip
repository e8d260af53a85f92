// The temporal prior of the latent common input (pyglm_amd/latents.py states the law; include/pyglm_hip_latent_dynamics.h the call; DESIGN.md
// section 21): under an AR(1) prior a data set's T bins are one block-tridiagonal Gaussian of dimension T Q, drawn exactly and in parallel over
// time by nested dissection -- segments and separators, recursively.
//
// A chain of n blocks D_i (Q x Q, SPD), E_i = J[i + 1][i], h_i.  Bins seg - 1, 2 seg - 1, ... are separators, the runs between them interiors;
// group g owns interior [g seg, g seg + seg - 2] (the last one may be short or empty), its left separator l = g seg - 1 and its right one.
//
//   ar_reduce_kernel<Q, L0>  a group eliminates its interior, serially:   L_i = chol(D~_i), W_i = E_i L_i^-T, V_i = F_i L_i^-T (F_a = E_l',
//                            the fill towards the left separator; V_i is U_i' of the derivation), y_i = L_i^-1 (h_i - W_{i-1} y_{i-1}),
//                            D~_{i+1} = D_{i+1} - W_i W_i', F_{i+1} = -V_i W_i'.  Past the last interior bin those are the right separator's
//                            left partial (D - W W', h - W y) and E' = F' towards the left separator; sum_i V_i V_i' and sum_i V_i y_i are
//                            the left separator's right partial.  L, W, V and y are kept in scratch for the way back.
//   ar_base_kernel<Q, L0>    the last chain (fewer than 2 seg blocks, or all T bins where seg >= T): one group factors it and draws it.
//   ar_expand_kernel<Q, L0>  given its separators' draws x_l, x_r a group draws its interior backwards:
//                            x_i = L_i^-T (y_i + z_i - V_i' x_l - W_i' x_{i+1}).  The level-0 launch is the last one and writes S -- its
//                            interior and its right separator -- only where the status word is still 0.
//
// A group is G = 1, 2, 4 or 8 lanes (the power of two >= Q); lane c owns column c of the symmetric D~ (= its row c), row c of W and of V,
// hence column c of U; y is held by every lane.  The Cholesky is right-looking: at step k every lane scales its own entry of column k
// (L[c][k] = D~[k][c] / L[k][k]) and the column crosses lanes by __shfl, Q (Q + 1) / 2 values per bin; the three forward solves ride on the
// same values, so no lane ever holds L whole.  The Schur updates need W's and V's rows in every lane: 2 Q^2 more values per bin.  The lanes
// of a group run the same trips, so every __shfl finds its source lane active.  Scratch is the transposer: a lane writes the rows it owns and
// the way back reads the columns it needs.  Level 0 takes D from Lambda and the prior's diagonal, E = diag(e) from the arguments and z from
// the stream; the levels above take dense blocks from the level below.  Block j of level k is bin (j + 1) seg^k - 1: that bin's normals draw it.
// No floating-point atomics; a group's arithmetic depends on its own blocks alone.
#include "pgl_common.h"
#include "pgl_rng.h"
#include "../../include/pyglm_hip_latents.h"
#include "../../include/pyglm_hip_latent_dynamics.h"

namespace {

constexpr int AR_SEG_DEFAULT = 10;                                  // T = 100 000: chains of 100 000, 10 000, 1 000, 100 and 10 blocks (tools/probe_latent_ar.py)
constexpr int AR_MAX_LEVELS = 34;                                   // seg = 2 halves a chain of < 2^31 blocks at most 31 times
constexpr int AR_BLOCK = 64;                                        // one wavefront: 64 / G groups

struct ArArgs {
    // level 0
    const double *Lambda, *r, *zo;
    double dmid[PGL_LATENT_MAX], dend[PGL_LATENT_MAX], e[PGL_LATENT_MAX];
    uint64_t seed, sweep, elem0;
    int T;
    // the chain of this launch: n blocks, block j is bin (j + 1) stride - 1
    int n, seg;
    long stride;
    const double *DL, *DR, *hL, *hR, *E;                            // levels >= 1: [j][c][r] = D[r][c] in two partials, h likewise, [j][c][r] = E_j[r][c]
    double *Lf, *Wf, *Vf, *yf;                                      // [i][c][k] = L_i[c][k], W_i[c][k], V_i[c][k]; y_i[c]
    double *nDL, *nDR, *nhL, *nhR, *nE;                             // the separators' chain (reduce)
    double* X;                                                      // the draw, T x Q by bin
    double* S;
    long lds;
    int col0;
    int* status;
};

template <int G>
__device__ __forceinline__ double ar_bc(double v, int src) {      // lane `src` of the group's value
    if constexpr (G == 1) return v;
    else return __shfl(v, src, G);
}

template <int Q>
__device__ __forceinline__ double ar_pick(const double (&v)[Q], int c) {     // v[c] without a runtime-indexed register array
    double s = v[0];
#pragma unroll
    for (int q = 1; q < Q; ++q) s = c == q ? v[q] : s;
    return s;
}

template <int Q, bool L0>
struct ArChain {
    static constexpr int P = Q * (Q + 1) / 2;
    const ArArgs& a;
    int c;
    double ec, dm, de;                                              // level 0: this lane's e, prior diagonal inside and at the two ends
    __device__ ArChain(const ArArgs& a_, int c_) : a(a_), c(c_) {
        ec = ar_pick<Q>(reinterpret_cast<const double(&)[Q]>(a.e), c);
        dm = ar_pick<Q>(reinterpret_cast<const double(&)[Q]>(a.dmid), c);
        de = ar_pick<Q>(reinterpret_cast<const double(&)[Q]>(a.dend), c);
    }
    __device__ __forceinline__ long bin(long i) const { return (i + 1) * a.stride - 1; }
    __device__ __forceinline__ void load_D(long i, double (&d)[Q]) const {              // column c of D_i
        if (L0) {
            const double* lam = a.Lambda + i * P;
#pragma unroll
            for (int r = 0; r < Q; ++r) {
                const int hi = r > c ? r : c, lo = r > c ? c : r;
                d[r] = lam[hi * (hi + 1) / 2 + lo];
            }
            const double pd = a.T == 1 ? 1.0 : (i == 0 || i == a.T - 1) ? de : dm;
#pragma unroll
            for (int r = 0; r < Q; ++r) d[r] = r == c ? d[r] + pd : d[r];
        } else {
            const double *l = a.DL + (i * Q + c) * Q, *rr = a.DR + (i * Q + c) * Q;
#pragma unroll
            for (int r = 0; r < Q; ++r) d[r] = l[r] + rr[r];                            // the left segment's partial, then the right one's
        }
    }
    __device__ __forceinline__ void load_h(long i, double (&g)[Q]) const {              // h_i, whole
#pragma unroll
        for (int m = 0; m < Q; ++m) g[m] = L0 ? a.r[i * Q + m] : a.hL[i * Q + m] + a.hR[i * Q + m];
    }
    __device__ __forceinline__ void load_E_row(long i, double (&w)[Q]) const {          // row c of E_i
#pragma unroll
        for (int m = 0; m < Q; ++m) w[m] = L0 ? (m == c ? ec : 0.0) : a.E[(i * Q + m) * Q + c];
    }
    __device__ __forceinline__ void load_E_col(long i, double (&v)[Q]) const {          // column c of E_i: row c of E_i'
#pragma unroll
        for (int m = 0; m < Q; ++m) v[m] = L0 ? (m == c ? ec : 0.0) : a.E[(i * Q + c) * Q + m];
    }
    __device__ __forceinline__ double normal(long i) const {                            // z of block i, entry c
        const long t = bin(i);
        if (a.zo) return a.zo[t * Q + c];
        PglPhilox g;
        pgl_rng_init(g, a.seed, a.sweep, a.elem0 + (uint64_t)t, PGL_PURPOSE_LATENT);
        g.j = (uint32_t)c;                                                              // call c of the bin's generator
        return pgl_norm(g);
    }
};

// D~ = L L' by columns with the solves of w, v (this lane's rows of E and F) and g (h, whole) riding along: afterwards w, v are the lane's
// rows of W and V, g is y and lrow row c of L (zero above the diagonal)
template <int Q, int G>
__device__ __forceinline__ void ar_factor(double (&d)[Q], double (&w)[Q], double (&v)[Q], double (&g)[Q], double (&lrow)[Q], int c, bool& bad) {
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        double piv = ar_bc<G>(d[k], k);
        if (!(piv > 0.0)) { bad = true; piv = 1.0; }
        const double lkk = sqrt(piv), rl = 1.0 / lkk;               // one division per column: the chain of a bin is its latency
        const double lck = c == k ? lkk : d[k] * rl;                // L[c][k] where c >= k
        lrow[k] = c >= k ? lck : 0.0;
        w[k] *= rl; v[k] *= rl; g[k] *= rl;
#pragma unroll
        for (int r = k + 1; r < Q; ++r) {
            const double lrk = ar_bc<G>(lck, r);                    // L[r][k]
            d[r] -= lrk * lck;
            w[r] -= lrk * w[k]; v[r] -= lrk * v[k]; g[r] -= lrk * g[k];
        }
    }
}

// the forward pass over interior [i0, i1] of one group.  In: hasL (a left separator at i0 - 1).  Out: d, g, f hold what the pass leaves for
// block i1 + 1 (D - W W' column c, h - W y, row c of F) where that block exists; accD, acch the left separator's right partial.
template <int Q, int G, bool L0>
__device__ __forceinline__ void ar_forward(const ArChain<Q, L0>& ch, long i0, long i1, bool hasL, bool writer, double (&d)[Q], double (&g)[Q],
                                           double (&f)[Q], double (&accD)[Q], double& acch, bool& bad) {
    const ArArgs& a = ch.a;
    const int c = ch.c;
    ch.load_D(i0, d);
    ch.load_h(i0, g);
    if (hasL) ch.load_E_col(i0 - 1, f);
    else {
#pragma unroll
        for (int m = 0; m < Q; ++m) f[m] = 0.0;
    }
    for (long i = i0; i <= i1; ++i) {
        const bool hasN = i + 1 < a.n;
        double w[Q], dn[Q], gn[Q], fn[Q], lrow[Q];
        if (hasN) {                                                 // the next block's loads do not wait for this block's arithmetic
            ch.load_E_row(i, w);
            ch.load_D(i + 1, dn);
            ch.load_h(i + 1, gn);
        } else {
#pragma unroll
            for (int m = 0; m < Q; ++m) w[m] = dn[m] = gn[m] = 0.0;
        }
        ar_factor<Q, G>(d, w, f, g, lrow, c, bad);
        if (writer) {
            double *lf = a.Lf + (i * Q + c) * Q, *wf = a.Wf + (i * Q + c) * Q;
#pragma unroll
            for (int m = 0; m < Q; ++m) { lf[m] = lrow[m]; wf[m] = w[m]; }
            if (a.Vf) {
                double* vf = a.Vf + (i * Q + c) * Q;
#pragma unroll
                for (int m = 0; m < Q; ++m) vf[m] = f[m];
            }
            a.yf[i * Q + c] = ar_pick<Q>(g, c);
        }
#pragma unroll
        for (int r = 0; r < Q; ++r) {                               // row r of W in every lane
            double s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
            for (int m = 0; m < Q; ++m) {
                const double wr = ar_bc<G>(w[m], r);
                s1 += wr * w[m];
                s2 += wr * f[m];
                s3 += wr * g[m];
            }
            dn[r] -= s1;
            fn[r] = -s2;
            gn[r] -= s3;
        }
        if (hasL) {
#pragma unroll
            for (int r = 0; r < Q; ++r) {                           // row r of V in every lane
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < Q; ++m) s += ar_bc<G>(f[m], r) * f[m];
                accD[r] -= s;
            }
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < Q; ++m) s += f[m] * g[m];
            acch -= s;
        }
#pragma unroll
        for (int m = 0; m < Q; ++m) { d[m] = dn[m]; g[m] = gn[m]; f[m] = fn[m]; }
    }
}

// what bin i brings to the way back that does not wait for x_{i+1}: column c of L_i and of W_i, 1 / L_i[c][c], and t0 = (y_i + z_i - V_i' x_l)[c]
template <int Q, bool L0>
__device__ __forceinline__ void ar_fetch(const ArChain<Q, L0>& ch, long i, bool hasL, const double (&xl)[Q], double (&lc)[Q], double (&wc)[Q],
                                         double& rd, double& t0) {
    const ArArgs& a = ch.a;
    const int c = ch.c;
#pragma unroll
    for (int m = 0; m < Q; ++m) lc[m] = a.Lf[(i * Q + m) * Q + c];
#pragma unroll
    for (int r = 0; r < Q; ++r) wc[r] = a.Wf[(i * Q + r) * Q + c];
    t0 = a.yf[i * Q + c] + ch.normal(i);
    if (hasL) {
#pragma unroll
        for (int r = 0; r < Q; ++r) t0 -= a.Vf[(i * Q + r) * Q + c] * xl[r];
    }
    rd = 1.0 / a.Lf[(i * Q + c) * Q + c];                           // (its own load: picking lc[c] by lane would put lc into private memory)
}

// the way back over interior [i0, i1]: xl the left separator's draw (zeros without one), xn the draw of block i1 + 1 (zeros without one).
// FINAL: the bins go to S where ok, else to X.
template <int Q, int G, bool L0, bool FINAL>
__device__ __forceinline__ void ar_backward(const ArChain<Q, L0>& ch, long i0, long i1, bool hasL, bool writer, bool ok, double (&xl)[Q],
                                            double (&xn)[Q]) {
    const ArArgs& a = ch.a;
    const int c = ch.c;
    double lc[Q], wc[Q], rd, t0;
    if (i0 <= i1) ar_fetch<Q, L0>(ch, i1, hasL, xl, lc, wc, rd, t0);
    for (long i = i1; i >= i0; --i) {
        double lcn[Q], wcn[Q], rdn = 0.0, t0n = 0.0;
        if (i > i0) ar_fetch<Q, L0>(ch, i - 1, hasL, xl, lcn, wcn, rdn, t0n);               // the next bin's loads fly while this one is solved
        double t = t0;
#pragma unroll
        for (int r = 0; r < Q; ++r) t -= wc[r] * xn[r];             // (W_i' x_{i+1})[c]
        double mine = 0.0;
#pragma unroll
        for (int k = Q - 1; k >= 0; --k) {                          // L_i' x = t: lane k finishes entry k
            double s = t;
#pragma unroll
            for (int m = k + 1; m < Q; ++m) s -= lc[m] * xn[m];
            s *= rd;
            mine = c == k ? s : mine;
            xn[k] = ar_bc<G>(s, k);
        }
        if (writer) {
            const long tb = ch.bin(i);
            if (FINAL) {
                if (ok) a.S[tb * a.lds + a.col0 + c] = mine;
            } else {
                a.X[tb * Q + c] = mine;
            }
        }
        if (i > i0) {
#pragma unroll
            for (int m = 0; m < Q; ++m) { lc[m] = lcn[m]; wc[m] = wcn[m]; }
            rd = rdn; t0 = t0n;
        }
    }
}

template <int Q>
struct ArGroup {
    static constexpr int G = Q <= 1 ? 1 : Q <= 2 ? 2 : Q <= 4 ? 4 : 8;
};

template <int Q, bool L0>
__global__ __launch_bounds__(AR_BLOCK) void ar_reduce_kernel(ArArgs a) {
    constexpr int G = ArGroup<Q>::G;
    const long tid = (long)blockIdx.x * AR_BLOCK + threadIdx.x;
    const long gi = tid / G, ns = a.n / a.seg;                      // groups 0 .. ns; separators 0 .. ns - 1
    if (gi > ns) return;
    const int lane = (int)(tid % G), c = lane < Q ? lane : Q - 1;
    const bool writer = lane < Q, hasL = gi >= 1, hasR = gi < ns;
    const ArChain<Q, L0> ch(a, c);
    const long i0 = gi * a.seg, i1 = hasR ? i0 + a.seg - 2 : (long)a.n - 1;
    double d[Q], g[Q], f[Q], accD[Q], acch = 0.0;
    bool bad = false;
#pragma unroll
    for (int m = 0; m < Q; ++m) accD[m] = 0.0;
    if (i0 <= i1) ar_forward<Q, G, L0>(ch, i0, i1, hasL, writer, d, g, f, accD, acch, bad);
    if (bad && lane == 0) atomicOr(a.status, 1);
    if (!writer) return;
    if (hasR) {                                                     // separator gi: its left partial, and E' towards separator gi - 1
        double* o = a.nDL + (gi * Q + c) * Q;
#pragma unroll
        for (int m = 0; m < Q; ++m) o[m] = d[m];
        a.nhL[gi * Q + c] = ar_pick<Q>(g, c);
        if (hasL) {
            double* e = a.nE + ((gi - 1) * Q + c) * Q;
#pragma unroll
            for (int m = 0; m < Q; ++m) e[m] = f[m];
        }
    }
    if (hasL) {                                                     // separator gi - 1: its right partial
        double* o = a.nDR + ((gi - 1) * Q + c) * Q;
#pragma unroll
        for (int m = 0; m < Q; ++m) o[m] = accD[m];
        a.nhR[(gi - 1) * Q + c] = acch;
    }
}

template <int Q, bool L0>
__global__ __launch_bounds__(AR_BLOCK) void ar_base_kernel(ArArgs a) {
    constexpr int G = ArGroup<Q>::G;
    const int lane = threadIdx.x, c = lane < Q ? lane : Q - 1;
    const bool active = lane < G, writer = lane < Q;
    bool bad = false;
    if (active) {
        const ArChain<Q, L0> ch(a, c);
        double d[Q], g[Q], f[Q], accD[Q], acch = 0.0;
        ar_forward<Q, G, L0>(ch, 0, (long)a.n - 1, false, writer, d, g, f, accD, acch, bad);
        if (bad && lane == 0) atomicOr(a.status, 1);
    }
    __threadfence();
    __syncthreads();                                                // the way back reads what the other lanes of the group wrote
    if (active) {
        const ArChain<Q, L0> ch(a, c);
        const bool ok = L0 && !bad && __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
        double xl[Q], xn[Q];
#pragma unroll
        for (int m = 0; m < Q; ++m) xl[m] = xn[m] = 0.0;
        ar_backward<Q, G, L0, L0>(ch, 0, (long)a.n - 1, false, writer, ok, xl, xn);
    }
}

template <int Q, bool L0>
__global__ __launch_bounds__(AR_BLOCK) void ar_expand_kernel(ArArgs a) {
    constexpr int G = ArGroup<Q>::G;
    const long tid = (long)blockIdx.x * AR_BLOCK + threadIdx.x;
    const long gi = tid / G, ns = a.n / a.seg;
    if (gi > ns) return;
    const int lane = (int)(tid % G), c = lane < Q ? lane : Q - 1;
    const bool writer = lane < Q, hasL = gi >= 1, hasR = gi < ns;
    const ArChain<Q, L0> ch(a, c);
    const long i0 = gi * a.seg, i1 = hasR ? i0 + a.seg - 2 : (long)a.n - 1;
    const bool ok = L0 && __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
    double xl[Q], xn[Q];
#pragma unroll
    for (int m = 0; m < Q; ++m) {
        xl[m] = hasL ? a.X[ch.bin(i0 - 1) * Q + m] : 0.0;
        xn[m] = hasR ? a.X[ch.bin(i1 + 1) * Q + m] : 0.0;
    }
    if (L0 && hasR && writer && ok) {                               // the right separator's draw goes out with its left segment
        const long tb = ch.bin(i1 + 1);
        a.S[tb * a.lds + a.col0 + c] = a.X[tb * Q + c];
    }
    ar_backward<Q, G, L0, L0>(ch, i0, i1, hasL, writer, ok, xl, xn);
}

// the level structure, from T and seg alone
struct ArPlan {
    int levels;                                                     // reduce launches; chain `levels` is the base
    long n[AR_MAX_LEVELS], stride[AR_MAX_LEVELS];
    size_t off_L[AR_MAX_LEVELS], off_W[AR_MAX_LEVELS], off_V[AR_MAX_LEVELS], off_y[AR_MAX_LEVELS];
    size_t off_DL[AR_MAX_LEVELS], off_DR[AR_MAX_LEVELS], off_hL[AR_MAX_LEVELS], off_hR[AR_MAX_LEVELS], off_E[AR_MAX_LEVELS];
    size_t off_X, doubles;
};

bool ar_plan(int T, int Q, int seg, ArPlan& p) {
    if (T < 0 || Q < 1 || Q > PGL_LATENT_MAX || seg < 2) return false;
    const size_t QQ = (size_t)Q * Q;
    size_t at = 0;
    long n = T, stride = 1;
    int k = 0;
    for (;; ++k) {
        if (k >= AR_MAX_LEVELS) return false;
        p.n[k] = n; p.stride[k] = stride;
        const bool base = n < 2L * seg;
        p.off_L[k] = at; at += (size_t)n * QQ;
        p.off_W[k] = at; at += (size_t)n * QQ;
        p.off_V[k] = at; at += base ? 0 : (size_t)n * QQ;
        p.off_y[k] = at; at += (size_t)n * Q;
        if (k) {
            p.off_DL[k] = at; at += (size_t)n * QQ;
            p.off_DR[k] = at; at += (size_t)n * QQ;
            p.off_E[k] = at; at += (size_t)n * QQ;
            p.off_hL[k] = at; at += (size_t)n * Q;
            p.off_hR[k] = at; at += (size_t)n * Q;
        }
        if (base) break;
        n /= seg;
        stride *= seg;
    }
    p.levels = k;
    p.off_X = at; at += (size_t)T * Q;
    p.doubles = at;
    return true;
}

void ar_level(ArArgs& a, const ArPlan& p, int k, int seg, double* sc) {
    const bool base = k == p.levels;
    a.n = (int)p.n[k]; a.seg = seg; a.stride = p.stride[k];
    a.Lf = sc + p.off_L[k]; a.Wf = sc + p.off_W[k]; a.Vf = base ? nullptr : sc + p.off_V[k]; a.yf = sc + p.off_y[k];
    a.DL = a.DR = a.hL = a.hR = a.E = nullptr;
    if (k) { a.DL = sc + p.off_DL[k]; a.DR = sc + p.off_DR[k]; a.hL = sc + p.off_hL[k]; a.hR = sc + p.off_hR[k]; a.E = sc + p.off_E[k]; }
    a.nDL = a.nDR = a.nhL = a.nhR = a.nE = nullptr;
    if (!base) {
        a.nDL = sc + p.off_DL[k + 1]; a.nDR = sc + p.off_DR[k + 1]; a.nhL = sc + p.off_hL[k + 1]; a.nhR = sc + p.off_hR[k + 1];
        a.nE = sc + p.off_E[k + 1];
    }
}

template <int Q>
int ar_run(ArArgs a, const ArPlan& p, int seg, double* sc, hipStream_t st) {
    constexpr int G = ArGroup<Q>::G;
    auto grid = [&](int k) { return dim3((unsigned)(((p.n[k] / seg + 1) * G + AR_BLOCK - 1) / AR_BLOCK)); };
    for (int k = 0; k < p.levels; ++k) {
        ar_level(a, p, k, seg, sc);
        if (k == 0) hipLaunchKernelGGL((ar_reduce_kernel<Q, true>), grid(k), dim3(AR_BLOCK), 0, st, a);
        else hipLaunchKernelGGL((ar_reduce_kernel<Q, false>), grid(k), dim3(AR_BLOCK), 0, st, a);
        PGL_CHECK_LAUNCH();
    }
    ar_level(a, p, p.levels, seg, sc);
    if (p.levels == 0) hipLaunchKernelGGL((ar_base_kernel<Q, true>), dim3(1), dim3(AR_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((ar_base_kernel<Q, false>), dim3(1), dim3(AR_BLOCK), 0, st, a);
    PGL_CHECK_LAUNCH();
    for (int k = p.levels - 1; k >= 0; --k) {
        ar_level(a, p, k, seg, sc);
        if (k == 0) hipLaunchKernelGGL((ar_expand_kernel<Q, true>), grid(k), dim3(AR_BLOCK), 0, st, a);
        else hipLaunchKernelGGL((ar_expand_kernel<Q, false>), grid(k), dim3(AR_BLOCK), 0, st, a);
        PGL_CHECK_LAUNCH();
    }
    return PGL_OK;
}

}  // namespace

extern "C" int pgl_latent_ar_seg(void) { return AR_SEG_DEFAULT; }

extern "C" size_t pgl_latent_ar_scratch(int T, int Q, int seg) {
    ArPlan p;
    if (!ar_plan(T, Q, seg == 0 ? AR_SEG_DEFAULT : seg, p)) return 0;
    return p.doubles * sizeof(double);
}

extern "C" int pgl_latent_ar_draw(const double* Lambda, const double* r, const double* phi, const double* z_override, uint64_t seed, uint64_t sweep,
                                  uint64_t elem0, double* S, long lds, int col0, int* status, int T, int Q, int seg, void* scratch,
                                  size_t scratch_bytes, void* hip_stream) {
    PGL_CHECK_ARG(Q >= 1 && Q <= PGL_LATENT_MAX && T >= 0 && col0 >= 0 && lds >= (long)col0 + Q && status && phi);
    PGL_CHECK_ARG(seg == 0 || seg >= 2);
    for (int q = 0; q < Q; ++q) PGL_CHECK_ARG(phi[q] >= 0.0 && phi[q] < 1.0);
    PGL_CHECK_ARG(T == 0 || (Lambda && r && S));
    if (T == 0) return PGL_OK;
    if (seg == 0) seg = AR_SEG_DEFAULT;
    ArPlan p;
    PGL_CHECK_ARG(ar_plan(T, Q, seg, p));
    PGL_CHECK_ARG(scratch && scratch_bytes >= p.doubles * sizeof(double) && ((uintptr_t)scratch & 7) == 0);
    ArArgs a;
    a.Lambda = Lambda; a.r = r; a.zo = z_override;
    for (int q = 0; q < PGL_LATENT_MAX; ++q) {
        const double f = q < Q ? phi[q] : 0.0, s = 1.0 - f * f;
        a.dmid[q] = (1.0 + f * f) / s; a.dend[q] = 1.0 / s; a.e[q] = -f / s;
    }
    a.seed = seed; a.sweep = sweep; a.elem0 = elem0; a.T = T;
    a.X = static_cast<double*>(scratch) + p.off_X;
    a.S = S; a.lds = lds; a.col0 = col0; a.status = status;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    double* sc = static_cast<double*>(scratch);
    switch (Q) {
        case 1: return ar_run<1>(a, p, seg, sc, st);
        case 2: return ar_run<2>(a, p, seg, sc, st);
        case 3: return ar_run<3>(a, p, seg, sc, st);
        case 4: return ar_run<4>(a, p, seg, sc, st);
        case 5: return ar_run<5>(a, p, seg, sc, st);
        case 6: return ar_run<6>(a, p, seg, sc, st);
        case 7: return ar_run<7>(a, p, seg, sc, st);
        default: return ar_run<8>(a, p, seg, sc, st);
    }
}
