// Time-rescaling goodness of fit of a recording under the fitted rates (Brown et al. 2002; in discrete time: Haslinger, Pipa & Brown 2010):
// per neuron the intensity q[t] = par * log1p(exp(psi[t])) = -log P(y[t] = 0) summed between consecutive events (Y > 0) is Exp(1) under
// the model, so z = 1 - exp(-xi) is uniform; the fold leaves the histogram of z on [0, 1) and (sum z, sum z^2) per neuron, pgl_rescale_ks the
// binned Kolmogorov-Smirnov statistic (pyglm_amd/rescale.py: rescale_host and ks_binned state the definition).  DESIGN.md section 14.
//
// A segmented floating-point sum along time, cut at every event, parallel in time as the inter-spike intervals are (pgl_isi.hip), on the
// split, the LDS histogram and the records of pgl_timescan.h:
//   rescale_scan_kernel    one workgroup = TS_SEG rows of time of 64 columns; lane = column, so a wave reads 512 contiguous bytes of Psi and
//                          of Y per row.  Each of the 4 waves walks its TS_WAVE_ROWS rows in time order, eight rows' loads in flight: q of the
//                          eight rows and the running sum in front of each come branch-free; then the lanes that have events in those
//                          rows take them one at a time (the loop runs as often as the busiest lane has events, not once per row): the
//                          uniform of the event's cell (Philox, evaluated at event cells only), delta, and -- unless it is the wave's first
//                          event -- the interval's z, which goes to the workgroup's histogram in LDS and to the lane's sum z, sum z^2.
//                          Behind the barrier wave 0 closes the intervals that cross the waves and writes the segment's record to `work`,
//                          doubles: first-event row or -1; the sum up to and including delta of the first event (without an event: the
//                          segment's whole sum); the sum behind the last event; sum z, sum z^2.  The workgroup then adds its histogram to
//                          hist.
//   rescale_stitch_kernel  one thread per column walks the records in time order, closes the intervals that cross segments (through any
//                          number of segments without an event; the eight expm1 of a batch side by side) and alone writes zsum.
// No floating-point atomics: every floating sum is formed by one thread in an order fixed by T and the split, so a column's result has the
// same bits whatever nloc, neuron0 or the shard; the histogram adds integers only.
#include "pgl_timescan.h"
#include "pgl_rng.h"

namespace {

// a record: first, head, tail, sum z, sum z^2

struct RsArgs {
    const double* Psi; long ldn; const double* bias; const double* Y;
    int T, nloc; const double* qpar; double qpar0; int D;
    uint32_t k0, k1, c0;                              // Philox key and counter word 0 (draw | purpose << 24)
    uint64_t neuron0, elem0;
};

// bin min(D - 1, (int)(z D)) of z
__device__ __forceinline__ int rs_bin(double z, int D) {
    const int b = (int)(z * (double)D);
    return b < 0 ? 0 : (b > D - 1 ? D - 1 : b);
}

// the interval whose rescaled length is x: its z to its bin of the histogram row h and to (sz, sz2)
__device__ __forceinline__ void rs_close(double x, int* h, int D, bool atomic, double& sz, double& sz2) {
    const double z = -expm1(-x);
    const int b = rs_bin(z, D);
    if (atomic) atomicAdd(h + b, 1); else h[b] += 1;
    sz += z; sz2 += z * z;
}

// delta of the event of local column n at row t, whose cell has -log P(y = 0) = q: the part of that bin in front of the event, drawn from the
// exponential law cut at q with the first uniform of the cell's Philox call
__device__ __forceinline__ double rs_delta(const RsArgs& a, double q, int n, int t) {
    const uint64_t stream = a.neuron0 + (uint64_t)n;
    uint32_t o0, o1, o2, o3;
    pgl_philox4x32_10(a.c0, (uint32_t)(a.elem0 + (uint64_t)t), (uint32_t)stream, (uint32_t)(stream >> 32), a.k0, a.k1, o0, o1, o2, o3);
    const double r = pgl_u64_to_unit((uint64_t)o0 | ((uint64_t)o1 << 32));
    return -log1p(-r * (-expm1(-q)));
}

__global__ __launch_bounds__(256) void rescale_scan_kernel(RsArgs a, int* __restrict__ hist, double* __restrict__ rec, long recStride) {
    extern __shared__ int hs[];
    __shared__ TsWaveRecs<double> wrec;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = blockIdx.x, n0 = blockIdx.y * 64;
    const int n = n0 + lane, D = a.D;
    int* h = ts_hist_begin(hs, D);
    double run = 0.0, head = 0.0, sz = 0.0, sz2 = 0.0;             // run: the sum since the column's last event (or the wave's first row)
    int first = -1;
    const int u0 = seg * TS_SEG + wave * TS_WAVE_ROWS, u1 = min(a.T, u0 + TS_WAVE_ROWS);
    if (n < a.nloc) {
        const double bn = a.bias ? a.bias[n] : 0.0, par = a.qpar ? a.qpar[n] : a.qpar0;
        const double* pp = a.Psi + n;
        const double* py = a.Y + n;
        for (int u = u0; u < u1; u += TS_BATCH) {
            double q[TS_BATCH], pre[TS_BATCH];
            unsigned ev = 0;
#pragma unroll
            for (int k = 0; k < TS_BATCH; ++k) {
                const bool in = u + k < u1;
                q[k] = in ? pp[(long)(u + k) * a.ldn] : 0.0;
                pre[k] = in ? py[(long)(u + k) * a.ldn] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < TS_BATCH; ++k) {
                const bool in = u + k < u1, e = pre[k] > 0.0;      // (NaN and negative values compare false; rows past the end hold 0)
                q[k] = in ? par * log1p(exp(q[k] + bn)) : 0.0;
                ev |= e ? 1u << k : 0u;
                pre[k] = run;
                run = e ? 0.0 : run + q[k];
            }
            while (ev) {                                           // this lane's events of the eight rows, in time order
                const int k = __ffs(ev) - 1;
                ev &= ev - 1;
                double qe = q[0], pe = pre[0];
#pragma unroll
                for (int j = 1; j < TS_BATCH; ++j) { qe = k == j ? q[j] : qe; pe = k == j ? pre[j] : pe; }
                const double x = pe + rs_delta(a, qe, n, u + k);
                if (first >= 0) rs_close(x, h, D, true, sz, sz2);
                else { first = u + k; head = x; }
            }
        }
        if (first < 0) head = run;
    }
    wrec.put(wave, lane, (double)first, head, run, sz, sz2);
    __syncthreads();
    if (wave == 0 && n < a.nloc) {                                 // the other waves add nothing to hs any more
        double acc = 0.0, shead = 0.0, ssz = 0.0, ssz2 = 0.0;
        int sfirst = -1;
        for (int w = 0; w < TS_WAVES; ++w) {
            const double f = wrec.v[0][w][lane], hd = wrec.v[1][w][lane];
            if (f < 0.0) { acc += hd; continue; }
            const double x = acc + hd;
            if (sfirst >= 0) rs_close(x, h, D, false, ssz, ssz2);
            else { sfirst = (int)f; shead = x; }
            ssz += wrec.v[3][w][lane]; ssz2 += wrec.v[4][w][lane];
            acc = wrec.v[2][w][lane];
        }
        if (sfirst < 0) shead = acc;
        ts_put_record(rec, recStride, seg, a.nloc, n, (double)sfirst, shead, acc, ssz, ssz2);
    }
    __syncthreads();
    ts_hist_flush(hs, D, hist + (long)n0 * D, a.nloc - n0);
}

__global__ __launch_bounds__(256) void rescale_stitch_kernel(const double* __restrict__ rec, long recStride, int nseg, int nloc, int D,
                                                             int* __restrict__ hist, double* __restrict__ zsum, int accumulate) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nloc) return;
    double acc = 0.0, Z1 = 0.0, Z2 = 0.0;
    bool has = false;
    int* h = hist + (long)i * D;
    for (int s0 = 0; s0 < nseg; s0 += TS_BATCH) {
        double v[TS_REC][TS_BATCH];
        ts_get_records(rec, recStride, s0, nseg, nloc, i, v);
        // the walk proper is a few adds per segment; the eight expm1 behind it do not depend on each other and are evaluated side by side
        double x[TS_BATCH];
        unsigned ev = 0, cl = 0;
#pragma unroll
        for (int k = 0; k < TS_BATCH; ++k) {
            const bool e = !(v[0][k] < 0.0);
            x[k] = acc + v[1][k];                                  // without an event: the segment's whole sum joins (past the end: + 0)
            ev |= e ? 1u << k : 0u;
            cl |= e && has ? 1u << k : 0u;                         // (the stretch in front of the column's first event is dropped)
            has = has || e;
            acc = e ? v[2][k] : x[k];
        }
#pragma unroll
        for (int k = 0; k < TS_BATCH; ++k) x[k] = -expm1(-x[k]);
#pragma unroll
        for (int k = 0; k < TS_BATCH; ++k) {
            if (cl >> k & 1u) {
                atomicAdd(h + rs_bin(x[k], D), 1);                 // (no value comes back: the walk does not wait for it)
                Z1 += x[k]; Z2 += x[k] * x[k];
            }
            if (ev >> k & 1u) { Z1 += v[3][k]; Z2 += v[4][k]; }
        }
    }
    zsum[2 * i] = accumulate ? zsum[2 * i] + Z1 : Z1;
    zsum[2 * i + 1] = accumulate ? zsum[2 * i + 1] + Z2 : Z2;
}

// one thread per neuron: the binned KS statistic of its histogram, in 64-bit integers up to the one division
__global__ __launch_bounds__(256) void rescale_ks_kernel(const int* __restrict__ hist, int nloc, int D, double coef, double* __restrict__ ks,
                                                         double* __restrict__ mean, double* __restrict__ M2, int* __restrict__ exceed,
                                                         long long* __restrict__ hsum, int k) {
#pragma clang fp contract(off)                                     // the Welford step rounds as summary._welford does, operation by operation
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= nloc) return;
    const int* h = hist + (long)n * D;
    long long M = 0, C = 0, best = 0;
    for (int d = 0; d < D; ++d) { M += h[d]; hsum[(long)n * D + d] += h[d]; }
    for (int d = 1; d < D; ++d) {
        C += h[d - 1];
        long long v = C * D - d * M;
        v = v < 0 ? -v : v;
        best = v > best ? v : best;
    }
    const double x = M > 0 ? (double)best / (double)(M * D) : __longlong_as_double(0x7ff8000000000000LL);
    ks[n] = x;
    const double m0 = mean[n], dlt = x - m0, m1 = m0 + dlt / (double)k;
    mean[n] = m1;
    M2[n] += dlt * (x - m1);
    if (M > 0 && x > coef / sqrt((double)M)) exceed[n] += 1;
}

PglPerDeviceSize rs_lds_set;

}  // namespace

int pgl_rescale_segment_rows(void) { return TS_SEG; }

size_t pgl_rescale_work_bytes(int nloc, int T) {
    if (nloc < 1 || T < 0) return 0;
    return ts_work_bytes(sizeof(double), nloc, T);
}

int pgl_rescale_fold(const double* Psi, long ldn, const double* bias, const double* Y, int T, int nloc, const double* qpar, double qpar0, int D,
                     uint64_t seed, uint32_t draw, uint64_t neuron0, uint64_t elem0, int* hist, double* zsum, int accumulate, void* work,
                     void* hip_stream) {
    PGL_CHECK_ARG(D >= 2 && D <= PGL_RESCALE_MAX_BINS && nloc >= 1 && T >= 0 && ldn >= nloc && hist && zsum);
    PGL_CHECK_ARG(accumulate == 0 || accumulate == 1);
    PGL_CHECK_ARG(T == 0 || (Psi && Y && work && ((uintptr_t)work % 8) == 0));
    PGL_CHECK_ARG(((long)nloc + 63) / 64 <= 65535 && T <= 2147483647 - TS_SEG);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!accumulate && (hipMemsetAsync(hist, 0, (size_t)nloc * D * sizeof(int), st) != hipSuccess ||
                        (T == 0 && hipMemsetAsync(zsum, 0, (size_t)nloc * 2 * sizeof(double), st) != hipSuccess))) {
        pgl_set_error("pgl_rescale_fold: hipMemsetAsync failed");
        return PGL_ERR_HIP;
    }
    if (T == 0) return PGL_OK;
    RsArgs a;
    a.Psi = Psi; a.ldn = ldn; a.bias = bias; a.Y = Y; a.T = T; a.nloc = nloc; a.qpar = qpar; a.qpar0 = qpar0; a.D = D;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.c0 = (draw & 0xFFFFFFu) | (PGL_PURPOSE_RESCALE << 24);
    a.neuron0 = neuron0; a.elem0 = elem0;
    const long nseg = ts_segments(T), recStride = nseg * nloc;
    double* rec = static_cast<double*>(work);
    const size_t lds = ts_hist_lds_bytes(D);
    if (int rc = pgl_grow_dynamic_lds(reinterpret_cast<const void*>(rescale_scan_kernel), lds, rs_lds_set)) return rc;
    hipLaunchKernelGGL(rescale_scan_kernel, dim3((unsigned)nseg, (unsigned)((nloc + 63) / 64)), dim3(256), lds, st, a, hist, rec, recStride);
    PGL_CHECK_LAUNCH();
    hipLaunchKernelGGL(rescale_stitch_kernel, dim3((unsigned)((nloc + 255) / 256)), dim3(256), 0, st, rec, recStride, (int)nseg, nloc, D, hist, zsum,
                       accumulate);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}

int pgl_rescale_ks(const int* hist, int nloc, int D, double coef, double* ks, double* ks_mean, double* ks_M2, int* exceed, long long* hist_sum, int k,
                   void* hip_stream) {
    PGL_CHECK_ARG(hist && ks && ks_mean && ks_M2 && exceed && hist_sum && nloc >= 1 && D >= 2 && D <= PGL_RESCALE_MAX_BINS && k >= 1);
    hipLaunchKernelGGL(rescale_ks_kernel, dim3((unsigned)((nloc + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(hip_stream), hist, nloc, D, coef,
                       ks, ks_mean, ks_M2, exceed, hist_sum, k);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}
