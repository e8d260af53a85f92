// Inter-spike intervals of spike trains: per column (replicate, neuron) the histogram of the distances between consecutive events (Y > 0) and
// the exact moments (M, sum d, sum d^2) of those distances -- the single-train statistic of the posterior predictive check
// (pyglm_amd/simulate.py: isi_host states the definition).  DESIGN.md section 13.
//
// The scan over time is parallel in time, on the split, the LDS histogram and the records of pgl_timescan.h:
//   isi_scan_kernel     one workgroup = TS_SEG rows of time of 64 columns of one replicate; lane = column, so a wave reads 512 contiguous bytes per
//                       row.  Each of the 4 waves walks its TS_WAVE_ROWS rows: an interval between two events of its own rows goes to the
//                       workgroup's histogram in LDS and to three per-lane counters; the wave leaves (first event, last event, M, sum d,
//                       sum d^2).  Behind the workgroup's barrier wave 0 closes the intervals that cross the waves' boundaries and writes the
//                       segment's record to `work` -- ints; inside a segment d <= 255, so its moments fit an int -- and the workgroup adds
//                       its histogram to hist.
//   isi_stitch_kernel   one thread per column walks the segments' records in time order: it sums the moments in 64 bits, closes the intervals
//                       that cross segment boundaries and the chunk boundary (`since`), skipping every segment without an event, and leaves
//                       the new `since`.  It alone writes moments and since, and hist after the scan kernel has finished.
// Both joins -- of the waves' records and of the segments' -- are isi_join.  Everything added is an integer: the result does not depend on the
// order of the atomics.
#include "pgl_timescan.h"

namespace {

// a stretch of time of one column: whether it has an event, the rows of its first and last event, and M, sum d, sum d^2 of the intervals
// closed inside; I: int inside a segment, long long along a column
template <class I> struct IsiCount {
    bool has = false;
    I first = -1, last = -1, M = 0, sd = 0, sd2 = 0;
};

// the event at row u of a column whose histogram row is h
template <class I> __device__ __forceinline__ void isi_event(IsiCount<I>& c, I u, int* h, int D, bool atomic) {
    if (c.has) {
        const I d = u - c.last;
        c.M += 1; c.sd += d; c.sd2 += d * d;
        int* cell = h + (d < D ? (int)d : D) - 1;
        if (atomic) atomicAdd(cell, 1); else *cell += 1;
    } else {
        c.first = u;
    }
    c.last = u; c.has = true;
}

// the stretch behind c, of record (first, last, M, sd, sd2): without an event there is nothing to close and nothing to add; with one, the
// interval from c's last event to its first closes, and its own counts add
template <class I> __device__ __forceinline__ void isi_join(IsiCount<I>& c, int first, int last, int M, int sd, int sd2, int* h, int D, bool atomic) {
    if (first < 0) return;
    isi_event(c, (I)first, h, D, atomic);
    c.last = last; c.M += M; c.sd += sd; c.sd2 += sd2;
}

__global__ __launch_bounds__(256) void isi_scan_kernel(const double* __restrict__ Y, long ldy, long strideY, int rows, int N, int D,
                                                       int* __restrict__ hist, int* __restrict__ rec, long recStride) {
    extern __shared__ int hs[];
    __shared__ TsWaveRecs<int> wrec;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = blockIdx.x, n0 = blockIdx.y * 64, r = blockIdx.z;
    const int n = n0 + lane;
    int* h = ts_hist_begin(hs, D);
    IsiCount<int> c;
    const int u0 = seg * TS_SEG + wave * TS_WAVE_ROWS, u1 = min(rows, u0 + TS_WAVE_ROWS);
    if (n < N) {
        const double* p = Y + (long)r * strideY + n;
        for (int u = u0; u < u1; u += TS_BATCH) {
            double v[TS_BATCH];
#pragma unroll
            for (int k = 0; k < TS_BATCH; ++k) v[k] = u + k < u1 ? p[(long)(u + k) * ldy] : 0.0;
#pragma unroll
            for (int k = 0; k < TS_BATCH; ++k)
                if (v[k] > 0.0) isi_event(c, u + k, h, D, true);      // (NaN and negative values compare false)
        }
    }
    wrec.put(wave, lane, c.first, c.last, c.M, c.sd, c.sd2);
    __syncthreads();
    if (wave == 0 && n < N) {                                      // the other waves add nothing to hs any more
        IsiCount<int> s;
        for (int w = 0; w < TS_WAVES; ++w)
            isi_join(s, wrec.v[0][w][lane], wrec.v[1][w][lane], wrec.v[2][w][lane], wrec.v[3][w][lane], wrec.v[4][w][lane], h, D, false);
        ts_put_record(rec, recStride, seg, (long)gridDim.z * N, (long)r * N + n, s.first, s.last, s.M, s.sd, s.sd2);
    }
    __syncthreads();
    ts_hist_flush(hs, D, hist + ((long)r * N + n0) * D, N - n0);
}

__global__ __launch_bounds__(256) void isi_stitch_kernel(const int* __restrict__ rec, long recStride, int nseg, int rows, long RN, int D,
                                                         int* __restrict__ hist, long long* __restrict__ moments, int* __restrict__ since,
                                                         int accumulate) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= RN) return;
    IsiCount<long long> c;                                         // the column up to this chunk: `since` is its last event
    if (accumulate) {
        const int sn = since[i];
        c.M = moments[3 * i]; c.sd = moments[3 * i + 1]; c.sd2 = moments[3 * i + 2];
        c.has = sn >= 0; c.last = -1 - (long long)sn;              // relative to the chunk, so negative: `has` cannot be read off the row
    }
    int* h = hist + i * D;
    for (int s0 = 0; s0 < nseg; s0 += TS_BATCH) {
        int v[TS_REC][TS_BATCH];
        ts_get_records(rec, recStride, s0, nseg, RN, i, v);
#pragma unroll
        for (int k = 0; k < TS_BATCH; ++k)                         // (no value comes back from the atomic: the walk does not wait for it)
            isi_join(c, v[0][k], v[1][k], v[2][k], v[3][k], v[4][k], h, D, true);
    }
    moments[3 * i] = c.M; moments[3 * i + 1] = c.sd; moments[3 * i + 2] = c.sd2;
    since[i] = c.has ? (int)(rows - 1 - c.last) : -1;
}

PglPerDeviceSize isi_lds_set;

}  // namespace

int pgl_isi_segment_rows(void) { return TS_SEG; }

size_t pgl_isi_work_bytes(int N, int R, int rows) {
    if (N < 1 || R < 1 || rows < 0) return 0;
    return ts_work_bytes(sizeof(int), (long)R * N, rows);
}

int pgl_isi_fold(const double* Y, long ldy, long strideY, int rows, int N, int R, int D, int* hist, long long* moments, int* since, int accumulate,
                 void* work, void* hip_stream) {
    PGL_CHECK_ARG(D >= 2 && D <= PGL_ISI_MAX_BINS && N >= 1 && R >= 1 && rows >= 0 && ldy >= N && hist && moments && since);
    PGL_CHECK_ARG(accumulate == 0 || accumulate == 1);
    PGL_CHECK_ARG(rows == 0 || (Y && work && ((uintptr_t)work % 4) == 0));
    PGL_CHECK_ARG(((long)N + 63) / 64 <= 65535 && R <= 65535);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const long RN = (long)R * N, nseg = ts_segments(rows);
    if (!accumulate && hipMemsetAsync(hist, 0, (size_t)RN * D * sizeof(int), st) != hipSuccess) {
        pgl_set_error("pgl_isi_fold: hipMemsetAsync failed");
        return PGL_ERR_HIP;
    }
    int* rec = static_cast<int*>(work);
    const long recStride = nseg * RN;
    if (rows > 0) {
        const size_t lds = ts_hist_lds_bytes(D);
        if (int rc = pgl_grow_dynamic_lds(reinterpret_cast<const void*>(isi_scan_kernel), lds, isi_lds_set)) return rc;
        hipLaunchKernelGGL(isi_scan_kernel, dim3((unsigned)nseg, (unsigned)((N + 63) / 64), (unsigned)R), dim3(256), lds, st, Y, ldy, strideY, rows, N,
                           D, hist, rec, recStride);
        PGL_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(isi_stitch_kernel, dim3((unsigned)((RN + 255) / 256)), dim3(256), 0, st, rec, recStride, (int)nseg, rows, RN, D, hist, moments,
                       since, accumulate);
    PGL_CHECK_LAUNCH();
    return PGL_OK;
}
