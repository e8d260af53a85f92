// Inter-spike intervals of spike trains: per column (replicate, neuron) the histogram of the distances between consecutive events (Y > 0) and
// the exact moments (M, sum d, sum d^2) of those distances -- the single-train statistic of the posterior predictive check
// (pyglm_amd/simulate.py: isi_host states the definition).  DESIGN.md section 13.
//
// The scan over time is parallel in time:
//   isi_scan_kernel     one workgroup = ISI_SEG rows of time of 64 columns of one replicate; lane = column, so a wave reads 512 contiguous bytes per
//                       row.  Each of the 4 waves walks its ISI_WAVE_ROWS rows: an interval between two events of its own rows goes to the
//                       workgroup's histogram in LDS ([column][D | 1] ints: the lanes of a wave that add to the same bin fall in 64 different
//                       banks, so the column in which every bin is an event costs what any other costs) and to three per-lane counters; the
//                       wave leaves (first event, last event, M, sum d, sum d^2).  Behind the workgroup's barrier wave 0 closes the intervals that
//                       cross the waves' boundaries, writes the segment's record to `work` -- [5][segments][R N] ints; inside a segment d <= 255,
//                       so its moments fit an int -- and the workgroup adds the non-zero cells of its histogram to hist with integer atomics
//                       (thread -> consecutive bins of one column: contiguous addresses).
//   isi_stitch_kernel   one thread per column walks the segments' records in time order, eight segments' loads in flight: it sums the moments in 64 bits,
//                       closes the intervals that cross segment boundaries and the chunk boundary (`since`), skipping every segment without an
//                       event, and leaves the new `since`.  It alone writes moments and since, and hist after the scan kernel has finished.
// Everything added is an integer: the result does not depend on the order of the atomics.
#include "pgl_common.h"

namespace {

constexpr int ISI_WAVES = 4;
constexpr int ISI_WAVE_ROWS = 64;                       // rows of time one wave walks
constexpr int ISI_SEG = ISI_WAVES * ISI_WAVE_ROWS;      // rows of time one workgroup owns
constexpr int ISI_REC = 5;                              // first, last (rows of the chunk; -1: no event), M, sum d, sum d^2

struct IsiCount {
    int first = -1, last = -1, M = 0, sd = 0, sd2 = 0;
};

// the event at row u of a column whose histogram row is h
__device__ __forceinline__ void isi_event(IsiCount& c, int u, int* h, int D, bool atomic) {
    if (c.last >= 0) {
        const int d = u - c.last;
        c.M += 1; c.sd += d; c.sd2 += d * d;
        int* cell = h + (d < D ? d : D) - 1;
        if (atomic) atomicAdd(cell, 1); else *cell += 1;
    } else {
        c.first = u;
    }
    c.last = u;
}

__global__ __launch_bounds__(256) void isi_scan_kernel(const double* __restrict__ Y, long ldy, long strideY, int rows, int N, int D,
                                                       int* __restrict__ hist, int* __restrict__ rec, long recStride) {
    extern __shared__ int hs[];                                    // [64][Dp]
    __shared__ int wrec[ISI_REC][ISI_WAVES][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = blockIdx.x, n0 = blockIdx.y * 64, r = blockIdx.z;
    const int n = n0 + lane, Dp = D | 1;
    for (int i = tid; i < 64 * Dp; i += 256) hs[i] = 0;
    __syncthreads();
    int* h = hs + lane * Dp;
    IsiCount c;
    const int u0 = seg * ISI_SEG + wave * ISI_WAVE_ROWS, u1 = min(rows, u0 + ISI_WAVE_ROWS);
    if (n < N) {
        const double* p = Y + (long)r * strideY + n;
        for (int u = u0; u < u1; u += 8) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = u + k < u1 ? p[(long)(u + k) * ldy] : 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (v[k] > 0.0) isi_event(c, u + k, h, D, true);      // (NaN and negative values compare false)
        }
    }
    wrec[0][wave][lane] = c.first; wrec[1][wave][lane] = c.last; wrec[2][wave][lane] = c.M; wrec[3][wave][lane] = c.sd; wrec[4][wave][lane] = c.sd2;
    __syncthreads();
    if (wave == 0 && n < N) {                                      // the other waves add nothing to hs any more
        IsiCount s;
        for (int w = 0; w < ISI_WAVES; ++w) {
            const int f = wrec[0][w][lane];
            if (f < 0) continue;
            isi_event(s, f, h, D, false);
            s.last = wrec[1][w][lane];
            s.M += wrec[2][w][lane]; s.sd += wrec[3][w][lane]; s.sd2 += wrec[4][w][lane];
        }
        int* q = rec + (long)seg * ((long)gridDim.z * N) + (long)r * N + n;
        q[0] = s.first; q[recStride] = s.last; q[2 * recStride] = s.M; q[3 * recStride] = s.sd; q[4 * recStride] = s.sd2;
    }
    __syncthreads();
    for (int i = tid; i < 64 * D; i += 256) {
        const int col = i / D, d = i - col * D;
        const int cnt = hs[col * Dp + d];
        if (cnt != 0 && n0 + col < N) atomicAdd(hist + ((long)r * N + n0 + col) * D + d, cnt);
    }
}

__global__ __launch_bounds__(256) void isi_stitch_kernel(const int* __restrict__ rec, long recStride, int nseg, int rows, long RN, int D,
                                                         int* __restrict__ hist, long long* __restrict__ moments, int* __restrict__ since,
                                                         int accumulate) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= RN) return;
    long long M = 0, sd = 0, sd2 = 0;
    int sn = -1;
    if (accumulate) { M = moments[3 * i]; sd = moments[3 * i + 1]; sd2 = moments[3 * i + 2]; sn = since[i]; }
    bool has = sn >= 0;
    long long last = -1 - (long long)sn;                           // row of the column's last event, relative to the chunk
    int* h = hist + i * D;
    for (int s0 = 0; s0 < nseg; s0 += 8) {
        int v[ISI_REC][8];                                         // the records of eight segments, all their loads in flight together
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int j = 0; j < ISI_REC; ++j) v[j][k] = s0 + k < nseg ? rec[j * recStride + (long)(s0 + k) * RN + i] : (j == 0 ? -1 : 0);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (v[0][k] < 0) continue;                             // a segment without an event: nothing to close, nothing to add
            if (has) {
                const long long d = v[0][k] - last;
                M += 1; sd += d; sd2 += d * d;
                atomicAdd(h + (d < D ? (int)d : D) - 1, 1);        // (no value comes back: the walk does not wait for it)
            }
            last = v[1][k]; has = true;
            M += v[2][k]; sd += v[3][k]; sd2 += v[4][k];
        }
    }
    moments[3 * i] = M; moments[3 * i + 1] = sd; moments[3 * i + 2] = sd2;
    since[i] = has ? (int)(rows - 1 - last) : -1;
}

inline long isi_segments(int rows) { return ((long)rows + ISI_SEG - 1) / ISI_SEG; }

PglPerDeviceSize isi_lds_set;

}  // namespace

int pgl_isi_segment_rows(void) { return ISI_SEG; }

size_t pgl_isi_work_bytes(int N, int R, int rows) {
    if (N < 1 || R < 1 || rows < 0) return 0;
    const size_t bytes = (size_t)ISI_REC * (size_t)isi_segments(rows) * (size_t)R * (size_t)N * sizeof(int);
    return bytes < 16 ? 16 : (bytes + 15) & ~(size_t)15;
}

int pgl_isi_fold(const double* Y, long ldy, long strideY, int rows, int N, int R, int D, int* hist, long long* moments, int* since, int accumulate,
                 void* work, void* hip_stream) {
    PGL_CHECK_ARG(D >= 2 && D <= PGL_ISI_MAX_BINS && N >= 1 && R >= 1 && rows >= 0 && ldy >= N && hist && moments && since);
    PGL_CHECK_ARG(accumulate == 0 || accumulate == 1);
    PGL_CHECK_ARG(rows == 0 || (Y && work && ((uintptr_t)work % 4) == 0));
    PGL_CHECK_ARG(((long)N + 63) / 64 <= 65535 && R <= 65535);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const long RN = (long)R * N, nseg = isi_segments(rows);
    if (!accumulate && hipMemsetAsync(hist, 0, (size_t)RN * D * sizeof(int), st) != hipSuccess) {
        pgl_set_error("pgl_isi_fold: hipMemsetAsync failed");
        return PGL_ERR_HIP;
    }
    int* rec = static_cast<int*>(work);
    const long recStride = nseg * RN;
    if (rows > 0) {
        const size_t lds = (size_t)64 * (D | 1) * sizeof(int);
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
