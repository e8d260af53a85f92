// The split of time that the per-column scans share (pgl_isi.hip, pgl_rescale.hip): a workgroup of 256 threads owns
// TS_SEG rows of time of 64 columns, lane = column, and each of its TS_WAVES waves walks TS_WAVE_ROWS of them.  The workgroup's histogram is
// in LDS, [column][D | 1] ints: the lanes of a wave that add to the same bin fall in 64 different banks, so the column in which every row
// adds to one bin costs what any other costs.  Every wave leaves a record of TS_REC values per column in LDS, wave 0 joins the four behind
// the workgroup's barrier, and the segment's record goes to `work`, [TS_REC][segments][columns]; value 0 of a record is the row of the
// stretch's first event, negative without one.  A second launch -- one thread per column, TS_BATCH segments' loads in flight -- stitches
// the segments' records in time order.  What a record's other four values are, and how two stretches join, is each statistic's own.
#pragma once
#include "pgl_common.h"

constexpr int TS_WAVES = 4;
constexpr int TS_WAVE_ROWS = 64;                        // rows of time one wave walks
constexpr int TS_SEG = TS_WAVES * TS_WAVE_ROWS;         // rows of time one workgroup owns
constexpr int TS_REC = 5;                               // values of a record
constexpr int TS_BATCH = 8;                             // rows (scan) or segments (stitch) whose loads are in flight together

inline long ts_segments(long rows) { return (rows + TS_SEG - 1) / TS_SEG; }
// bytes of `work`: the records of every segment of `cols` columns, in elements of `elem` bytes
inline size_t ts_work_bytes(size_t elem, long cols, long rows) {
    const size_t bytes = (size_t)TS_REC * (size_t)ts_segments(rows) * (size_t)cols * elem;
    return bytes < 16 ? 16 : (bytes + 15) & ~(size_t)15;
}
inline size_t ts_hist_lds_bytes(int D) { return (size_t)64 * (D | 1) * sizeof(int); }

// zero the workgroup's histogram hs; behind the barrier -> the histogram row of this lane's column
__device__ __forceinline__ int* ts_hist_begin(int* hs, int D) {
    const int Dp = D | 1;
    for (int i = threadIdx.x; i < 64 * Dp; i += 256) hs[i] = 0;
    __syncthreads();
    return hs + (threadIdx.x & 63) * Dp;
}

// add the non-zero cells of hs to hist, the row of the workgroup's first column, of whose 64 columns ncols exist, with integer atomics
// (thread -> consecutive bins of one column: contiguous addresses)
__device__ __forceinline__ void ts_hist_flush(const int* hs, int D, int* hist, int ncols) {
    const int Dp = D | 1;
    for (int i = threadIdx.x; i < 64 * D; i += 256) {
        const int col = i / D, d = i - col * D;
        const int cnt = hs[col * Dp + d];
        if (cnt != 0 && col < ncols) atomicAdd(hist + (long)col * D + d, cnt);
    }
}

// the records of a workgroup's waves, in LDS
template <class T> struct TsWaveRecs {
    T v[TS_REC][TS_WAVES][64];
    __device__ __forceinline__ void put(int wave, int lane, T a, T b, T c, T d, T e) {
        v[0][wave][lane] = a; v[1][wave][lane] = b; v[2][wave][lane] = c; v[3][wave][lane] = d; v[4][wave][lane] = e;
    }
};

// the record of segment seg of column col (of cols) to `work`
template <class T> __device__ __forceinline__ void ts_put_record(T* rec, long recStride, long seg, long cols, long col, T a, T b, T c, T d, T e) {
    T* q = rec + seg * cols + col;
    q[0] = a; q[recStride] = b; q[2 * recStride] = c; q[3 * recStride] = d; q[4 * recStride] = e;
}

// the records of segments s0 ... s0 + TS_BATCH - 1 of column col, all their loads in flight together; past the last segment: no event, zeros
template <class T> __device__ __forceinline__ void ts_get_records(const T* rec, long recStride, int s0, int nseg, long cols, long col,
                                                                  T (&v)[TS_REC][TS_BATCH]) {
#pragma unroll
    for (int k = 0; k < TS_BATCH; ++k)
#pragma unroll
        for (int j = 0; j < TS_REC; ++j) v[j][k] = s0 + k < nseg ? rec[j * recStride + (long)(s0 + k) * cols + col] : (j == 0 ? (T)-1 : (T)0);
}
