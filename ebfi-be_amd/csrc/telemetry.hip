// Per-segment statistics of a flat fp32 buffer (the parameters of FlatAdam, the packed gradient of FlatGradBucket): for every
// segment [offsets[s], offsets[s + 1]) the moments {finite count, non-finite count, min, max, sum, sum of squares} in float64 and
// a histogram over a table of ascending float64 bucket limits.  What the training monitor writes as weight / gradient norms and
// TensorBoard histograms, computed where the buffers live: the buffers never leave the device, and the 255 tensors of the model
// cost three small launches, not 255.
//
// Work split.  The segment offsets live on the DEVICE (the entry point never reads them: no host synchronisation, capturable),
// so the grid is sized from what the host knows: a segment of L elements is cut into ceil(L / kChunk) chunks, and there are at
// most ceil(n / kChunk) + S of those whatever the offsets say.  Workgroup b walks the offsets (S scalar loads at most) to find
// its (segment, chunk); workgroups past the last chunk leave.  The split depends on the offsets only, never on the data.
//
// stats_zero    clears the histograms the chunks add into.  (A kernel, not a memset: captured into a graph, a memset node of this
//               size filled the table with a stale 16-byte pattern from its second replay on, on ROCm 7.2; a launch replays right.)
// stats_chunk   one workgroup per chunk.  Every value is widened to float64 first: all comparisons, sums and squares are float64
//               (the square of an fp32 value is exact there).  A thread folds its kChunk / kThreads values in index order, the
//               workgroup folds the threads in a fixed tree: the chunk's six moments go to the workspace.  The bucket of a finite
//               value is found by binary search over the limits table, staged in LDS, and counted with integer LDS adds; the
//               non-zero bins are merged into the segment's global histogram with integer atomic adds.
// stats_finish  one workgroup per segment folds the segment's chunk records in a fixed order (thread t takes records t, t +
//               kThreads, ... in turn, then the same tree) and writes moments[s].
// Integer counts do not depend on arrival order and every float64 fold has one order: two calls on the same data give the same
// bits.  Offsets are clamped into [0, n] and made ascending on the device, so no offset table can take a load out of bounds.
#include "common.hpp"

#include <cmath>

#pragma clang fp contract(off)

using namespace ebfi;

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 4096;         // elements per workgroup: 16 per thread
constexpr int kMaxBuckets = 2048;    // limits (8 bytes) + counts (4 bytes) in LDS: 24 KiB
constexpr int kMoments = 6;          // finite count, non-finite count, min, max, sum, sum of squares

struct Acc {
    double cnt, bad, mn, mx, sum, sq;
};

__device__ inline Acc acc_empty() { return Acc{0.0, 0.0, INFINITY, -INFINITY, 0.0, 0.0}; }

__device__ inline Acc acc_merge(const Acc &a, const Acc &b) {
    return Acc{a.cnt + b.cnt, a.bad + b.bad, b.mn < a.mn ? b.mn : a.mn, b.mx > a.mx ? b.mx : a.mx, a.sum + b.sum, a.sq + b.sq};
}

// the workgroup's fold: a fixed binary tree over the threads; the result is valid in thread 0
__device__ inline Acc block_fold(Acc a, double (*s)[kThreads]) {
    const int tid = threadIdx.x;
    s[0][tid] = a.cnt, s[1][tid] = a.bad, s[2][tid] = a.mn, s[3][tid] = a.mx, s[4][tid] = a.sum, s[5][tid] = a.sq;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (tid < off) {
            const Acc x{s[0][tid], s[1][tid], s[2][tid], s[3][tid], s[4][tid], s[5][tid]};
            const Acc y{s[0][tid + off], s[1][tid + off], s[2][tid + off], s[3][tid + off], s[4][tid + off], s[5][tid + off]};
            const Acc m = acc_merge(x, y);
            s[0][tid] = m.cnt, s[1][tid] = m.bad, s[2][tid] = m.mn, s[3][tid] = m.mx, s[4][tid] = m.sum, s[5][tid] = m.sq;
        }
        __syncthreads();
    }
    return Acc{s[0][0], s[1][0], s[2][0], s[3][0], s[4][0], s[5][0]};
}

// segment s as the kernels read it: both ends clamped into [0, n], the upper one not below the lower
__device__ inline void segment_range(const int64_t *__restrict__ offsets, int s, int64_t n, int64_t *lo, int64_t *hi) {
    int64_t a = offsets[s], b = offsets[s + 1];
    a = a < 0 ? 0 : (a > n ? n : a);
    b = b < a ? a : (b > n ? n : b);
    *lo = a, *hi = b;
}

__device__ inline int64_t chunks_of(int64_t len) { return (len + kChunk - 1) / kChunk; }

__global__ __launch_bounds__(kThreads) void stats_zero(int32_t *__restrict__ hist, int64_t count) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < count; i += (int64_t)gridDim.x * kThreads) hist[i] = 0;
}

// grid: ceil(n / kChunk) + S workgroups (an upper bound of the chunk count); ws: [grid][kMoments] float64
__global__ __launch_bounds__(kThreads) void stats_chunk(const float *__restrict__ x, int64_t n, const int64_t *__restrict__ offsets,
                                                        int S, const double *__restrict__ limits, int nb,
                                                        int32_t *__restrict__ hist, double *__restrict__ ws) {
    __shared__ double lim[kMaxBuckets];
    __shared__ int32_t bins[kMaxBuckets];
    __shared__ double fold[kMoments][kThreads];
    const int tid = threadIdx.x;

    // which (segment, chunk) is this workgroup's: uniform over the workgroup
    int seg = -1;
    int64_t lo = 0, hi = 0, first = 0;
    for (int s = 0; s < S; ++s) {
        int64_t a, b;
        segment_range(offsets, s, n, &a, &b);
        const int64_t c = chunks_of(b - a);
        if ((int64_t)blockIdx.x < first + c) {
            seg = s, lo = a, hi = b;
            break;
        }
        first += c;
    }
    if (seg < 0) return;
    const int64_t c0 = lo + ((int64_t)blockIdx.x - first) * kChunk;
    const int64_t c1 = c0 + kChunk < hi ? c0 + kChunk : hi;

    for (int i = tid; i < nb; i += kThreads) lim[i] = limits[i], bins[i] = 0;
    __syncthreads();

    Acc a = acc_empty();
    for (int64_t i = c0 + tid; i < c1; i += kThreads) {
        const float f = x[i];
        if ((__float_as_uint(f) & 0x7f800000u) == 0x7f800000u) {   // NaN or +-Inf: counted in their own column only
            a.bad += 1.0;
            continue;
        }
        const double v = (double)f;
        a.cnt += 1.0;
        a.mn = v < a.mn ? v : a.mn;
        a.mx = v > a.mx ? v : a.mx;
        a.sum += v;
        a.sq += v * v;
        // first bucket whose limit is not below v: limit[b - 1] < v <= limit[b]; past the last limit -> the last bucket
        int l = 0, r = nb - 1;
        while (l < r) {
            const int m = (l + r) >> 1;
            if (v <= lim[m]) r = m;
            else l = m + 1;
        }
        atomicAdd(&bins[l], 1);
    }
    const Acc t = block_fold(a, fold);   // (its barriers also order the LDS adds before the merge below)
    if (tid == 0) {
        double *o = ws + (int64_t)blockIdx.x * kMoments;
        o[0] = t.cnt, o[1] = t.bad, o[2] = t.mn, o[3] = t.mx, o[4] = t.sum, o[5] = t.sq;
    }
    int32_t *g = hist + (int64_t)seg * nb;
    for (int i = tid; i < nb; i += kThreads) {
        const int32_t c = bins[i];
        if (c) atomicAdd(&g[i], c);
    }
}

// grid: S workgroups
__global__ __launch_bounds__(kThreads) void stats_finish(int64_t n, const int64_t *__restrict__ offsets,
                                                         const double *__restrict__ ws, double *__restrict__ moments) {
    __shared__ double fold[kMoments][kThreads];
    const int seg = blockIdx.x;
    int64_t first = 0, lo, hi;
    for (int s = 0; s < seg; ++s) {
        segment_range(offsets, s, n, &lo, &hi);
        first += chunks_of(hi - lo);
    }
    segment_range(offsets, seg, n, &lo, &hi);
    const int64_t count = chunks_of(hi - lo);
    Acc a = acc_empty();
    for (int64_t k = threadIdx.x; k < count; k += kThreads) {
        const double *r = ws + (first + k) * kMoments;
        a = acc_merge(a, Acc{r[0], r[1], r[2], r[3], r[4], r[5]});
    }
    const Acc t = block_fold(a, fold);
    if (threadIdx.x == 0) {
        double *o = moments + (int64_t)seg * kMoments;
        o[0] = t.cnt, o[1] = t.bad, o[2] = t.mn, o[3] = t.mx, o[4] = t.sum, o[5] = t.sq;
    }
}

int64_t grid_of(int64_t n, int S) { return ceil_div(n, kChunk) + S; }

}  // namespace

extern "C" int64_t ebfi_segment_stats_workspace(int64_t n, int S) {
    if (n < 0 || S < 0) return 0;
    return grid_of(n, S) * kMoments * (int64_t)sizeof(double);
}

extern "C" int ebfi_segment_stats(const float *x, int64_t n, const int64_t *offsets, int S, const double *limits, int nb,
                                  double *moments, int32_t *hist, void *workspace, int64_t workspace_bytes, void *stream) {
    if (n < 0 || S < 0) return fail(EBFI_ERR_ARG, "segment_stats: bad sizes n=%lld S=%d", (long long)n, S);
    if (nb < 1 || nb > kMaxBuckets)
        return fail(EBFI_ERR_ARG, "segment_stats: %d bucket limits, the table in LDS holds 1..%d", nb, kMaxBuckets);
    if (S == 0) return EBFI_OK;
    if (!offsets || !limits || !moments || !hist || (n > 0 && !x)) return fail(EBFI_ERR_ARG, "segment_stats: null pointer");
    const int64_t grid = grid_of(n, S);
    if (grid > INT32_MAX) return fail(EBFI_ERR_UNSUPPORTED, "segment_stats: %lld elements exceed the launch grid", (long long)n);
    const int64_t need = ebfi_segment_stats_workspace(n, S);
    if (!workspace) return fail(EBFI_ERR_WORKSPACE, "segment_stats: workspace missing (%lld bytes needed)", (long long)need);
    if (!aligned16(workspace)) return fail(EBFI_ERR_ARG, "segment_stats: workspace must be 16-byte aligned");
    if (workspace_bytes < need)
        return fail(EBFI_ERR_WORKSPACE, "segment_stats: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *ws = static_cast<double *>(workspace);
    {
        const int64_t count = (int64_t)S * nb;
        const int64_t blocks = ceil_div(count, kThreads);
        ProfScope ps_("segment_stats_zero", st, 0.0, (double)count * 4.0);
        hipLaunchKernelGGL(stats_zero, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(kThreads), 0, st, hist, count);
    }
    {
        ProfScope ps_("segment_stats_chunk", st, 0.0, (double)n * 4.0);
        hipLaunchKernelGGL(stats_chunk, dim3((unsigned)grid), dim3(kThreads), 0, st, x, n, offsets, S, limits, nb, hist, ws);
    }
    {
        ProfScope ps_("segment_stats_finish", st, 0.0, 0.0);
        hipLaunchKernelGGL(stats_finish, dim3((unsigned)S), dim3(kThreads), 0, st, n, offsets, ws, moments);
    }
    return check_launch("segment_stats");
}
