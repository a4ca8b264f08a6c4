// Total norm of the flat gradient and the clipping coefficient of torch.nn.utils.clip_grad_norm_ (ebfi_amd.dp.FlatOptimizer with
// clip=...), both left on the device: the update launch (optim.hip, ebfi_optim_step_ex) reads the coefficient as its gradient
// scale, the host never sees either.  torch's own function wants one norm per parameter tensor (255 here), a host-visible
// scalar for its error check and scales the gradients in place -- in the all-reduce's wire buffer, which telemetry reads later.
// Two launches: one workgroup per chunk of EBFI_GRAD_NORM_CHUNK elements -> one float64 partial each; one workgroup that folds
// the partials.  Everything is float64 from the load on: during the first steps of a run this model holds gradients whose
// squares overflow float32 (|g| > 1.8e19) and others whose squares flush to zero (< 1e-38) (x * x of a widened float32 is exact
// in float64, so contraction cannot change a bit).  Every fold has a fixed order (per thread in index order, then one tree
// over the workgroup), no atomics, no completion counter: bit-reproducible and independent of the launch's timing.
#include "common.hpp"

using namespace ebfi;

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = EBFI_GRAD_NORM_CHUNK;               // elements per workgroup: 16 float4 per thread
constexpr int kVecPerThread = kChunk / 4 / kThreads;
static_assert(kChunk % (4 * kThreads) == 0, "a chunk is a whole number of float4 rounds");

// sum, or the maximum that keeps a NaN from either side (torch.maximum; fmax would drop it)
template <bool INF>
__device__ __forceinline__ double fold(double a, double b) {
    if (INF) return (a != a) ? a : ((b != b || b > a) ? b : a);
    return a + b;
}

template <bool INF>
__device__ __forceinline__ double take(double acc, float x) {
    const double d = (double)x;
    return INF ? fold<true>(acc, fabs(d)) : acc + d * d;
}

// a fixed tree over the 256 threads: six exchange steps inside each wave of 64, then the four waves' values in wave order.
// The result is valid in thread 0.
template <bool INF>
__device__ __forceinline__ double block_fold(double v) {
    __shared__ double per_wave[kThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fold<INF>(v, __shfl_down(v, off, 64));
    if ((threadIdx.x & 63) == 0) per_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = per_wave[0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) r = fold<INF>(r, per_wave[w]);
    return r;
}

template <bool INF>
__global__ __launch_bounds__(kThreads) void grad_norm_chunk(const float *__restrict__ g, int64_t n, double *__restrict__ partial) {
    const int64_t n4 = n >> 2;                                         // whole float4 of the buffer
    const int64_t v0 = (int64_t)blockIdx.x * (kChunk / 4);             // first float4 of this chunk
    const float4 *__restrict__ g4 = reinterpret_cast<const float4 *>(g);
    double acc = 0.0;
    float4 x[kVecPerThread];
    // all sixteen loads of a thread in flight at once (unconditional, clamped into the buffer when there is a float4 at all);
    // what lies past the end is never folded
#pragma unroll
    for (int k = 0; k < kVecPerThread; ++k) {
        const int64_t i = v0 + threadIdx.x + (int64_t)k * kThreads;
        x[k] = n4 > 0 ? g4[i < n4 ? i : n4 - 1] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < kVecPerThread; ++k) {
        const int64_t i = v0 + threadIdx.x + (int64_t)k * kThreads;
        if (i < n4) {
            acc = take<INF>(acc, x[k].x);
            acc = take<INF>(acc, x[k].y);
            acc = take<INF>(acc, x[k].z);
            acc = take<INF>(acc, x[k].w);
        }
    }
    // the n % 4 last elements belong to the chunk their index falls into (a chunk of their own when n4 * 4 ends one)
    const int64_t t0 = n4 * 4;
    if (t0 / kChunk == (int64_t)blockIdx.x && t0 + threadIdx.x < n) acc = take<INF>(acc, g[t0 + threadIdx.x]);
    const double r = block_fold<INF>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

template <bool INF>
__global__ __launch_bounds__(kThreads) void grad_norm_finish(const double *__restrict__ partial, int64_t count, int empty,
                                                             float max_norm, float *__restrict__ out) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += kThreads) acc = fold<INF>(acc, partial[i]);
    const double r = block_fold<INF>(acc);
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
        const float norm = INF ? (float)r : (float)sqrt(r);
        float c = max_norm / (norm + 1e-6f);
        c = c > 1.f ? 1.f : c;                                         // (a NaN stays: torch.clamp(max=1.0))
        out[0] = norm;
        out[1] = empty ? 1.f : c;                                      // (no gradient at all: torch returns before it scales)
    }
}

int64_t chunks_of(int64_t n) { return n <= 0 ? 0 : ceil_div(n, (int64_t)kChunk); }

}  // namespace

extern "C" int64_t ebfi_grad_norm_workspace(int64_t n) { return chunks_of(n) * (int64_t)sizeof(double); }

extern "C" int ebfi_grad_norm(const float *grad, int64_t n, int norm_kind, double max_norm, float *out, void *workspace,
                              int64_t workspace_bytes, void *stream) {
    if (n < 0) return fail(EBFI_ERR_ARG, "grad_norm: n = %lld", (long long)n);
    if (norm_kind != EBFI_NORM_L2 && norm_kind != EBFI_NORM_INF)
        return fail(EBFI_ERR_ARG, "grad_norm: norm_kind %d is neither EBFI_NORM_L2 nor EBFI_NORM_INF", norm_kind);
    if (!(max_norm > 0.0)) return fail(EBFI_ERR_ARG, "grad_norm: max_norm must be positive, got %g", max_norm);
    if (!out || (n > 0 && !grad)) return fail(EBFI_ERR_ARG, "grad_norm: null pointer");
    if (n > 0 && !aligned16(grad)) return fail(EBFI_ERR_ARG, "grad_norm: the gradient buffer must be 16-byte aligned");
    const int64_t chunks = chunks_of(n);
    if (chunks > INT32_MAX) return fail(EBFI_ERR_UNSUPPORTED, "grad_norm: %lld elements exceed the launch grid", (long long)n);
    const int64_t need = ebfi_grad_norm_workspace(n);
    if (n > 0) {
        if (!workspace) return fail(EBFI_ERR_WORKSPACE, "grad_norm: workspace missing (%lld bytes needed)", (long long)need);
        if (!aligned16(workspace)) return fail(EBFI_ERR_ARG, "grad_norm: workspace must be 16-byte aligned");
        if (workspace_bytes < need)
            return fail(EBFI_ERR_WORKSPACE, "grad_norm: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *ws = static_cast<double *>(workspace);
    const bool inf = norm_kind == EBFI_NORM_INF;
    if (n > 0) {
        ProfScope ps_("grad_norm_chunk", st, 0.0, 4.0 * (double)n);
        if (inf)
            hipLaunchKernelGGL(grad_norm_chunk<true>, dim3((unsigned)chunks), dim3(kThreads), 0, st, grad, n, ws);
        else
            hipLaunchKernelGGL(grad_norm_chunk<false>, dim3((unsigned)chunks), dim3(kThreads), 0, st, grad, n, ws);
    }
    {
        ProfScope ps_("grad_norm_finish", st, 0.0, 8.0 * (double)chunks);
        if (inf)
            hipLaunchKernelGGL(grad_norm_finish<true>, dim3(1), dim3(kThreads), 0, st, ws, chunks, n == 0 ? 1 : 0, (float)max_norm, out);
        else
            hipLaunchKernelGGL(grad_norm_finish<false>, dim3(1), dim3(kThreads), 0, st, ws, chunks, n == 0 ? 1 : 0, (float)max_norm, out);
    }
    return check_launch("grad_norm");
}
