// What the LPIPS trunks (lpips.hip: AlexNet, lpips_vgg.hip: VGG-16) share: the non-finite flags' geometry, the NaN-propagating
// maximum of the pools, the fixed-order fp64 sums of a wave and a workgroup, and the finalize kernel.  (The per-pixel distance
// stays with each trunk: AlexNet's walks the channels twice in fp32, VGG-16's once in fp64 and pools in the same walk.)
//   flags     [2N][C][strips] int (images 0 .. N-1 pred, N .. 2N-1 target; one flag per LP_FROWS input rows of a channel):
//             any NaN / Inf in that strip of the inputs
//   partials  [N][tiles] fp64: per pair the distance sums of its tiles, layer l's at tile0[l] .. tile0[l + 1] - 1
//   finalize  one wave per pair: fixed-order fp64 sums of each layer's tiles, / (H_l W_l); NaN when a flag of the pair is set
#pragma once
#include "common.hpp"

namespace ebfi {
namespace lpips_shared {

constexpr int LP_THREADS = 256;
constexpr int LP_FROWS = 16;   // input rows per finite-check flag
constexpr int LP_LAYERS = 5;

static inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// torch max_pool2d propagates NaN: a NaN element wins
__device__ __forceinline__ float nanmax(float m, float v) { return (v > m || v != v) ? v : m; }

static __global__ void copy_kernel(const float *__restrict__ src, int n, float *__restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// the sum of a 256-thread workgroup's values, in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double (&red)[LP_THREADS / 64]) {
    const double s = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

struct FinalArgs {
    const double *partial;
    const int *flags;
    int tile0[LP_LAYERS + 1];
    int hw[LP_LAYERS];
    int N, nflags;        // flags per image (C * strips)
    float *lpips, *layers;
};

static __global__ __launch_bounds__(64) void finalize_kernel(FinalArgs a) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const double *p = a.partial + (int64_t)n * a.tile0[LP_LAYERS];
    int bad = 0;
    for (int i = lane; i < a.nflags; i += 64)
        bad |= a.flags[(int64_t)n * a.nflags + i] | a.flags[(int64_t)(a.N + n) * a.nflags + i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) bad |= __shfl_xor(bad, d, 64);
    const float qnan = __builtin_nanf("");
    double total = 0.0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        double s = 0.0;
        for (int t = a.tile0[l] + lane; t < a.tile0[l + 1]; t += 64) s += p[t];
        s = wave_sum(s) / (double)a.hw[l];
        total += s;
        if (a.layers && lane == 0) a.layers[(int64_t)n * LP_LAYERS + l] = bad ? qnan : (float)s;
    }
    if (lane == 0) a.lpips[n] = bad ? qnan : (float)total;
}

}  // namespace lpips_shared
}  // namespace ebfi
