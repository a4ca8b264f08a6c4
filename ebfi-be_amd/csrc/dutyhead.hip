// Duty head of ExposureDecision and its stage-1 loss (reference models/Ours/model_singleframe.py:75-76 and
// train_ours_exposuredecision.py:250-252):
//   Ex[b] = sigmoid(mean over h, w of ex[b, 0, h, w])                       -- sigmoid(AVGPool(ex).view(-1, 1))
//   loss  = scale * mean over b of (Ex[b] - duty[b])^2                       -- MSELoss(Ex, duty) / accu_step, scale = 1 / accu_step
// for an fp32 map ex [B, 1, H, W] read through int64 strides (unit column stride), and the gradient of the loss with respect to ex.
//
// Forward: two launches, no host synchronisation, no allocation, no atomics (capturable, bit-reproducible), the pattern of
// csrc/charbonnier.hip:
//   tile kernel     one workgroup of 256 lanes per (sample b, strip of R consecutive rows), R = ceil(4096 / W).  A lane walks the
//                   tile's 4-column quads with a stride of 256 -- one 16-byte load when the base pointer and the strides allow,
//                   scalar loads otherwise and for the ragged last quad of a row -- and sums its elements in fp64 in that order;
//                   the 64 lanes of a wave and then the 4 waves are added in a fixed order.  One fp64 partial per tile.
//   finalize kernel ONE workgroup of 4 waves: wave w sums the tile partials of samples w, w + 4, ... in a fixed order, divides by
//                   H * W, applies the sigmoid in fp64 and rounds Ex[b] to fp32 once; then wave 0 sums (Ex[b] - duty[b])^2 over
//                   the samples in fp64 (from the ROUNDED Ex, the values backward reads) in a fixed order.
// A NaN or inf element propagates into its sample's Ex and into the loss, and into no other sample: nothing is masked.
// Backward: one streaming fill, grad_ex[b, :, :] = g * scale * 2 (Ex_b - duty_b) / B * Ex_b (1 - Ex_b) / (H * W) with g read from
// device memory; every lane of a plane forms the value by the same operations, so a plane is constant bit for bit.
#include "common.hpp"

#include <cmath>

using namespace ebfi;

namespace {

constexpr int DH_THREADS = 256;
constexpr int DH_WAVES = DH_THREADS / 64;
constexpr int DH_TILE_ELEMS = 4096;     // a tile is the fewest whole rows that hold at least this many elements
constexpr int DH_FILL_ELEMS = 4096;     // elements of a plane one workgroup of the backward fill writes

struct DhArgs {
    const float *ex;
    int64_t sb, sr;         // strides of samples and rows (elements); columns are unit-stride
    int H, W;
    int rows_per_tile;      // R
    int quads_per_row;      // ceil(W / 4)
    int64_t tiles_per_sample;
};

__device__ __forceinline__ double dh_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(DH_THREADS) void duty_head_tile_kernel(DhArgs a, double *__restrict__ partial) {
    __shared__ double wave_part[DH_WAVES];
    const int64_t tile = blockIdx.x;
    const int64_t b = tile / a.tiles_per_sample, t = tile - b * a.tiles_per_sample;
    const int64_t r0 = t * a.rows_per_tile;
    const int nrow = (int)min((int64_t)a.rows_per_tile, (int64_t)a.H - r0);
    const int quads = nrow * a.quads_per_row;
    const float *base = a.ex + b * a.sb;
    double acc = 0.0;
    for (int q = threadIdx.x; q < quads; q += DH_THREADS) {
        const int rr = q / a.quads_per_row, c0 = (q - rr * a.quads_per_row) * 4;
        const float *row = base + (r0 + rr) * a.sr;
        if (c0 + 3 < a.W) {
            if (VEC) {
                const float4 v = *reinterpret_cast<const float4 *>(row + c0);
                acc += (double)v.x, acc += (double)v.y, acc += (double)v.z, acc += (double)v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc += (double)row[c0 + j];
            }
        } else {
            for (int c = c0; c < a.W; ++c) acc += (double)row[c];     // ragged row tail
        }
    }
    acc = dh_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[tile] = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

__global__ __launch_bounds__(DH_THREADS) void duty_head_finalize_kernel(const double *__restrict__ partial, int64_t tiles_per_sample,
                                                                        int64_t B, double inv_hw, const float *__restrict__ duty,
                                                                        float scale, float *Ex_out, float *__restrict__ loss_out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t b = wave; b < B; b += DH_WAVES) {
        const double *p = partial + b * tiles_per_sample;
        double s = 0.0;
        for (int64_t t = lane; t < tiles_per_sample; t += 64) s += p[t];
        s = dh_wave_sum(s);
        if (lane == 0) Ex_out[b] = (float)(1.0 / (1.0 + exp(-(s * inv_hw))));
    }
    if (duty == nullptr) return;
    __threadfence_block();
    __syncthreads();        // the rounded Ex of every sample is visible to wave 0
    if (wave == 0) {
        double s = 0.0;
        for (int64_t b = lane; b < B; b += 64) {
            const double d = (double)Ex_out[b] - (double)duty[b];
            s += d * d;
        }
        s = dh_wave_sum(s);
        if (lane == 0) loss_out[0] = (float)((double)scale * (s / (double)B));
    }
}

template <bool VEC>
__global__ __launch_bounds__(DH_THREADS) void duty_head_backward_kernel(const float *__restrict__ g, const float *__restrict__ Ex,
                                                                        const float *__restrict__ duty, int64_t B, int64_t plane,
                                                                        int64_t chunks, float scale, float *__restrict__ grad_ex) {
    const int64_t b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const double e = (double)Ex[b];
    const double coef = (double)g[0] * (double)scale * 2.0 * (e - (double)duty[b]) / (double)B * (e * (1.0 - e)) / (double)plane;
    const float v = (float)coef;
    float *dst = grad_ex + b * plane;
    const int64_t i0 = chunk * DH_FILL_ELEMS, i1 = min(i0 + (int64_t)DH_FILL_ELEMS, plane);
    if (VEC) {      // plane % 4 == 0 and a 16-byte aligned grad_ex: every quad of the chunk is whole and aligned
        const float4 q = make_float4(v, v, v, v);
        for (int64_t i = i0 + 4 * (int64_t)threadIdx.x; i < i1; i += 4 * DH_THREADS) *reinterpret_cast<float4 *>(dst + i) = q;
    } else {
        for (int64_t i = i0 + threadIdx.x; i < i1; i += DH_THREADS) dst[i] = v;
    }
}

struct DhGrid {
    int rows_per_tile, quads_per_row;
    int64_t tiles_per_sample;
};

DhGrid dh_grid(int H, int W) {
    DhGrid g;
    g.rows_per_tile = (int)ceil_div(DH_TILE_ELEMS, W);
    g.quads_per_row = (int)ceil_div(W, 4);
    g.tiles_per_sample = ceil_div((int64_t)H, g.rows_per_tile);
    return g;
}

}  // namespace

extern "C" int64_t ebfi_duty_head_workspace(int64_t B, int H, int W) {
    if (B < 0 || H < 1 || W < 1) return 0;
    return B * dh_grid(H, W).tiles_per_sample * (int64_t)sizeof(double);
}

extern "C" int ebfi_duty_head_forward(const float *ex, const int64_t ex_strides[4], const float *duty, int64_t B, int H, int W,
                                      float scale, void *workspace, int64_t workspace_bytes, float *Ex_out, float *loss_out,
                                      void *stream) {
    if (!ex || !ex_strides || !workspace || !Ex_out) return fail(EBFI_ERR_ARG, "duty_head_forward: null argument");
    if (duty && !loss_out) return fail(EBFI_ERR_ARG, "duty_head_forward: a duty needs loss_out");
    if (B < 0 || H < 1 || W < 1)
        return fail(EBFI_ERR_ARG, "duty_head_forward: bad shape B=%lld H=%d W=%d (H, W >= 1)", (long long)B, H, W);
    if (duty && !std::isfinite(scale)) return fail(EBFI_ERR_ARG, "duty_head_forward: scale must be finite");
    if (ex_strides[3] != 1)
        return fail(EBFI_ERR_UNSUPPORTED, "duty_head_forward: the column stride must be 1 (got %lld)", (long long)ex_strides[3]);
    const DhGrid g = dh_grid(H, W);
    const int64_t tiles = B * g.tiles_per_sample;
    if (tiles > INT32_MAX || B > INT32_MAX) return fail(EBFI_ERR_ARG, "duty_head_forward: too many tiles (%lld)", (long long)tiles);
    const int64_t need = ebfi_duty_head_workspace(B, H, W);
    if (workspace_bytes < need)
        return fail(EBFI_ERR_WORKSPACE, "duty_head_forward: workspace %lld bytes, %lld needed", (long long)workspace_bytes,
                    (long long)need);
    if (!aligned16(workspace)) return fail(EBFI_ERR_ARG, "duty_head_forward: workspace must be 16-byte aligned");
    if (B == 0) return EBFI_OK;
    DhArgs a;
    a.ex = ex, a.sb = ex_strides[0], a.sr = ex_strides[2];
    a.H = H, a.W = W;
    a.rows_per_tile = g.rows_per_tile, a.quads_per_row = g.quads_per_row, a.tiles_per_sample = g.tiles_per_sample;
    const bool vec = aligned16(ex) && a.sb % 4 == 0 && a.sr % 4 == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace);
    {
        ProfScope ps(vec ? "duty_head_tile/vec" : "duty_head_tile/narrow", st, 0.0, 4.0 * (double)B * H * (double)W);
        if (vec)
            hipLaunchKernelGGL(duty_head_tile_kernel<true>, dim3((unsigned)tiles), dim3(DH_THREADS), 0, st, a, partial);
        else
            hipLaunchKernelGGL(duty_head_tile_kernel<false>, dim3((unsigned)tiles), dim3(DH_THREADS), 0, st, a, partial);
    }
    int rc = check_launch("duty_head_tile");
    if (rc != EBFI_OK) return rc;
    {
        ProfScope ps("duty_head_finalize", st, 0.0, 8.0 * (double)tiles);
        hipLaunchKernelGGL(duty_head_finalize_kernel, dim3(1), dim3(DH_THREADS), 0, st, (const double *)partial, a.tiles_per_sample,
                           B, 1.0 / ((double)H * (double)W), duty, scale, Ex_out, loss_out);
    }
    return check_launch("duty_head_finalize");
}

extern "C" int ebfi_duty_head_backward(const float *g, const float *Ex, const float *duty, int64_t B, int H, int W, float scale,
                                       float *grad_ex, void *stream) {
    if (!g || !Ex || !duty || !grad_ex) return fail(EBFI_ERR_ARG, "duty_head_backward: null argument");
    if (B < 0 || H < 1 || W < 1)
        return fail(EBFI_ERR_ARG, "duty_head_backward: bad shape B=%lld H=%d W=%d (H, W >= 1)", (long long)B, H, W);
    if (!std::isfinite(scale)) return fail(EBFI_ERR_ARG, "duty_head_backward: scale must be finite");
    const int64_t plane = (int64_t)H * W;
    const int64_t chunks = ceil_div(plane, DH_FILL_ELEMS);
    if (B * chunks > INT32_MAX) return fail(EBFI_ERR_ARG, "duty_head_backward: too many chunks (%lld)", (long long)(B * chunks));
    if (B == 0) return EBFI_OK;
    const bool vec = aligned16(grad_ex) && plane % 4 == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ProfScope ps(vec ? "duty_head_bwd/vec" : "duty_head_bwd/narrow", st, 0.0, 4.0 * (double)B * (double)plane);
        if (vec)
            hipLaunchKernelGGL(duty_head_backward_kernel<true>, dim3((unsigned)(B * chunks)), dim3(DH_THREADS), 0, st, g, Ex, duty, B,
                               plane, chunks, scale, grad_ex);
        else
            hipLaunchKernelGGL(duty_head_backward_kernel<false>, dim3((unsigned)(B * chunks)), dim3(DH_THREADS), 0, st, g, Ex, duty,
                               B, plane, chunks, scale, grad_ex);
    }
    return check_launch("duty_head_backward");
}
