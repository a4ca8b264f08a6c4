// Charbonnier loss of the validation loop (reference loss/restore.py:95-105, scored at train_ours.py:588):
//   out[n] = sum over c, h, w of sqrt((x - y)^2 + eps)      -- a SUM, eps under the root and not squared
// for an fp32 pair x / y [N, C, H, W] read through int64 strides (unit column stride), and its gradient with respect to x.
//
// Forward: two launches, no host synchronisation, no allocation, no atomics (capturable, bit-reproducible), the pattern of
// csrc/metrics.hip:
//   tile kernel     one workgroup of 256 lanes per (sample n, strip of R consecutive rows of the sample's C*H rows),
//                   R = ceil(4096 / W): a tile holds at least 4096 elements.  A lane walks the tile's 4-column quads with a
//                   stride of 256 -- one 16-byte load per image when base pointers and strides allow, scalar loads otherwise
//                   and for the ragged last quad of a row -- converts every term to fp64 and sums its terms in that order;
//                   the 64 lanes of a wave and then the 4 waves are added in a fixed order.  One fp64 partial per tile.
//   finalize kernel one wave per sample sums its tiles' partials in a fixed order in fp64 and rounds once to fp32.
// A NaN or inf element propagates through its term into the partial and the sample's sum: nothing is masked or dropped.
// Backward: one streaming pass, grad_x = g * d / sqrt(d^2 + eps) with g read from device memory, contiguous output.
#include "common.hpp"

#include <cmath>

using namespace ebfi;

namespace {

constexpr int CB_THREADS = 256;
constexpr int CB_WAVES = CB_THREADS / 64;
constexpr int CB_TILE_ELEMS = 4096;     // a tile is the fewest whole rows that hold at least this many elements

struct CbArgs {
    const float *x, *y;
    int64_t xs[3], ys[3];   // strides of N, C, rows (elements); columns are unit-stride
    int C, H, W;
    int rows_per_tile;      // R
    int quads_per_row;      // ceil(W / 4)
    int64_t tiles_per_sample;
    float eps;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// columns c0 .. c0 + 3 of a row into v[0..3]; returns how many are inside [0, W)
template <bool VEC>
__device__ __forceinline__ int load_quad(const float *row, int c0, int W, float v[4]) {
    if (c0 + 3 < W) {
        if (VEC) {
            const float4 q = *reinterpret_cast<const float4 *>(row + c0);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = row[c0 + j];
        }
        return 4;
    }
    const int n = W - c0;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < n ? row[c0 + j] : 0.f;
    return n;
}

// row r (of the sample's C*H) of tile `tile`: pointers to its first element in x and y
struct RowPtrs {
    const float *x, *y;
};

__device__ __forceinline__ RowPtrs row_ptrs(const CbArgs &a, int64_t n, int64_t r) {
    const int64_t c = r / a.H, h = r - c * a.H;
    return RowPtrs{a.x + n * a.xs[0] + c * a.xs[1] + h * a.xs[2], a.y + n * a.ys[0] + c * a.ys[1] + h * a.ys[2]};
}

template <bool VEC>
__global__ __launch_bounds__(CB_THREADS) void charbonnier_tile_kernel(CbArgs a, double *__restrict__ partial) {
    __shared__ double wave_part[CB_WAVES];
    const int64_t tile = blockIdx.x;
    const int64_t n = tile / a.tiles_per_sample, t = tile - n * a.tiles_per_sample;
    const int64_t rows = (int64_t)a.C * a.H;
    const int64_t r0 = t * a.rows_per_tile;
    const int nrow = (int)min((int64_t)a.rows_per_tile, rows - r0);
    const int quads = nrow * a.quads_per_row;
    double acc = 0.0;
    for (int q = threadIdx.x; q < quads; q += CB_THREADS) {
        const int rr = q / a.quads_per_row, c0 = (q - rr * a.quads_per_row) * 4;
        const RowPtrs p = row_ptrs(a, n, r0 + rr);
        float vx[4], vy[4];
        const int cnt = load_quad<VEC>(p.x, c0, a.W, vx);
        load_quad<VEC>(p.y, c0, a.W, vy);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < cnt) {
                const float d = vx[j] - vy[j];
                acc += (double)sqrtf(fmaf(d, d, a.eps));
            }
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[tile] = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

__global__ __launch_bounds__(64) void charbonnier_finalize_kernel(const double *__restrict__ partial, int64_t tiles_per_sample,
                                                                  float *__restrict__ out) {
    const int64_t n = blockIdx.x;
    const double *p = partial + n * tiles_per_sample;
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < tiles_per_sample; t += 64) s += p[t];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[n] = (float)s;
}

template <bool VEC>
__global__ __launch_bounds__(CB_THREADS) void charbonnier_backward_kernel(CbArgs a, const float *__restrict__ g,
                                                                          float *__restrict__ grad_x) {
    const int64_t tile = blockIdx.x;
    const int64_t n = tile / a.tiles_per_sample, t = tile - n * a.tiles_per_sample;
    const int64_t rows = (int64_t)a.C * a.H;
    const int64_t r0 = t * a.rows_per_tile;
    const int nrow = (int)min((int64_t)a.rows_per_tile, rows - r0);
    const int quads = nrow * a.quads_per_row;
    const float gv = g[0];
    for (int q = threadIdx.x; q < quads; q += CB_THREADS) {
        const int rr = q / a.quads_per_row, c0 = (q - rr * a.quads_per_row) * 4;
        const RowPtrs p = row_ptrs(a, n, r0 + rr);
        float vx[4], vy[4], o[4];
        const int cnt = load_quad<VEC>(p.x, c0, a.W, vx);
        load_quad<VEC>(p.y, c0, a.W, vy);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = vx[j] - vy[j];
            o[j] = gv * (d / sqrtf(fmaf(d, d, a.eps)));
        }
        float *dst = grad_x + (n * rows + r0 + rr) * a.W + c0;      // contiguous [N, C, H, W]
        if (VEC && cnt == 4) {                                      // (VEC implies W % 4 == 0 and a 16-byte aligned grad_x)
            *reinterpret_cast<float4 *>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) dst[j] = o[j];
        }
    }
}

struct CbGrid {
    int rows_per_tile, quads_per_row;
    int64_t tiles_per_sample;
};

CbGrid cb_grid(int C, int H, int W) {
    CbGrid g;
    g.rows_per_tile = (int)ceil_div(CB_TILE_ELEMS, W);
    g.quads_per_row = (int)ceil_div(W, 4);
    g.tiles_per_sample = ceil_div((int64_t)C * H, g.rows_per_tile);
    return g;
}

// the checks both entry points share; fills `a` and `vec` (16-byte loads possible) and returns the launch's tile count
int cb_prepare(const char *who, const float *x, const int64_t *xs, const float *y, const int64_t *ys, int64_t N, int C, int H,
               int W, float eps, CbArgs &a, bool &vec, int64_t &tiles) {
    if (N < 0 || C < 1 || H < 1 || W < 1)
        return fail(EBFI_ERR_ARG, "%s: bad shape N=%lld C=%d H=%d W=%d (C, H, W >= 1)", who, (long long)N, C, H, W);
    if (!(eps > 0.f) || !std::isfinite(eps)) return fail(EBFI_ERR_ARG, "%s: eps must be positive and finite", who);
    if (xs[3] != 1 || ys[3] != 1)
        return fail(EBFI_ERR_UNSUPPORTED, "%s: the column stride must be 1 (got %lld / %lld)", who, (long long)xs[3],
                    (long long)ys[3]);
    const CbGrid g = cb_grid(C, H, W);
    tiles = N * g.tiles_per_sample;
    if (tiles > INT32_MAX || N > INT32_MAX) return fail(EBFI_ERR_ARG, "%s: too many tiles (%lld)", who, (long long)tiles);
    a.x = x, a.y = y;
    vec = aligned16(x) && aligned16(y);
    for (int d = 0; d < 3; ++d) {
        a.xs[d] = xs[d], a.ys[d] = ys[d];
        vec = vec && (xs[d] % 4 == 0) && (ys[d] % 4 == 0);
    }
    a.C = C, a.H = H, a.W = W;
    a.rows_per_tile = g.rows_per_tile, a.quads_per_row = g.quads_per_row, a.tiles_per_sample = g.tiles_per_sample;
    a.eps = eps;
    return EBFI_OK;
}

}  // namespace

extern "C" int64_t ebfi_charbonnier_workspace(int64_t N, int C, int H, int W) {
    if (N < 0 || C < 1 || H < 1 || W < 1) return 0;
    return N * cb_grid(C, H, W).tiles_per_sample * (int64_t)sizeof(double);
}

extern "C" int ebfi_charbonnier_forward(const float *x, const int64_t x_strides[4], const float *y, const int64_t y_strides[4],
                                        int64_t N, int C, int H, int W, float eps, void *workspace, int64_t workspace_bytes,
                                        float *out, void *stream) {
    if (!x || !y || !x_strides || !y_strides || !workspace || !out) return fail(EBFI_ERR_ARG, "charbonnier_forward: null argument");
    CbArgs a;
    bool vec;
    int64_t tiles;
    int rc = cb_prepare("charbonnier_forward", x, x_strides, y, y_strides, N, C, H, W, eps, a, vec, tiles);
    if (rc != EBFI_OK) return rc;
    const int64_t need = ebfi_charbonnier_workspace(N, C, H, W);
    if (workspace_bytes < need)
        return fail(EBFI_ERR_WORKSPACE, "charbonnier_forward: workspace %lld bytes, %lld needed", (long long)workspace_bytes,
                    (long long)need);
    if (!aligned16(workspace)) return fail(EBFI_ERR_ARG, "charbonnier_forward: workspace must be 16-byte aligned");
    if (N == 0) return EBFI_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace);
    {
        ProfScope ps(vec ? "charbonnier_tile/vec" : "charbonnier_tile/narrow", st, 0.0, 8.0 * (double)N * C * H * (double)W);
        if (vec)
            hipLaunchKernelGGL(charbonnier_tile_kernel<true>, dim3((unsigned)tiles), dim3(CB_THREADS), 0, st, a, partial);
        else
            hipLaunchKernelGGL(charbonnier_tile_kernel<false>, dim3((unsigned)tiles), dim3(CB_THREADS), 0, st, a, partial);
    }
    rc = check_launch("charbonnier_tile");
    if (rc != EBFI_OK) return rc;
    {
        ProfScope ps("charbonnier_finalize", st, 0.0, 8.0 * (double)tiles);
        hipLaunchKernelGGL(charbonnier_finalize_kernel, dim3((unsigned)N), dim3(64), 0, st, (const double *)partial,
                           a.tiles_per_sample, out);
    }
    return check_launch("charbonnier_finalize");
}

extern "C" int ebfi_charbonnier_backward(const float *x, const int64_t x_strides[4], const float *y, const int64_t y_strides[4],
                                         int64_t N, int C, int H, int W, float eps, const float *g, float *grad_x, void *stream) {
    if (!x || !y || !x_strides || !y_strides || !g || !grad_x) return fail(EBFI_ERR_ARG, "charbonnier_backward: null argument");
    CbArgs a;
    bool vec;
    int64_t tiles;
    int rc = cb_prepare("charbonnier_backward", x, x_strides, y, y_strides, N, C, H, W, eps, a, vec, tiles);
    if (rc != EBFI_OK) return rc;
    if (N == 0) return EBFI_OK;
    vec = vec && aligned16(grad_x) && W % 4 == 0;      // the contiguous output's rows start on 16-byte bounds only then
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ProfScope ps(vec ? "charbonnier_bwd/vec" : "charbonnier_bwd/narrow", st, 0.0, 12.0 * (double)N * C * H * (double)W);
        if (vec)
            hipLaunchKernelGGL(charbonnier_backward_kernel<true>, dim3((unsigned)tiles), dim3(CB_THREADS), 0, st, a, g, grad_x);
        else
            hipLaunchKernelGGL(charbonnier_backward_kernel<false>, dim3((unsigned)tiles), dim3(CB_THREADS), 0, st, a, g, grad_x);
    }
    return check_launch("charbonnier_backward");
}
