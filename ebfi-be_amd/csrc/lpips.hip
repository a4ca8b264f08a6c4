// LPIPS (AlexNet trunk, linear heads v0.1) of the evaluation loop (the reference's perceptual_loss(net='alex') in eval mode,
// spatial=False): per pair n of an fp32 pred / target [N, C, H, W], C in {1, 3} (one channel is read as three),
//   x'       = (x * (normalize ? 2 : 1) - (normalize ? 1 : 0) - shift_c) / scale_c, zero padding after it
//   f1..f5   = the five ReLU outputs of AlexNet's `features` (conv1 11x11/s4/p2, pool, conv2 5x5/p2, pool, conv3..5 3x3/p1;
//              max-pools 3x3/s2, no padding, floor mode)
//   d_l(p)   = sum_c w_lc (u0_c - u1_c)^2,  u = f / (sqrt(sum_c f_c^2) + 1e-10)
//   lpips[n] = sum_l mean_p d_l(p)
//
// Launches, all on one stream, no host synchronisation, no allocation, no atomics (capturable, bit-reproducible):
//   finite kernel    one flag per (image, channel, 16-row strip): any NaN / Inf in the inputs
//   conv kernels x5  implicit GEMM on exact fp32 MFMA (v_mfma_f32_32x32x2_f32): out[img][co][p] = relu(b + W[co][:] . X[:][p]).
//                    A workgroup of 4 waves computes 64 output channels x 256 output pixels of one image, each wave 64 pixels
//                    (2 x 2 tiles of 32 x 32); the weight chunk comes from the packed [Kpad][Cout] image, and the next chunk is
//                    loaded into registers while the MFMAs of the current one run.  Bias + ReLU in the epilogue, fp32 out.
//                    conv1: 256 consecutive pixels; per K chunk of 16 every thread gathers the 16 im2col values of its pixel
//                    from pred / target (through their strides, applying x') into LDS.
//                    conv2 .. conv5: a 16 x 16 pixel tile; per chunk of 4 input channels the tile's input patch is staged in
//                    LDS once and the im2col operands are read from it.  conv2 / conv3 take the 3x3/s2 max of the previous
//                    ReLU map while they stage the patch, so no pooled map is written.
//   distance kernel  one thread per pixel of one layer of one pair: the two channel norms, then sum_c w_c (u0 - u1)^2 (two
//                    passes over the channels: the difference is formed before it is squared); per-tile fp64 sums
//   finalize kernel  one wave per pair: fixed-order fp64 sums of each layer's tiles, / (H_l W_l); NaN when a flag is set.
// The finalize kernel, the block sums and the flags' geometry are shared with the VGG-16 trunk: lpips_common.hpp.
#include "lpips_common.hpp"

#include <cmath>

using namespace ebfi;
using namespace ebfi::lpips_shared;

namespace {

constexpr int LP_BM = 64;      // output channels of a workgroup
constexpr int LP_BP = 256;     // output pixels of a workgroup (one per thread in the gather)
constexpr int LP_BK = 16;      // K chunk
constexpr int LP_PAD = 32;     // LDS row padding: the two lane halves of an MFMA operand read land on different banks

constexpr int LP_COUT[LP_LAYERS] = {64, 192, 384, 256, 256};
constexpr int LP_CIN[LP_LAYERS] = {3, 64, 192, 384, 256};
constexpr int LP_KS[LP_LAYERS] = {11, 5, 3, 3, 3};

__host__ __device__ constexpr int lp_k(int l) { return LP_CIN[l] * LP_KS[l] * LP_KS[l]; }
__host__ __device__ constexpr int lp_kpad(int l) { return (lp_k(l) + LP_BK - 1) / LP_BK * LP_BK; }

// packed parameters: per layer W [Kpad][Cout] (zero rows past K), bias [Cout], head [Cout]; float offsets
struct ParamLayout {
    int64_t w[LP_LAYERS], b[LP_LAYERS], h[LP_LAYERS], total;
};

ParamLayout param_layout() {
    ParamLayout p;
    int64_t off = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        p.w[l] = off;
        off += (int64_t)lp_kpad(l) * LP_COUT[l];
        p.b[l] = off;
        off += LP_COUT[l];
        p.h[l] = off;
        off += LP_COUT[l];
    }
    p.total = off;
    return p;
}

struct Shapes {
    int H[LP_LAYERS], W[LP_LAYERS];   // spatial size of f1 .. f5
};

Shapes shapes(int H, int W) {
    Shapes s;
    s.H[0] = (H + 4 - 11) / 4 + 1, s.W[0] = (W + 4 - 11) / 4 + 1;
    s.H[1] = (s.H[0] - 3) / 2 + 1, s.W[1] = (s.W[0] - 3) / 2 + 1;
    const int h3 = (s.H[1] - 3) / 2 + 1, w3 = (s.W[1] - 3) / 2 + 1;
    for (int l = 2; l < LP_LAYERS; ++l) s.H[l] = h3, s.W[l] = w3;
    return s;
}

// workspace: f1 .. f5 [2N][C_l][H_l][W_l] fp32 (images 0 .. N-1 pred, N .. 2N-1 target), tile partials [N][tiles] fp64,
// finite flags [2N][C][strips] int; each region 256-byte aligned
struct WsLayout {
    int64_t feat[LP_LAYERS], partial, flags, total;   // byte offsets
    int tile0[LP_LAYERS + 1];                          // first distance tile of each layer (per pair)
    int strips;
};

WsLayout ws_layout(int64_t N, int C, int H, int W) {
    WsLayout w;
    const Shapes s = shapes(H, W);
    int64_t off = 0;
    w.tile0[0] = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        w.feat[l] = off;
        const int64_t hw = (int64_t)s.H[l] * s.W[l];
        off = align256(off + 2 * N * LP_COUT[l] * hw * (int64_t)sizeof(float));
        w.tile0[l + 1] = w.tile0[l] + (int)ceil_div(hw, LP_THREADS);
    }
    w.partial = off;
    off = align256(off + N * w.tile0[LP_LAYERS] * (int64_t)sizeof(double));
    w.strips = (int)ceil_div(H, LP_FROWS);
    w.flags = off;
    off = align256(off + 2 * N * C * w.strips * (int64_t)sizeof(int));
    w.total = off;
    return w;
}

// ------------------------------------------------------------------ parameter packing
__global__ void pack_weight_kernel(const float *__restrict__ w, int K, int Kpad, int Cout, float *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)Kpad * Cout) return;
    const int k = (int)(i / Cout), co = (int)(i - (int64_t)k * Cout);
    dst[i] = k < K ? w[(int64_t)co * K + k] : 0.f;
}

// ------------------------------------------------------------------ non-finite inputs
struct FiniteArgs {
    const float *pred, *target;
    int64_t ps[3], ts[3];
    int N, C, H, W, strips;
    int *flags;   // [2N][C][strips]
};

__global__ __launch_bounds__(LP_THREADS) void finite_kernel(FiniteArgs a) {
    const int strip = blockIdx.x, c = blockIdx.y, img = blockIdx.z;
    const bool tgt = img >= a.N;
    const int n = tgt ? img - a.N : img;
    const float *base = tgt ? a.target + n * a.ts[0] + c * a.ts[1] : a.pred + n * a.ps[0] + c * a.ps[1];
    const int64_t rs = tgt ? a.ts[2] : a.ps[2];
    const int r0 = strip * LP_FROWS, r1 = min(r0 + LP_FROWS, a.H);
    int bad = 0;
    for (int r = r0; r < r1; ++r)
        for (int x = threadIdx.x; x < a.W; x += LP_THREADS) bad |= !isfinite(base[r * rs + x]);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) a.flags[((int64_t)img * a.C + c) * a.strips + strip] = bad;
}

// ------------------------------------------------------------------ convolutions
struct ConvArgs {
    // conv1: the images, read through their strides (channel stride 0 for a one-channel input)
    const float *pred, *target;
    int64_t ps[3], ts[3];
    int N;
    float mul[3], add[3];          // x' = x * mul + add
    // otherwise: the previous layer's ReLU map [2N][Cin][Hs][Ws]
    const float *src;
    int Hs, Ws;                    // source map (before the pool)
    int Hi, Wi;                    // convolution input (after the pool)
    int Ho, Wo;
    const float *w, *bias;         // packed [Kpad][Cout], [Cout]
    float *out;                    // [2N][Cout][Ho][Wo]
};

// conv1 (11x11, stride 4, padding 2): each thread gathers the K chunk of its own pixel from pred / target
__global__ __launch_bounds__(LP_THREADS) void lpips_conv1_kernel(ConvArgs a) {
    constexpr int KS = LP_KS[0], S = 4, P = 2;
    constexpr int COUT = LP_COUT[0], K = lp_k(0), NCH = lp_kpad(0) / LP_BK;
    __shared__ float xs[LP_BK][LP_BP + LP_PAD];
    __shared__ float ws[LP_BK][LP_BM + LP_PAD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HWo = a.Ho * a.Wo;
    const int p = blockIdx.x * LP_BP + tid;          // this thread's gather pixel
    const int co0 = blockIdx.y * LP_BM;
    const int img = blockIdx.z;
    const bool pin = p < HWo;
    const int oy = pin ? p / a.Wo : 0, ox = pin ? p - oy * a.Wo : 0;
    const int iy0 = oy * S - P, ix0 = ox * S - P;

    const bool tgt = img >= a.N;
    const int n = tgt ? img - a.N : img;
    const float *base = tgt ? a.target + n * a.ts[0] : a.pred + n * a.ps[0];
    const int64_t cs = tgt ? a.ts[1] : a.ps[1], rs = tgt ? a.ts[2] : a.ps[2];

    auto gather = [&](int chunk, float v[LP_BK], float4 &wv) {
#pragma unroll
        for (int j = 0; j < LP_BK; ++j) {
            const int k = chunk * LP_BK + j;
            const int ci = k / (KS * KS), r = k - ci * (KS * KS);
            const int ky = r / KS, kx = r - ky * KS;
            const int iy = iy0 + ky, ix = ix0 + kx;
            float x = 0.f;
            if (pin && k < K && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi) {
                x = fmaf(base[ci * cs + iy * rs + ix], a.mul[ci], a.add[ci]);
            }
            v[j] = x;
        }
        // weight chunk rows chunk * 16 .. + 15, columns co0 .. co0 + 63: one float4 per thread
        wv = *reinterpret_cast<const float4 *>(a.w + (int64_t)(chunk * LP_BK + (tid >> 4)) * COUT + co0 + 4 * (tid & 15));
    };
    auto stage = [&](const float v[LP_BK], const float4 &wv) {
#pragma unroll
        for (int j = 0; j < LP_BK; ++j) xs[j][tid] = v[j];
        *reinterpret_cast<float4 *>(&ws[tid >> 4][4 * (tid & 15)]) = wv;
    };

    using f32x16 = __attribute__((ext_vector_type(16))) float;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float v[LP_BK];
    float4 wv;
    gather(0, v, wv);
    stage(v, wv);
    __syncthreads();
    const int kl = lane >> 5, cl = lane & 31;
    for (int chunk = 0; chunk < NCH; ++chunk) {
        const bool more = chunk + 1 < NCH;
        if (more) gather(chunk + 1, v, wv);
#pragma unroll
        for (int s = 0; s < LP_BK / 2; ++s) {
            const int kk = 2 * s + kl;
            // A = weights (row: output channel), B = im2col (column: pixel)
            const float a0 = ws[kk][cl], a1 = ws[kk][32 + cl];
            const float b0 = xs[kk][64 * wave + cl], b1 = xs[kk][64 * wave + 32 + cl];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            stage(v, wv);
            __syncthreads();
        }
    }
    // C/D: column (pixel) = lane & 31, row (output channel) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float *out = a.out + (int64_t)img * COUT * HWo;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int px = blockIdx.x * LP_BP + 64 * wave + 32 * j + cl;
        if (px >= HWo) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * kl;
                const float y = acc[i][j][r] + a.bias[co];
                out[(int64_t)co * HWo + px] = y < 0.f ? 0.f : y;   // (NaN stays NaN, as torch's relu keeps it)
            }
    }
}

// conv2 .. conv5: a 16 x 16 output tile per workgroup.  Per K chunk of LP_CG input channels the tile's input patch (16 + k - 1
// square, zero outside the map; conv2 / conv3: each value the 3x3/s2 max of the previous ReLU map) is staged in LDS once, and
// every im2col operand is read from it: an input value feeds all k x k taps instead of being gathered (and max-pooled) per tap.
constexpr int LP_T = 16;    // output tile: LP_T x LP_T pixels; wave w owns rows 4 w .. 4 w + 3 (two 32-pixel MFMA columns)
constexpr int LP_CG = 4;    // input channels per K chunk

template <int L>
__global__ __launch_bounds__(LP_THREADS) void lpips_conv_patch_kernel(ConvArgs a) {
    constexpr int KS = LP_KS[L], P = KS / 2;
    constexpr bool POOL = L == 1 || L == 2;
    constexpr int CIN = LP_CIN[L], COUT = LP_COUT[L];
    constexpr int PW = LP_T + KS - 1, PSZ = PW * PW;     // patch row length and size per channel
    constexpr int KC = LP_CG * KS * KS;                  // K of a chunk (torch's (ci, ky, kx) order: a contiguous K range)
    constexpr int NCH = CIN / LP_CG;
    constexpr int PV = (LP_CG * PSZ + LP_THREADS - 1) / LP_THREADS, WV = KC * LP_BM / LP_THREADS;
    static_assert(CIN % LP_CG == 0 && KC % 2 == 0 && (KC * LP_BM) % LP_THREADS == 0, "chunking");
    __shared__ float patch[LP_CG * PSZ];
    __shared__ float ws[KC][LP_BM + LP_PAD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HWo = a.Ho * a.Wo;
    const int ntx = (a.Wo + LP_T - 1) / LP_T;
    const int ty0 = (blockIdx.x / ntx) * LP_T, tx0 = (blockIdx.x % ntx) * LP_T;
    const int co0 = blockIdx.y * LP_BM;
    const int img = blockIdx.z;
    const int64_t cs = (int64_t)a.Hs * a.Ws, rs = a.Ws;
    const float *base = a.src + (int64_t)img * CIN * cs;

    float pv[PV], wv[WV];     // the next chunk's patch values and weights of this thread
    auto gather = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < PV; ++i) {
            const int e = tid + LP_THREADS * i;
            const int c = e / PSZ, r = e - c * PSZ, y = r / PW, x = r - y * PW;
            const int iy = ty0 - P + y, ix = tx0 - P + x;
            float v = 0.f;
            if (e < LP_CG * PSZ && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi) {
                const float *q = base + (chunk * LP_CG + c) * cs;
                if constexpr (POOL) {
                    q += (2 * iy) * rs + 2 * ix;
                    v = q[0];
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx)
                            if (dy | dx) v = nanmax(v, q[dy * rs + dx]);
                } else {
                    v = q[iy * rs + ix];
                }
            }
            pv[i] = v;
        }
#pragma unroll
        for (int i = 0; i < WV; ++i) {
            const int e = tid + LP_THREADS * i;
            wv[i] = a.w[(int64_t)(chunk * KC + e / LP_BM) * COUT + co0 + e % LP_BM];
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < PV; ++i) {
            const int e = tid + LP_THREADS * i;
            if (e < LP_CG * PSZ) patch[e] = pv[i];
        }
#pragma unroll
        for (int i = 0; i < WV; ++i) {
            const int e = tid + LP_THREADS * i;
            ws[e / LP_BM][e % LP_BM] = wv[i];
        }
    };

    using f32x16 = __attribute__((ext_vector_type(16))) float;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[i][0] = acc[i][1] = f32x16{};

    gather(0);
    stage();
    __syncthreads();
    const int kl = lane >> 5, cl = lane & 31;
    // this lane's pixel of MFMA column tile j: row 4 wave + 2 j + (cl >> 4), column cl & 15 of the tile
    const int pix0 = (4 * wave + (cl >> 4)) * PW + (cl & 15), pix1 = pix0 + 2 * PW;
    for (int chunk = 0; chunk < NCH; ++chunk) {
        const bool more = chunk + 1 < NCH;
        if (more) gather(chunk + 1);
#pragma unroll 5
        for (int s2 = 0; s2 < KC / 2; ++s2) {
            const int k = 2 * s2 + kl;
            const int c = k / (KS * KS), r = k - c * (KS * KS), ky = r / KS, kx = r - ky * KS;
            const int off = c * PSZ + ky * PW + kx;
            const float b0 = patch[off + pix0], b1 = patch[off + pix1];
            const float a0 = ws[k][cl], a1 = ws[k][32 + cl];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            stage();
            __syncthreads();
        }
    }
    float *out = a.out + (int64_t)img * COUT * HWo;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int oy = ty0 + 4 * wave + 2 * j + (cl >> 4), ox = tx0 + (cl & 15);
        if (oy >= a.Ho || ox >= a.Wo) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * kl;
                const float y = acc[i][j][r] + a.bias[co];
                out[(int64_t)co * HWo + oy * a.Wo + ox] = y < 0.f ? 0.f : y;
            }
    }
}

// ------------------------------------------------------------------ distances
struct DistArgs {
    const float *feat[LP_LAYERS];
    const float *head[LP_LAYERS];
    int hw[LP_LAYERS];
    int tile0[LP_LAYERS + 1];
    int N;
    double *partial;   // [N][tiles]
};

template <int C>
__device__ float pixel_distance(const float *f0, const float *f1, const float *w, int hw) {
    float s0 = 0.f, s1 = 0.f;
    for (int c = 0; c < C; ++c) {
        const float x = f0[(int64_t)c * hw], y = f1[(int64_t)c * hw];
        s0 = fmaf(x, x, s0);
        s1 = fmaf(y, y, s1);
    }
    const float r0 = 1.f / (sqrtf(s0) + 1e-10f), r1 = 1.f / (sqrtf(s1) + 1e-10f);
    float d = 0.f;
    for (int c = 0; c < C; ++c) {
        const float e = f0[(int64_t)c * hw] * r0 - f1[(int64_t)c * hw] * r1;
        d = fmaf(w[c], e * e, d);
    }
    return d;
}

__global__ __launch_bounds__(LP_THREADS) void distance_kernel(DistArgs a) {
    __shared__ double red[LP_THREADS / 64];
    const int t = blockIdx.x, n = blockIdx.y;
    int l = 0;
#pragma unroll
    for (int j = 1; j < LP_LAYERS; ++j) l += t >= a.tile0[j];
    const int hw = a.hw[l];
    const int p = (t - a.tile0[l]) * LP_THREADS + threadIdx.x;
    float d = 0.f;
    if (p < hw) {
        const int C = l == 0 ? LP_COUT[0] : l == 1 ? LP_COUT[1] : l == 2 ? LP_COUT[2] : 256;
        const float *f0 = a.feat[l] + (int64_t)n * C * hw + p;
        const float *f1 = a.feat[l] + (int64_t)(a.N + n) * C * hw + p;
        switch (l) {
        case 0: d = pixel_distance<LP_COUT[0]>(f0, f1, a.head[0], hw); break;
        case 1: d = pixel_distance<LP_COUT[1]>(f0, f1, a.head[1], hw); break;
        case 2: d = pixel_distance<LP_COUT[2]>(f0, f1, a.head[2], hw); break;
        default: d = pixel_distance<256>(f0, f1, a.head[l], hw); break;
        }
    }
    const double s = block_sum((double)d, red);
    if (threadIdx.x == 0) a.partial[(int64_t)n * a.tile0[LP_LAYERS] + t] = s;
}

}  // namespace

extern "C" int64_t ebfi_lpips_params_bytes(void) { return param_layout().total * (int64_t)sizeof(float); }

extern "C" int ebfi_lpips_pack_params(const float *const *conv_w, const float *const *conv_b, const float *const *lin_w,
                                      void *params, int64_t params_bytes, void *stream) {
    if (!conv_w || !conv_b || !lin_w || !params) return fail(EBFI_ERR_ARG, "lpips_pack_params: null argument");
    for (int l = 0; l < LP_LAYERS; ++l)
        if (!conv_w[l] || !conv_b[l] || !lin_w[l]) return fail(EBFI_ERR_ARG, "lpips_pack_params: null tensor of layer %d", l + 1);
    if (params_bytes < ebfi_lpips_params_bytes())
        return fail(EBFI_ERR_WORKSPACE, "lpips_pack_params: %lld bytes, %lld needed", (long long)params_bytes,
                    (long long)ebfi_lpips_params_bytes());
    if (!aligned16(params)) return fail(EBFI_ERR_ARG, "lpips_pack_params: params must be 16-byte aligned");
    const ParamLayout pl = param_layout();
    float *dst = static_cast<float *>(params);
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int l = 0; l < LP_LAYERS; ++l) {
        const int64_t n = (int64_t)lp_kpad(l) * LP_COUT[l];
        hipLaunchKernelGGL(pack_weight_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, conv_w[l], lp_k(l), lp_kpad(l),
                           LP_COUT[l], dst + pl.w[l]);
        hipLaunchKernelGGL(copy_kernel, dim3((unsigned)ceil_div(LP_COUT[l], 256)), dim3(256), 0, st, conv_b[l], LP_COUT[l], dst + pl.b[l]);
        hipLaunchKernelGGL(copy_kernel, dim3((unsigned)ceil_div(LP_COUT[l], 256)), dim3(256), 0, st, lin_w[l], LP_COUT[l], dst + pl.h[l]);
    }
    return check_launch("lpips_pack_params");
}

extern "C" int64_t ebfi_lpips_workspace(int64_t N, int C, int H, int W) {
    if (N < 0 || (C != 1 && C != 3) || H < 31 || W < 31) return 0;
    return ws_layout(N, C, H, W).total;
}

extern "C" int ebfi_lpips_alex(const float *pred, const int64_t pred_strides[4], const float *target, const int64_t target_strides[4],
                               int64_t N, int C, int H, int W, int normalize, const void *params, void *workspace,
                               int64_t workspace_bytes, float *out_lpips, float *out_layers, void *stream) {
    if (!pred || !target || !pred_strides || !target_strides || !params || !workspace || !out_lpips)
        return fail(EBFI_ERR_ARG, "lpips_alex: null argument");
    if (N < 0 || (C != 1 && C != 3) || H < 31 || W < 31)
        return fail(EBFI_ERR_ARG, "lpips_alex: bad shape N=%lld C=%d H=%d W=%d (C in {1, 3}; H, W >= 31: AlexNet's trunk needs them)",
                    (long long)N, C, H, W);
    if (pred_strides[3] != 1 || target_strides[3] != 1)
        return fail(EBFI_ERR_ARG, "lpips_alex: the column stride must be 1 (got %lld / %lld)", (long long)pred_strides[3],
                    (long long)target_strides[3]);
    if (N > 16384 || (int64_t)H * W > (1LL << 30))
        return fail(EBFI_ERR_ARG, "lpips_alex: N=%lld pairs of %d x %d in one call (at most 16384 pairs of 2^30 pixels)", (long long)N,
                    H, W);
    const WsLayout wl = ws_layout(N, C, H, W);
    if (workspace_bytes < wl.total)
        return fail(EBFI_ERR_WORKSPACE, "lpips_alex: workspace %lld bytes, %lld needed", (long long)workspace_bytes, (long long)wl.total);
    if (!aligned16(workspace) || !aligned16(params)) return fail(EBFI_ERR_ARG, "lpips_alex: workspace / params must be 16-byte aligned");
    if (N == 0) return EBFI_OK;
    const Shapes s = shapes(H, W);
    const ParamLayout pl = param_layout();
    const float *prm = static_cast<const float *>(params);
    char *ws = static_cast<char *>(workspace);
    float *feat[LP_LAYERS];
    for (int l = 0; l < LP_LAYERS; ++l) feat[l] = reinterpret_cast<float *>(ws + wl.feat[l]);
    int *flags = reinterpret_cast<int *>(ws + wl.flags);
    double *partial = reinterpret_cast<double *>(ws + wl.partial);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int imgs = (int)(2 * N);

    {
        FiniteArgs f;
        f.pred = pred, f.target = target;
        for (int d = 0; d < 3; ++d) f.ps[d] = pred_strides[d], f.ts[d] = target_strides[d];
        f.N = (int)N, f.C = C, f.H = H, f.W = W, f.strips = wl.strips, f.flags = flags;
        ProfScope ps("lpips_finite", st, 0.0, 8.0 * N * C * H * (double)W);
        hipLaunchKernelGGL(finite_kernel, dim3((unsigned)wl.strips, (unsigned)C, (unsigned)imgs), dim3(LP_THREADS), 0, st, f);
    }
    int rc = check_launch("lpips_finite");
    if (rc != EBFI_OK) return rc;

    static const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
    static const char *names[LP_LAYERS] = {"lpips_conv1", "lpips_conv2", "lpips_conv3", "lpips_conv4", "lpips_conv5"};
    for (int l = 0; l < LP_LAYERS; ++l) {
        ConvArgs a{};   // (conv1 reads the images, conv2 .. conv5 the previous layer's map)
        a.pred = pred, a.target = target;
        for (int d = 0; d < 3; ++d) a.ps[d] = pred_strides[d], a.ts[d] = target_strides[d];
        if (C == 1) a.ps[1] = a.ts[1] = 0;      // one channel, read as three
        a.N = (int)N;
        for (int c = 0; c < 3; ++c) {
            // normalize: x' = ((2x - 1) - shift) / scale; otherwise (x - shift) / scale
            a.mul[c] = (normalize ? 2.f : 1.f) / scale[c];
            a.add[c] = ((normalize ? -1.f : 0.f) - shift[c]) / scale[c];
        }
        a.src = l == 0 ? nullptr : feat[l - 1];
        a.Hs = l == 0 ? H : s.H[l - 1], a.Ws = l == 0 ? W : s.W[l - 1];
        const bool pool = l == 1 || l == 2;
        a.Hi = pool ? (a.Hs - 3) / 2 + 1 : a.Hs, a.Wi = pool ? (a.Ws - 3) / 2 + 1 : a.Ws;
        a.Ho = s.H[l], a.Wo = s.W[l];
        a.w = prm + pl.w[l], a.bias = prm + pl.b[l];
        a.out = feat[l];
        const int64_t hw = (int64_t)a.Ho * a.Wo;
        const unsigned tiles = l == 0 ? (unsigned)ceil_div(hw, LP_BP) : (unsigned)(ceil_div(a.Ho, LP_T) * ceil_div(a.Wo, LP_T));
        const dim3 grid(tiles, (unsigned)(LP_COUT[l] / LP_BM), (unsigned)imgs);
        ProfScope ps(names[l], st, 2.0 * imgs * hw * LP_COUT[l] * lp_k(l), 4.0 * imgs * hw * LP_COUT[l]);
        switch (l) {
        case 0: hipLaunchKernelGGL(lpips_conv1_kernel, grid, dim3(LP_THREADS), 0, st, a); break;
        case 1: hipLaunchKernelGGL(lpips_conv_patch_kernel<1>, grid, dim3(LP_THREADS), 0, st, a); break;
        case 2: hipLaunchKernelGGL(lpips_conv_patch_kernel<2>, grid, dim3(LP_THREADS), 0, st, a); break;
        case 3: hipLaunchKernelGGL(lpips_conv_patch_kernel<3>, grid, dim3(LP_THREADS), 0, st, a); break;
        default: hipLaunchKernelGGL(lpips_conv_patch_kernel<4>, grid, dim3(LP_THREADS), 0, st, a); break;
        }
        rc = check_launch(names[l]);
        if (rc != EBFI_OK) return rc;
    }

    {
        DistArgs d;
        for (int l = 0; l < LP_LAYERS; ++l) d.feat[l] = feat[l], d.head[l] = prm + pl.h[l], d.hw[l] = s.H[l] * s.W[l];
        for (int l = 0; l <= LP_LAYERS; ++l) d.tile0[l] = wl.tile0[l];
        d.N = (int)N, d.partial = partial;
        double bytes = 0.0;   // every feature value read twice (norms, then distances)
        for (int l = 0; l < LP_LAYERS; ++l) bytes += 2.0 * imgs * LP_COUT[l] * (double)d.hw[l] * 4.0;
        ProfScope ps("lpips_distance", st, 0.0, bytes);
        hipLaunchKernelGGL(distance_kernel, dim3((unsigned)wl.tile0[LP_LAYERS], (unsigned)N), dim3(LP_THREADS), 0, st, d);
    }
    rc = check_launch("lpips_distance");
    if (rc != EBFI_OK) return rc;
    {
        FinalArgs f;
        f.partial = partial, f.flags = flags;
        for (int l = 0; l <= LP_LAYERS; ++l) f.tile0[l] = wl.tile0[l];
        for (int l = 0; l < LP_LAYERS; ++l) f.hw[l] = s.H[l] * s.W[l];
        f.N = (int)N, f.nflags = C * wl.strips;
        f.lpips = out_lpips, f.layers = out_layers;
        ProfScope ps("lpips_finalize", st, 0.0, 8.0 * N * wl.tile0[LP_LAYERS]);
        hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)N), dim3(64), 0, st, f);
    }
    return check_launch("lpips_finalize");
}
