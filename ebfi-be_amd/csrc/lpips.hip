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
//
// The training form (ebfi_lpips_alex_forward_train / ebfi_lpips_alex_backward; the gradient's definition: include/ebfi_hip.h) is
// the same forward -- the same function on a workspace whose front is the score's -- and a backward over the pred images:
//   tap adjoint x5   sixteen threads per pixel of a tap map, two walks over the channels (the fp64 sums, then the gradient): the
//                    distance's gradient plus what the next block returned -- a map of the same size (f3, f4), or the gradient
//                    of the 3x3/s2 pooled map gathered from the at most 2 x 2 windows that hold the pixel (f1, f2): added where
//                    the pixel is the window's first maximum, which is found again from the kept map
//   conv5 .. conv2   lpips_conv_bwd_kernel: the forward's patch kernel turned round (flipped taps, K = Cout x k x k, on 8 x 8
//                    tiles: the maps are small), the ReLU mask of the kept output applied while the patch is staged
//   conv1            lpips_conv1_bwd_kernel: direct fp32, one (row phase, column phase) of the stride-4 taps per thread; its
//                    epilogue is the input epilogue (mul_c, the one-channel fold, the strides, NaN for a flagged pair)
#include "lpips_common.hpp"

#include <algorithm>
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

// The score and the training form's forward: the same launches on the same values.  `need` is what the caller's workspace must
// hold (the training form's is the score's followed by the gradient maps, so the offsets below are the same in both).
static int lpips_alex_run(const char *what, int64_t need, const float *pred, const int64_t *pred_strides, const float *target,
                          const int64_t *target_strides, int64_t N, int C, int H, int W, int normalize, const void *params,
                          void *workspace, int64_t workspace_bytes, float *out_lpips, float *out_layers, void *stream) {
    if (!pred || !target || !pred_strides || !target_strides || !params || !workspace || !out_lpips)
        return fail(EBFI_ERR_ARG, "%s: null argument", what);
    if (N < 0 || (C != 1 && C != 3) || H < 31 || W < 31)
        return fail(EBFI_ERR_ARG, "%s: bad shape N=%lld C=%d H=%d W=%d (C in {1, 3}; H, W >= 31: AlexNet's trunk needs them)", what,
                    (long long)N, C, H, W);
    if (pred_strides[3] != 1 || target_strides[3] != 1)
        return fail(EBFI_ERR_ARG, "%s: the column stride must be 1 (got %lld / %lld)", what, (long long)pred_strides[3],
                    (long long)target_strides[3]);
    if (N > 16384 || (int64_t)H * W > (1LL << 30))
        return fail(EBFI_ERR_ARG, "%s: N=%lld pairs of %d x %d in one call (at most 16384 pairs of 2^30 pixels)", what, (long long)N, H,
                    W);
    const WsLayout wl = ws_layout(N, C, H, W);
    if (workspace_bytes < need)
        return fail(EBFI_ERR_WORKSPACE, "%s: workspace %lld bytes, %lld needed", what, (long long)workspace_bytes, (long long)need);
    if (!aligned16(workspace) || !aligned16(params)) return fail(EBFI_ERR_ARG, "%s: workspace / params must be 16-byte aligned", what);
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

extern "C" int ebfi_lpips_alex(const float *pred, const int64_t pred_strides[4], const float *target, const int64_t target_strides[4],
                               int64_t N, int C, int H, int W, int normalize, const void *params, void *workspace,
                               int64_t workspace_bytes, float *out_lpips, float *out_layers, void *stream) {
    const bool ok = N >= 0 && (C == 1 || C == 3) && H >= 31 && W >= 31;      // (a bad shape is refused inside, before `need` is read)
    return lpips_alex_run("lpips_alex", ok ? ws_layout(N, C, H, W).total : 0, pred, pred_strides, target, target_strides, N, C, H, W,
                          normalize, params, workspace, workspace_bytes, out_lpips, out_layers, stream);
}

// ------------------------------------------------------------------ the training form: the gradient with respect to pred
namespace {

// gradient-side weights, float offsets: conv1 as given ([64][3][11][11]: the direct kernel stages from torch's layout); conv2 ..
// conv5 as the image of the turned-round implicit GEMM, [K][Cin] with K = (co, ky, kx) of Cout x k x k and the taps flipped: row
// (co, ky, kx) holds W[co][:][k - 1 - ky][k - 1 - kx]
struct GradParamLayout {
    int64_t w[LP_LAYERS], total;
};

GradParamLayout grad_param_layout() {
    GradParamLayout p;
    int64_t off = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        p.w[l] = off;
        off += (int64_t)LP_COUT[l] * lp_k(l);      // (every count is a multiple of 64 floats: each block is 256-byte aligned)
    }
    p.total = off;
    return p;
}

__global__ void pack_conv_bwd_kernel(const float *__restrict__ w, int CO, int CI, int KS, float *__restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= CO * KS * KS * CI) return;
    const int k = i / CI, ci = i - k * CI;
    const int co = k / (KS * KS), r = k - co * (KS * KS), ky = r / KS, kx = r - ky * KS;
    dst[i] = w[((co * CI + ci) * KS + (KS - 1 - ky)) * KS + (KS - 1 - kx)];
}

// training workspace: the score's, then two gradient maps of the pred images, each as large as the largest of f1 .. f5
struct TrainLayout {
    int64_t gmap[2], total;   // byte offsets
};

TrainLayout train_layout(int64_t N, int H, int W, const WsLayout &wl) {
    TrainLayout t;
    const Shapes s = shapes(H, W);
    int64_t most = 0;
    for (int l = 0; l < LP_LAYERS; ++l) most = std::max<int64_t>(most, (int64_t)LP_COUT[l] * s.H[l] * s.W[l]);
    int64_t off = wl.total;
    for (int i = 0; i < 2; ++i) {
        t.gmap[i] = off;
        off = align256(off + N * most * (int64_t)sizeof(float));
    }
    t.total = off;
    return t;
}

// ------------------------------------------------------------------ tap adjoint
struct TapBwdArgs {
    const float *f0, *f1;     // [N][C][H][W]: the pred images' tap map and the target images'
    const float *head;        // [C]
    const float *gin;         // SAME: [N][C][H][W]; POOLED: [N][C][PH][PW], the gradient of the 3x3/s2 pooled map; NONE: unused
    const float *grad_out;    // [N]
    float *gf;                // [N][C][H][W]: the gradient of the pred images' tap map
    int C, H, W, PH, PW;
};

enum { TAP_NONE = 0, TAP_SAME = 1, TAP_POOLED = 2 };

constexpr int TB_PX = 16;                       // pixels of a workgroup
constexpr int TB_CL = LP_THREADS / TB_PX;       // channel lanes of a pixel: lane j walks the channels j, j + 16, ...

// A workgroup owns 16 consecutive pixels, 16 threads each: the maps of f2 .. f5 have a few hundred pixels and up to 384 channels,
// so the channels are what there is to spread.  The gradient of a pixel needs its channel sums first, so the channels are walked
// twice: the first walk forms sum x^2, sum y^2, sum w x^2, sum w x (y - x) in fp64 -- per lane, then over the 16 lanes through LDS
// in lane order, every thread of the pixel the same sum -- the second reads x and y again and writes
//   grad_out[n] / (H W) * (a_k r0 - x_k r0^2 S / n0) + (what arrives from the next block)
// The target enters as e = y - x (exact in fp64): a_k = 2 w_k ((r0 - r1) x_k - r1 e_k), S = 2 ((r0 - r1) sum w x^2 - r1 sum w x e),
// so that a near-identical pair loses nothing to the cancellation of r0 x against r1 y and an identical pair gets exactly 0.
// POOLED: pixel (y, x) lies in the windows wy in [(y - 1) / 2, y / 2], wx likewise, that exist (wy < PH, wx < PW: at most 2 x 2;
// none past the last window).  For each the window's first maximum in row-major order is found again (torch's rule; a NaN wins,
// as in the forward's pool), and the window's gradient is added when that is this pixel: a gather, in a fixed order.
template <int MODE>
__global__ __launch_bounds__(LP_THREADS) void lpips_alex_tap_bwd_kernel(TapBwdArgs a) {
    __shared__ double part[4][TB_CL][TB_PX];
    const int n = blockIdx.y;
    const int hw = a.H * a.W;
    const int px = threadIdx.x % TB_PX, cl = threadIdx.x / TB_PX;
    const int p = blockIdx.x * TB_PX + px;
    const bool in = p < hw;
    const int y = p / a.W, x = p - y * a.W;
    const int64_t at = (int64_t)n * a.C * hw;
    const float *f0 = a.f0 + at + p, *f1 = a.f1 + at + p;
    float *gf = a.gf + at + p;

    double sxx = 0.0, syy = 0.0, wxx = 0.0, wxe = 0.0;
    if (in)
        for (int c = cl; c < a.C; c += TB_CL) {
            const double u = f0[(int64_t)c * hw], v = f1[(int64_t)c * hw], e = v - u, wu = (double)a.head[c] * u;
            sxx = fma(u, u, sxx);
            syy = fma(v, v, syy);
            wxx = fma(wu, u, wxx);
            wxe = fma(wu, e, wxe);
        }
    part[0][cl][px] = sxx, part[1][cl][px] = syy, part[2][cl][px] = wxx, part[3][cl][px] = wxe;
    __syncthreads();
    if (!in) return;
    sxx = syy = wxx = wxe = 0.0;
#pragma unroll
    for (int j = 0; j < TB_CL; ++j) sxx += part[0][j][px], syy += part[1][j][px], wxx += part[2][j][px], wxe += part[3][j][px];
    const double sc = (double)a.grad_out[n] / (double)hw;
    const double n0 = sqrt(sxx);
    const double r0 = 1.0 / (n0 + 1e-10), r1 = 1.0 / (sqrt(syy) + 1e-10), ra = r0 - r1;
    const double S = 2.0 * (ra * wxx - r1 * wxe);
    const bool live = !(n0 == 0.0);     // n0 == 0: every x_k is a ReLU zero, the gradient is exactly 0 (0 / 0 is never formed)
    const double q = live ? r0 * r0 * S / n0 : 0.0;

    int wy0 = 0, wy1 = -1, wx0 = 0, wx1 = -1;
    if constexpr (MODE == TAP_POOLED) {
        wy0 = y > 0 ? (y - 1) / 2 : 0, wy1 = min(y / 2, a.PH - 1);
        wx0 = x > 0 ? (x - 1) / 2 : 0, wx1 = min(x / 2, a.PW - 1);
    }
    const int phw = a.PH * a.PW;
    const float *gin = a.gin;
    if constexpr (MODE == TAP_SAME) gin += at + p;
    if constexpr (MODE == TAP_POOLED) gin += (int64_t)n * a.C * phw;

    for (int c = cl; c < a.C; c += TB_CL) {
        const double u = f0[(int64_t)c * hw], v = f1[(int64_t)c * hw], e = v - u;
        const double ak = 2.0 * (double)a.head[c] * (ra * u - r1 * e);
        double g = live ? sc * (ak * r0 - u * q) : 0.0;
        if constexpr (MODE == TAP_SAME) g += (double)gin[(int64_t)c * hw];
        if constexpr (MODE == TAP_POOLED) {
            const float *m = a.f0 + at + (int64_t)c * hw;      // this channel's map
            for (int wy = wy0; wy <= wy1; ++wy)
                for (int wx = wx0; wx <= wx1; ++wx) {
                    const float *win = m + (2 * wy) * a.W + 2 * wx;
                    float best = win[0];
                    int first = 0;
#pragma unroll
                    for (int k = 1; k < 9; ++k) {
                        const float t = win[(k / 3) * a.W + (k % 3)];
                        if (t > best || (t != t && best == best)) best = t, first = k;
                    }
                    if (first == (y - 2 * wy) * 3 + (x - 2 * wx)) g += (double)gin[(int64_t)c * phw + wy * a.PW + wx];
                }
        }
        gf[(int64_t)c * hw] = (float)g;
    }
}

// ------------------------------------------------------------------ the stride-1 data gradients: conv2 (5x5) and conv3 .. conv5 (3x3)
struct ConvBwdArgs {
    const float *g;        // [N][CRED][H][W]: the gradient of the layer's ReLU output
    const float *f;        // [N][CRED][H][W]: that output of the pred images (the ReLU mask)
    const float *w;        // [CRED * k * k][COUT], the flipped image of pack_conv_bwd_kernel
    float *out;            // [N][COUT][H][W]: the gradient of the layer's input
    int H, W;
};

constexpr int LB_T = 8;     // output tile: LB_T x LB_T pixels

// The forward's patch kernel turned round: out[ci][p] = sum over (co, ky, kx) of W'[(co, ky, kx)][ci] * gm[co][p + (ky, kx) - k / 2],
// gm = g where the kept output is > 0 and 0 elsewhere (and outside the map), masked as the patch is staged.  The maps here are
// small (15 x 15 and 31 x 31 at 256 x 256) and only the pred images are walked, so a workgroup takes 64 output channels of an
// 8 x 8 tile, a quarter of the forward's: wave w computes channels 32 (w & 1) .. + 31 of the pixel rows 4 (w >> 1) .. + 3, one
// 32 x 32 MFMA tile, and four times as many workgroups fill the device.  One accumulator chain per output, K in order: exact
// fp32, bit-reproducible.
template <int KS, int CRED, int COUT>
__global__ __launch_bounds__(LP_THREADS) void lpips_conv_bwd_kernel(ConvBwdArgs a) {
    constexpr int P = KS / 2;
    constexpr int PW = LB_T + KS - 1, PSZ = PW * PW;
    constexpr int KC = LP_CG * KS * KS;
    constexpr int NCH = CRED / LP_CG;
    constexpr int PV = (LP_CG * PSZ + LP_THREADS - 1) / LP_THREADS, WV = KC * LP_BM / LP_THREADS;
    static_assert(COUT % LP_BM == 0 && CRED % LP_CG == 0 && KC % 2 == 0 && (KC * LP_BM) % LP_THREADS == 0, "chunking");
    __shared__ float patch[LP_CG * PSZ];
    __shared__ float ws[KC][LP_BM + LP_PAD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = a.H * a.W;
    const int ntx = (a.W + LB_T - 1) / LB_T;
    const int ty0 = (blockIdx.x / ntx) * LB_T, tx0 = (blockIdx.x % ntx) * LB_T;
    const int co0 = blockIdx.y * LP_BM;
    const int img = blockIdx.z;
    const float *gbase = a.g + (int64_t)img * CRED * HW, *fbase = a.f + (int64_t)img * CRED * HW;

    float pv[PV], wv[WV];
    auto gather = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < PV; ++i) {
            const int e = tid + LP_THREADS * i;
            const int c = e / PSZ, r = e - c * PSZ, y = r / PW, x = r - y * PW;
            const int iy = ty0 - P + y, ix = tx0 - P + x;
            float v = 0.f;
            if (e < LP_CG * PSZ && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                const int64_t o = (int64_t)(chunk * LP_CG + c) * HW + iy * a.W + ix;
                v = fbase[o] > 0.f ? gbase[o] : 0.f;
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
    f32x16 acc = f32x16{};

    gather(0);
    stage();
    __syncthreads();
    const int kl = lane >> 5, cl = lane & 31;
    const int ch = 32 * (wave & 1), row0 = 4 * (wave >> 1);
    const int pix = (row0 + (cl >> 3)) * PW + (cl & 7);      // this lane's pixel of the MFMA column tile
    for (int chunk = 0; chunk < NCH; ++chunk) {
        const bool more = chunk + 1 < NCH;
        if (more) gather(chunk + 1);
#pragma unroll 2
        for (int s2 = 0; s2 < KC / 2; ++s2) {
            const int k = 2 * s2 + kl;
            const int c = k / (KS * KS), r = k - c * (KS * KS), ky = r / KS, kx = r - ky * KS;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[k][ch + cl], patch[c * PSZ + ky * PW + kx + pix], acc, 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            stage();
            __syncthreads();
        }
    }
    // C/D: column (pixel) = lane & 31, row (channel) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int oy = ty0 + row0 + (cl >> 3), ox = tx0 + (cl & 7);
    if (oy >= a.H || ox >= a.W) return;
    float *out = a.out + ((int64_t)img * COUT + co0 + ch) * HW + oy * a.W + ox;
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(int64_t)((r & 3) + 8 * (r >> 2) + 4 * kl) * HW] = acc[r];
}

// ------------------------------------------------------------------ conv1's data gradient (11x11, stride 4, padding 2) and the input epilogue
struct Conv1BwdArgs {
    const float *g;        // [N][64][Ho][Wo]: the gradient of f1
    const float *f;        // [N][64][Ho][Wo]: f1 of the pred images (the ReLU mask)
    const float *w;        // [64][3][11][11]
    const int *flags;      // [2N][C][strips], the forward's
    float *grad_pred;
    int64_t gs[3];
    int N, C, H, W, Ho, Wo, strips;
    float mul[3];
};

constexpr int C1_TILE = 32;                    // input pixels of a workgroup: 32 x 32, in u = i + 2 (so that u = 4 q + r)
constexpr int C1_Q = C1_TILE / 4;              // 8 x 8 blocks of 4 x 4 phases
constexpr int C1_G = C1_Q + 2;                 // rows / columns of f1's grid a tile reads: q - 2 .. q + 7
constexpr int C1_CO = 16;                      // output channels of conv1 per LDS chunk
constexpr int C1_WK = 3 * 11 * 11;             // weights of one output channel

// With u = i + 2 = 4 q + r, input row i meets conv1's output row o = q - d through tap k = 4 d + r, d in {0, 1, 2} (k <= 10: r = 3
// has no d = 2); columns likewise.  A thread owns one phase (r_y, r_x) and four pixels of it, q_x consecutive: per output channel
// it holds the phase's 3 x 3 x 3 weights and 3 x 6 masked gradients in registers and does 108 multiply-adds.  Sixteen lanes cover
// the sixteen phases of a 4 x 4 block.  The sum runs over the output channels in order, per channel over (d_y, d_x) in order: a
// fixed order, no atomics.  A row or column that no window covers only meets o >= Ho (zero in LDS) or an absent tap: exactly 0.
__global__ __launch_bounds__(LP_THREADS) void lpips_conv1_bwd_kernel(Conv1BwdArgs a) {
    __shared__ float gm[C1_CO][C1_G][C1_G];
    __shared__ __attribute__((aligned(16))) float wl[C1_CO * C1_WK];
    const int tid = threadIdx.x;
    const int ntx = (a.W + 2 + C1_TILE - 1) / C1_TILE;
    const int tqy = (blockIdx.x / ntx) * C1_Q, tqx = (blockIdx.x % ntx) * C1_Q;      // the tile's first q
    const int n = blockIdx.y;
    const int nflags = a.C * a.strips;
    int bad = 0;
    for (int i = tid; i < nflags; i += LP_THREADS) bad |= a.flags[(int64_t)n * nflags + i] | a.flags[(int64_t)(a.N + n) * nflags + i];
    bad = __syncthreads_or(bad);

    const int phase = tid & 15, ry = phase >> 2, rx = phase & 3;
    const int grp = tid >> 4, by = grp >> 1, bx0 = (grp & 1) * 4;
    const int HWo = a.Ho * a.Wo;
    const float *gbase = a.g + (int64_t)n * LP_COUT[0] * HWo, *fbase = a.f + (int64_t)n * LP_COUT[0] * HWo;

    float acc[4][3];
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p][0] = acc[p][1] = acc[p][2] = 0.f;

    for (int co0 = 0; co0 < LP_COUT[0]; co0 += C1_CO) {
        if (co0) __syncthreads();
        for (int e = tid; e < C1_CO * C1_G * C1_G; e += LP_THREADS) {
            const int c = e / (C1_G * C1_G), r = e - c * (C1_G * C1_G), ly = r / C1_G, lx = r - ly * C1_G;
            const int oy = tqy - 2 + ly, ox = tqx - 2 + lx;
            float v = 0.f;
            if (oy >= 0 && oy < a.Ho && ox >= 0 && ox < a.Wo) {
                const int64_t o = (int64_t)(co0 + c) * HWo + oy * a.Wo + ox;
                v = fbase[o] > 0.f ? gbase[o] : 0.f;
            }
            gm[c][ly][lx] = v;
        }
        const float4 *wsrc = reinterpret_cast<const float4 *>(a.w + co0 * C1_WK);
        for (int e = tid; e < C1_CO * C1_WK / 4; e += LP_THREADS) reinterpret_cast<float4 *>(wl)[e] = wsrc[e];
        __syncthreads();
        for (int c = 0; c < C1_CO; ++c) {
            float wr[3][3][3];      // [channel][d_y][d_x]
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int ky = 4 * dy + ry, kx = 4 * dx + rx;
                        const bool tap = ky < 11 && kx < 11;
                        wr[ch][dy][dx] = tap ? wl[c * C1_WK + ch * 121 + min(ky, 10) * 11 + min(kx, 10)] : 0.f;   // (never past wl)
                    }
            float gv[3][6];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int j = 0; j < 6; ++j) gv[dy][j] = gm[c][by + 2 - dy][bx0 + j];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                    for (int p = 0; p < 4; ++p)
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) acc[p][ch] = fmaf(wr[ch][dy][dx], gv[dy][p + 2 - dx], acc[p][ch]);
        }
    }
    const float qnan = __builtin_nanf("");
    const int i = 4 * (tqy + by) + ry - 2;
    if (i < 0 || i >= a.H) return;
    float *dst = a.grad_pred + n * a.gs[0] + i * a.gs[2];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int j = 4 * (tqx + bx0 + p) + rx - 2;
        if (j < 0 || j >= a.W) continue;
        if (a.C == 3) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) dst[ch * a.gs[1] + j] = bad ? qnan : a.mul[ch] * acc[p][ch];
        } else {   // one channel was read as three
            dst[j] = bad ? qnan : (a.mul[0] * acc[p][0] + a.mul[1] * acc[p][1]) + a.mul[2] * acc[p][2];
        }
    }
}

bool alex_shape_ok(int64_t N, int C, int H, int W) { return N >= 0 && (C == 1 || C == 3) && H >= 31 && W >= 31; }

}  // namespace

extern "C" int64_t ebfi_lpips_alex_grad_params_bytes(void) { return grad_param_layout().total * (int64_t)sizeof(float); }

extern "C" int ebfi_lpips_alex_pack_grad_params(const float *const *conv_w, void *grad_params, int64_t bytes, void *stream) {
    if (!conv_w || !grad_params) return fail(EBFI_ERR_ARG, "lpips_alex_pack_grad_params: null argument");
    for (int l = 0; l < LP_LAYERS; ++l)
        if (!conv_w[l]) return fail(EBFI_ERR_ARG, "lpips_alex_pack_grad_params: null tensor of layer %d", l + 1);
    if (bytes < ebfi_lpips_alex_grad_params_bytes())
        return fail(EBFI_ERR_WORKSPACE, "lpips_alex_pack_grad_params: %lld bytes, %lld needed", (long long)bytes,
                    (long long)ebfi_lpips_alex_grad_params_bytes());
    if (!aligned16(grad_params)) return fail(EBFI_ERR_ARG, "lpips_alex_pack_grad_params: grad_params must be 16-byte aligned");
    const GradParamLayout gl = grad_param_layout();
    float *dst = static_cast<float *>(grad_params);
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int l = 0; l < LP_LAYERS; ++l) {
        const int n = LP_COUT[l] * lp_k(l);
        if (l) hipLaunchKernelGGL(pack_conv_bwd_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, conv_w[l], LP_COUT[l], LP_CIN[l], LP_KS[l], dst + gl.w[l]);
        else hipLaunchKernelGGL(copy_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, conv_w[l], n, dst + gl.w[l]);
    }
    return check_launch("lpips_alex_pack_grad_params");
}

extern "C" int64_t ebfi_lpips_alex_train_workspace(int64_t N, int C, int H, int W) {
    if (!alex_shape_ok(N, C, H, W)) return 0;
    return train_layout(N, H, W, ws_layout(N, C, H, W)).total;
}

extern "C" int ebfi_lpips_alex_forward_train(const float *pred, const int64_t pred_strides[4], const float *target,
                                             const int64_t target_strides[4], int64_t N, int C, int H, int W, int normalize,
                                             const void *params, void *workspace, int64_t workspace_bytes, float *out_lpips,
                                             float *out_layers, void *stream) {
    return lpips_alex_run("lpips_alex_forward_train", ebfi_lpips_alex_train_workspace(N, C, H, W), pred, pred_strides, target,
                          target_strides, N, C, H, W, normalize, params, workspace, workspace_bytes, out_lpips, out_layers, stream);
}

extern "C" int ebfi_lpips_alex_backward(const float *grad_out, const void *params, const void *grad_params, void *workspace,
                                        int64_t workspace_bytes, int64_t N, int C, int H, int W, int normalize, float *grad_pred,
                                        const int64_t grad_pred_strides[4], void *stream) {
    const char *what = "lpips_alex_backward";
    if (!grad_out || !params || !grad_params || !workspace || !grad_pred || !grad_pred_strides)
        return fail(EBFI_ERR_ARG, "%s: null argument", what);
    if (!alex_shape_ok(N, C, H, W))
        return fail(EBFI_ERR_ARG, "%s: bad shape N=%lld C=%d H=%d W=%d (C in {1, 3}; H, W >= 31: AlexNet's trunk needs them)", what,
                    (long long)N, C, H, W);
    if (grad_pred_strides[3] != 1) return fail(EBFI_ERR_ARG, "%s: the column stride must be 1 (got %lld)", what, (long long)grad_pred_strides[3]);
    if (N > 16384 || (int64_t)H * W > (1LL << 30))
        return fail(EBFI_ERR_ARG, "%s: N=%lld pairs of %d x %d in one call (at most 16384 pairs of 2^30 pixels)", what, (long long)N, H, W);
    const WsLayout wl = ws_layout(N, C, H, W);
    const TrainLayout tl = train_layout(N, H, W, wl);
    if (workspace_bytes < tl.total)
        return fail(EBFI_ERR_WORKSPACE, "%s: workspace %lld bytes, %lld needed", what, (long long)workspace_bytes, (long long)tl.total);
    if (!aligned16(workspace) || !aligned16(params) || !aligned16(grad_params))
        return fail(EBFI_ERR_ARG, "%s: workspace / params / grad_params must be 16-byte aligned", what);
    if (N == 0) return EBFI_OK;
    const Shapes s = shapes(H, W);
    const ParamLayout pl = param_layout();
    const GradParamLayout gl = grad_param_layout();
    const float *prm = static_cast<const float *>(params), *gprm = static_cast<const float *>(grad_params);
    char *ws = static_cast<char *>(workspace);
    const float *feat[LP_LAYERS];      // [2N][C_l][H_l][W_l]: the pred images first
    for (int l = 0; l < LP_LAYERS; ++l) feat[l] = reinterpret_cast<const float *>(ws + wl.feat[l]);
    float *g[2] = {reinterpret_cast<float *>(ws + tl.gmap[0]), reinterpret_cast<float *>(ws + tl.gmap[1])};
    hipStream_t st = static_cast<hipStream_t>(stream);

    // g[0] takes every tap adjoint's sum, g[1] every data gradient: what block l + 1 returned to layer l
    int rc;
    for (int l = LP_LAYERS - 1; l >= 0; --l) {
        const int h = s.H[l], w = s.W[l];
        const int64_t hw = (int64_t)h * w;
        TapBwdArgs a;
        a.f0 = feat[l], a.f1 = feat[l] + N * LP_COUT[l] * hw;
        a.head = prm + pl.h[l], a.gin = g[1], a.grad_out = grad_out, a.gf = g[0];
        a.C = LP_COUT[l], a.H = h, a.W = w;
        a.PH = (h - 3) / 2 + 1, a.PW = (w - 3) / 2 + 1;
        {
            // both maps read twice, the gradient written once; the routed windows are read from cache
            ProfScope ps("lpips_alex_tap_bwd", st, 0.0, 4.0 * N * LP_COUT[l] * (double)hw * (l == 4 ? 5.0 : 6.0));
            const dim3 grid((unsigned)ceil_div(hw, TB_PX), (unsigned)N);
            if (l == 4) hipLaunchKernelGGL(lpips_alex_tap_bwd_kernel<TAP_NONE>, grid, dim3(LP_THREADS), 0, st, a);
            else if (l >= 2) hipLaunchKernelGGL(lpips_alex_tap_bwd_kernel<TAP_SAME>, grid, dim3(LP_THREADS), 0, st, a);
            else hipLaunchKernelGGL(lpips_alex_tap_bwd_kernel<TAP_POOLED>, grid, dim3(LP_THREADS), 0, st, a);
        }
        rc = check_launch("lpips_alex_tap_bwd");
        if (rc != EBFI_OK) return rc;
        if (l >= 1) {
            static const char *names[LP_LAYERS] = {"", "lpips_alex_conv2_bwd", "lpips_alex_conv3_bwd", "lpips_alex_conv4_bwd", "lpips_alex_conv5_bwd"};
            ConvBwdArgs c;
            c.g = g[0], c.f = feat[l], c.w = gprm + gl.w[l], c.out = g[1], c.H = h, c.W = w;
            {
                ProfScope ps(names[l], st, 2.0 * N * hw * LP_CIN[l] * (double)(LP_COUT[l] * LP_KS[l] * LP_KS[l]),
                             4.0 * N * hw * (2.0 * LP_COUT[l] + LP_CIN[l]));
                const dim3 grid((unsigned)(ceil_div(h, LB_T) * ceil_div(w, LB_T)), (unsigned)(LP_CIN[l] / LP_BM), (unsigned)N);
                switch (l) {
                case 1: hipLaunchKernelGGL((lpips_conv_bwd_kernel<5, LP_COUT[1], LP_CIN[1]>), grid, dim3(LP_THREADS), 0, st, c); break;
                case 2: hipLaunchKernelGGL((lpips_conv_bwd_kernel<3, LP_COUT[2], LP_CIN[2]>), grid, dim3(LP_THREADS), 0, st, c); break;
                case 3: hipLaunchKernelGGL((lpips_conv_bwd_kernel<3, LP_COUT[3], LP_CIN[3]>), grid, dim3(LP_THREADS), 0, st, c); break;
                default: hipLaunchKernelGGL((lpips_conv_bwd_kernel<3, LP_COUT[4], LP_CIN[4]>), grid, dim3(LP_THREADS), 0, st, c); break;
                }
            }
            rc = check_launch(names[l]);
            if (rc != EBFI_OK) return rc;
        } else {
            Conv1BwdArgs c;
            c.g = g[0], c.f = feat[0], c.w = gprm + gl.w[0], c.flags = reinterpret_cast<const int *>(ws + wl.flags);
            c.grad_pred = grad_pred;
            for (int d = 0; d < 3; ++d) c.gs[d] = grad_pred_strides[d];
            c.N = (int)N, c.C = C, c.H = H, c.W = W, c.Ho = h, c.Wo = w, c.strips = wl.strips;
            static const float scale[3] = {0.458f, 0.448f, 0.450f};
            for (int ch = 0; ch < 3; ++ch) c.mul[ch] = (normalize ? 2.f : 1.f) / scale[ch];
            {
                ProfScope ps("lpips_alex_conv1_bwd", st, 2.0 * N * hw * LP_COUT[0] * (double)C1_WK,
                             4.0 * N * (2.0 * LP_COUT[0] * hw + (double)C * H * W));
                const dim3 grid((unsigned)(ceil_div(H + 2, C1_TILE) * ceil_div(W + 2, C1_TILE)), (unsigned)N);
                hipLaunchKernelGGL(lpips_conv1_bwd_kernel, grid, dim3(LP_THREADS), 0, st, c);
            }
            rc = check_launch("lpips_alex_conv1_bwd");
            if (rc != EBFI_OK) return rc;
        }
    }
    return EBFI_OK;
}
