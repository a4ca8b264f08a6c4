// LPIPS (VGG-16 trunk, linear heads v0.1) of the evaluation loop (the reference's perceptual_loss(net='vgg') in eval mode,
// spatial=False): the definition of lpips.hip with the trunk exchanged.  Per pair n of an fp32 pred / target [N, C, H, W],
// C in {1, 3} (one channel is read as three), H, W >= 16:
//   x'       = (x * (normalize ? 2 : 1) - (normalize ? 1 : 0) - shift_c) / scale_c, zero padding after it
//   f1..f5   = the ReLU outputs of conv1_2, conv2_2, conv3_3, conv4_3, conv5_3 of torchvision's vgg16.features: 13 convolutions
//              3x3 / stride 1 / pad 1, channels 3-64-64 | 128-128 | 256-256-256 | 512-512-512 | 512-512-512, `|` a 2x2 / stride 2
//              max-pool without padding in floor mode (an odd last row or column is dropped)
//   d_l(p)   = sum_c w_lc (u0_c - u1_c)^2,  u = f / (sqrt(sum_c f_c^2) + 1e-10)
//   lpips[n] = sum_l mean_p d_l(p)
//
// Launches, all on one stream, no host synchronisation, no allocation, no atomics (capturable, bit-reproducible):
//   prologue kernel  reads pred / target through their strides and writes x' of the 2N images as contiguous fp32 [2N][3][H][W]
//                    (one channel broadcast to three), and one flag per (image, channel, 16-row strip): any NaN / Inf
//   convolutions x13 the library's exact-fp32 3x3 forward (conv2d.hip, conv_fwd_f32 on v_mfma_f32_32x32x2_f32) with bias and
//                    ReLU (its LeakyReLU at slope 0) in the epilogue, between two ping-pong maps; the weights stay in torch's
//                    [Cout][Cin][3][3] layout, which is what that kernel stages from.  Exact fp32 because near-identical pairs
//                    cancel most of every feature.
//   tap kernel x5    one thread per 2x2 window of a tap map of one pair, one walk over the channels: five fp64 running sums per
//                    pixel (sum x^2, sum y^2, sum w x^2, sum w x e, sum w e^2 with e = y - x) give the two channel norms and the
//                    head-weighted squared difference of the unit vectors -- in fp64 from the fp32 map, so that what is left of
//                    the error is the convolutions' -- and the same walk writes the NaN-propagating 2x2 max of both images'
//                    maps as the next block's input: the map is read once, no separate pooling pass reads it again, and no tap
//                    map outlives its block.  The last row / column of an odd map is scored and not pooled.  f5 has
//                    no pool after it.  Per-tile fp64 sums.
//   finalize kernel  lpips_common.hpp
#include "lpips_common.hpp"

#include <cmath>

using namespace ebfi;
using namespace ebfi::lpips_shared;

namespace {

constexpr int VG_CONVS = 13;
constexpr int VG_MIN = 16;     // the smallest H / W: four floor-mode pools leave one pixel
constexpr int VG_CIN[VG_CONVS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int VG_COUT[VG_CONVS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int VG_LAST[LP_LAYERS] = {1, 3, 6, 9, 12};      // the convolution whose ReLU output is tap l
constexpr int VG_TAPC[LP_LAYERS] = {64, 128, 256, 512, 512};
// conv2d.hip addresses one image of a layer with 32-bit offsets: (channels + 64) * H * W * 4 bytes < 2^31 - 2^26 at the 64-channel
// layers
constexpr int64_t VG_MAX_PIXELS = ((1LL << 31) - (1LL << 26)) / (128 * 4) - 1;

// packed parameters: the 13 weights [Cout][Cin][3][3], the 13 biases [Cout], the 5 heads; float offsets, each 64-float aligned
struct ParamLayout {
    int64_t w[VG_CONVS], b[VG_CONVS], h[LP_LAYERS], total;
};

int64_t align64(int64_t v) { return (v + 63) / 64 * 64; }

ParamLayout param_layout() {
    ParamLayout p;
    int64_t off = 0;
    for (int i = 0; i < VG_CONVS; ++i) {
        p.w[i] = off;
        off = align64(off + (int64_t)VG_COUT[i] * VG_CIN[i] * 9);
        p.b[i] = off;
        off = align64(off + VG_COUT[i]);
    }
    for (int l = 0; l < LP_LAYERS; ++l) {
        p.h[l] = off;
        off = align64(off + VG_TAPC[l]);
    }
    p.total = off;
    return p;
}

bool shape_ok(int64_t N, int C, int H, int W) {
    return N >= 0 && N <= 16384 && (C == 1 || C == 3) && H >= VG_MIN && W >= VG_MIN && (int64_t)H * W <= VG_MAX_PIXELS;
}

// workspace: x' [2N][3][H][W] fp32, two maps [2N][64][H][W] fp32 (the largest layer; images 0 .. N-1 pred, N .. 2N-1 target),
// tile partials [N][tiles] fp64, finite flags [2N][C][strips] int; each region 256-byte aligned
struct WsLayout {
    int64_t xin, map[2], partial, flags, total;   // byte offsets
    int H[LP_LAYERS], W[LP_LAYERS];                // spatial size of f1 .. f5
    int tile0[LP_LAYERS + 1];                      // first tap tile of each layer (per pair)
    int strips;
};

WsLayout ws_layout(int64_t N, int C, int H, int W) {
    WsLayout w;
    int64_t off = 0;
    w.xin = off;
    off = align256(off + 2 * N * 3 * H * W * (int64_t)sizeof(float));
    for (int i = 0; i < 2; ++i) {
        w.map[i] = off;
        off = align256(off + 2 * N * 64 * H * W * (int64_t)sizeof(float));
    }
    w.tile0[0] = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        w.H[l] = H >> l, w.W[l] = W >> l;
        const int64_t windows = (int64_t)((w.H[l] + 1) / 2) * ((w.W[l] + 1) / 2);
        w.tile0[l + 1] = w.tile0[l] + (int)ceil_div(windows, LP_THREADS);
    }
    w.partial = off;
    off = align256(off + N * w.tile0[LP_LAYERS] * (int64_t)sizeof(double));
    w.strips = (int)ceil_div(H, LP_FROWS);
    w.flags = off;
    off = align256(off + 2 * N * C * w.strips * (int64_t)sizeof(int));
    w.total = off;
    return w;
}

// ------------------------------------------------------------------ prologue: x' and the non-finite flags
struct PrologueArgs {
    const float *pred, *target;
    int64_t ps[3], ts[3];
    int N, C, H, W, strips;
    float mul[3], add[3];   // x' = x * mul + add
    float *xin;             // [2N][3][H][W]
    int *flags;             // [2N][C][strips]
};

__global__ __launch_bounds__(LP_THREADS) void lpips_vgg_prologue_kernel(PrologueArgs a) {
    const int strip = blockIdx.x, c = blockIdx.y, img = blockIdx.z;
    const bool tgt = img >= a.N;
    const int n = tgt ? img - a.N : img;
    const float *base = tgt ? a.target + n * a.ts[0] + c * a.ts[1] : a.pred + n * a.ps[0] + c * a.ps[1];
    const int64_t rs = tgt ? a.ts[2] : a.ps[2];
    const int64_t hw = (int64_t)a.H * a.W;
    float *dst = a.xin + (int64_t)img * 3 * hw;
    const int r0 = strip * LP_FROWS, r1 = min(r0 + LP_FROWS, a.H);
    int bad = 0;
    for (int r = r0; r < r1; ++r)
        for (int x = threadIdx.x; x < a.W; x += LP_THREADS) {
            const float v = base[r * rs + x];
            bad |= !isfinite(v);
            const int64_t o = (int64_t)r * a.W + x;
            if (a.C == 3) {
                dst[c * hw + o] = fmaf(v, a.mul[c], a.add[c]);
            } else {   // one channel, read as three
#pragma unroll
                for (int k = 0; k < 3; ++k) dst[k * hw + o] = fmaf(v, a.mul[k], a.add[k]);
            }
        }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) a.flags[((int64_t)img * a.C + c) * a.strips + strip] = bad;
}

// ------------------------------------------------------------------ tap pass: distances of one layer and the pool after it
struct TapArgs {
    const float *feat;     // [2N][C][H][W]
    const float *head;     // [C]
    float *pooled;         // [2N][C][H / 2][W / 2], or null (f5)
    int N, C, H, W;
    int tile0, tiles;      // this layer's first tile and the tiles of a pair (all layers)
    double *partial;       // [N][tiles]
};

// VEC: W is even, so both pixels of a window row exist and lie in one aligned float2 (H * W, y = 2 wy and x = 2 wx are even, the
// maps 256-byte aligned): two 8-byte loads per image and channel instead of four 4-byte ones.
template <bool VEC>
__global__ __launch_bounds__(LP_THREADS) void lpips_vgg_tap_kernel(TapArgs a) {
    __shared__ double red[LP_THREADS / 64];
    const int t = blockIdx.x, n = blockIdx.y;
    const int wh = (a.H + 1) / 2, ww = (a.W + 1) / 2;          // windows, the odd border's partial ones included
    const int ph = a.H / 2, pw = a.W / 2;                      // pooled map
    const int p = t * LP_THREADS + threadIdx.x;
    double d = 0.0;
    if (p < wh * ww) {
        const int wy = p / ww, wx = p - wy * ww;
        const int y = 2 * wy, x = 2 * wx;
        const bool vx = x + 1 < a.W, vy = y + 1 < a.H;
        const int64_t hw = (int64_t)a.H * a.W;
        const float *f0 = a.feat + (int64_t)n * a.C * hw + (int64_t)y * a.W + x;
        const float *f1 = a.feat + (int64_t)(a.N + n) * a.C * hw + (int64_t)y * a.W + x;
        // the window's pixels: 0 (y, x), 1 (y, x + 1), 2 (y + 1, x), 3 (y + 1, x + 1); an absent one reads pixel 0 again
        const int o1 = vx ? 1 : 0, o2 = vy ? a.W : 0, o3 = o1 + o2;
        const bool pool = a.pooled != nullptr && wy < ph && wx < pw;     // (then all four pixels exist)
        const int64_t phw = (int64_t)ph * pw;
        float *g0 = a.pooled + (int64_t)n * a.C * phw + (int64_t)wy * pw + wx;
        float *g1 = a.pooled + (int64_t)(a.N + n) * a.C * phw + (int64_t)wy * pw + wx;
        // One walk over the channels.  With y = x + e (e = y - x, formed first), a = r0 - r1 and b = r1:
        //   x r0 - y r1 = a x - b e,   sum_c w (a x - b e)^2 = a^2 sum w x^2 - 2 a b sum w x e + b^2 sum w e^2
        // so five running sums per pixel give the norms and the distance.  All in fp64: the expansion's rounding is 1e-16 of its
        // largest term, far below the difference that near-identical pairs leave (the fp32 form would lose it).
        double sxx[4] = {}, syy[4] = {}, wxx[4] = {}, wxe[4] = {}, wee[4] = {};
#pragma unroll 4
        for (int c = 0; c < a.C; ++c) {
            const float *q0 = f0 + c * hw, *q1 = f1 + c * hw;
            float x0[4], x1[4];
            if constexpr (VEC) {
                const float2 t0 = *reinterpret_cast<const float2 *>(q0), b0 = *reinterpret_cast<const float2 *>(q0 + o2);
                const float2 t1 = *reinterpret_cast<const float2 *>(q1), b1 = *reinterpret_cast<const float2 *>(q1 + o2);
                x0[0] = t0.x, x0[1] = t0.y, x0[2] = b0.x, x0[3] = b0.y;
                x1[0] = t1.x, x1[1] = t1.y, x1[2] = b1.x, x1[3] = b1.y;
            } else {
                x0[0] = q0[0], x0[1] = q0[o1], x0[2] = q0[o2], x0[3] = q0[o3];
                x1[0] = q1[0], x1[1] = q1[o1], x1[2] = q1[o2], x1[3] = q1[o3];
            }
            const double w = a.head[c];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double u = x0[k], v = x1[k], e = v - u, wu = w * u;
                sxx[k] = fma(u, u, sxx[k]);
                syy[k] = fma(v, v, syy[k]);
                wxx[k] = fma(wu, u, wxx[k]);
                wxe[k] = fma(wu, e, wxe[k]);
                wee[k] = fma(w * e, e, wee[k]);
            }
            if (pool) {
                g0[c * phw] = nanmax(nanmax(x0[0], x0[1]), nanmax(x0[2], x0[3]));
                g1[c * phw] = nanmax(nanmax(x1[0], x1[1]), nanmax(x1[2], x1[3]));
            }
        }
        double dk[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double r0 = 1.0 / (sqrt(sxx[k]) + 1e-10), r1 = 1.0 / (sqrt(syy[k]) + 1e-10), ra = r0 - r1;
            dk[k] = ra * ra * wxx[k] - 2.0 * ra * r1 * wxe[k] + r1 * r1 * wee[k];
        }
        d = dk[0] + (vx ? dk[1] : 0.0) + (vy ? dk[2] : 0.0) + (vx && vy ? dk[3] : 0.0);
    }
    const double s = block_sum(d, red);
    if (threadIdx.x == 0) a.partial[(int64_t)n * a.tiles + a.tile0 + t] = s;
}

}  // namespace

extern "C" int64_t ebfi_lpips_vgg_params_bytes(void) { return param_layout().total * (int64_t)sizeof(float); }

extern "C" int ebfi_lpips_vgg_pack_params(const float *const *conv_w, const float *const *conv_b, const float *const *lin_w,
                                          void *params, int64_t params_bytes, void *stream) {
    if (!conv_w || !conv_b || !lin_w || !params) return fail(EBFI_ERR_ARG, "lpips_vgg_pack_params: null argument");
    for (int i = 0; i < VG_CONVS; ++i)
        if (!conv_w[i] || !conv_b[i]) return fail(EBFI_ERR_ARG, "lpips_vgg_pack_params: null tensor of convolution %d", i + 1);
    for (int l = 0; l < LP_LAYERS; ++l)
        if (!lin_w[l]) return fail(EBFI_ERR_ARG, "lpips_vgg_pack_params: null head of layer %d", l + 1);
    if (params_bytes < ebfi_lpips_vgg_params_bytes())
        return fail(EBFI_ERR_WORKSPACE, "lpips_vgg_pack_params: %lld bytes, %lld needed", (long long)params_bytes,
                    (long long)ebfi_lpips_vgg_params_bytes());
    if (!aligned16(params)) return fail(EBFI_ERR_ARG, "lpips_vgg_pack_params: params must be 16-byte aligned");
    const ParamLayout pl = param_layout();
    float *dst = static_cast<float *>(params);
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto copy = [&](const float *src, int n, float *to) {
        hipLaunchKernelGGL(copy_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, src, n, to);
    };
    for (int i = 0; i < VG_CONVS; ++i) {
        copy(conv_w[i], VG_COUT[i] * VG_CIN[i] * 9, dst + pl.w[i]);
        copy(conv_b[i], VG_COUT[i], dst + pl.b[i]);
    }
    for (int l = 0; l < LP_LAYERS; ++l) copy(lin_w[l], VG_TAPC[l], dst + pl.h[l]);
    return check_launch("lpips_vgg_pack_params");
}

extern "C" int64_t ebfi_lpips_vgg_workspace(int64_t N, int C, int H, int W) {
    if (!shape_ok(N, C, H, W)) return 0;
    return ws_layout(N, C, H, W).total;
}

extern "C" int ebfi_lpips_vgg(const float *pred, const int64_t pred_strides[4], const float *target, const int64_t target_strides[4],
                              int64_t N, int C, int H, int W, int normalize, const void *params, void *workspace,
                              int64_t workspace_bytes, float *out_lpips, float *out_layers, void *stream) {
    if (!pred || !target || !pred_strides || !target_strides || !params || !workspace || !out_lpips)
        return fail(EBFI_ERR_ARG, "lpips_vgg: null argument");
    if (N < 0 || (C != 1 && C != 3) || H < VG_MIN || W < VG_MIN)
        return fail(EBFI_ERR_ARG, "lpips_vgg: bad shape N=%lld C=%d H=%d W=%d (C in {1, 3}; H, W >= %d: four pools must leave a pixel)",
                    (long long)N, C, H, W, VG_MIN);
    if (pred_strides[3] != 1 || target_strides[3] != 1)
        return fail(EBFI_ERR_ARG, "lpips_vgg: the column stride must be 1 (got %lld / %lld)", (long long)pred_strides[3],
                    (long long)target_strides[3]);
    if (!shape_ok(N, C, H, W))
        return fail(EBFI_ERR_ARG, "lpips_vgg: N=%lld pairs of %d x %d in one call (at most 16384 pairs of %lld pixels)", (long long)N, H,
                    W, (long long)VG_MAX_PIXELS);
    const WsLayout wl = ws_layout(N, C, H, W);
    if (workspace_bytes < wl.total)
        return fail(EBFI_ERR_WORKSPACE, "lpips_vgg: workspace %lld bytes, %lld needed", (long long)workspace_bytes, (long long)wl.total);
    if (!aligned16(workspace) || !aligned16(params)) return fail(EBFI_ERR_ARG, "lpips_vgg: workspace / params must be 16-byte aligned");
    if (N == 0) return EBFI_OK;
    const ParamLayout pl = param_layout();
    const float *prm = static_cast<const float *>(params);
    char *ws = static_cast<char *>(workspace);
    float *xin = reinterpret_cast<float *>(ws + wl.xin);
    float *map[2] = {reinterpret_cast<float *>(ws + wl.map[0]), reinterpret_cast<float *>(ws + wl.map[1])};
    int *flags = reinterpret_cast<int *>(ws + wl.flags);
    double *partial = reinterpret_cast<double *>(ws + wl.partial);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int imgs = (int)(2 * N);

    {
        static const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
        PrologueArgs a;
        a.pred = pred, a.target = target;
        for (int d = 0; d < 3; ++d) a.ps[d] = pred_strides[d], a.ts[d] = target_strides[d];
        a.N = (int)N, a.C = C, a.H = H, a.W = W, a.strips = wl.strips;
        for (int c = 0; c < 3; ++c) {
            // normalize: x' = ((2x - 1) - shift) / scale; otherwise (x - shift) / scale
            a.mul[c] = (normalize ? 2.f : 1.f) / scale[c];
            a.add[c] = ((normalize ? -1.f : 0.f) - shift[c]) / scale[c];
        }
        a.xin = xin, a.flags = flags;
        ProfScope ps("lpips_vgg_prologue", st, 0.0, 4.0 * imgs * (C + 3.0) * H * (double)W);
        hipLaunchKernelGGL(lpips_vgg_prologue_kernel, dim3((unsigned)wl.strips, (unsigned)C, (unsigned)imgs), dim3(LP_THREADS), 0, st, a);
    }
    int rc = check_launch("lpips_vgg_prologue");
    if (rc != EBFI_OK) return rc;

    const float *src = xin;
    int cur = 0;                       // the map the next convolution writes
    int conv = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        const int h = wl.H[l], w = wl.W[l];
        for (; conv <= VG_LAST[l]; ++conv) {
            // bias + ReLU in the epilogue: activation 1 (LeakyReLU) at slope 0
            rc = ebfi_conv2d_forward(src, prm + pl.w[conv], prm + pl.b[conv], map[cur], imgs, VG_CIN[conv], h, w, VG_COUT[conv], 3, 1,
                                     1, 1, 0.f, EBFI_F32, stream);
            if (rc != EBFI_OK) return rc;
            src = map[cur];
            cur ^= 1;
        }
        TapArgs a;
        a.feat = src, a.head = prm + pl.h[l];
        a.pooled = l + 1 < LP_LAYERS ? map[cur] : nullptr;
        a.N = (int)N, a.C = VG_TAPC[l], a.H = h, a.W = w;
        a.tile0 = wl.tile0[l], a.tiles = wl.tile0[LP_LAYERS], a.partial = partial;
        const double values = (double)imgs * VG_TAPC[l] * h * w;
        {
            ProfScope ps("lpips_vgg_tap", st, 0.0, 4.0 * values * (a.pooled ? 1.25 : 1.0));   // read once, a quarter written
            const dim3 grid((unsigned)(wl.tile0[l + 1] - wl.tile0[l]), (unsigned)N);
            if (w % 2 == 0) hipLaunchKernelGGL(lpips_vgg_tap_kernel<true>, grid, dim3(LP_THREADS), 0, st, a);
            else hipLaunchKernelGGL(lpips_vgg_tap_kernel<false>, grid, dim3(LP_THREADS), 0, st, a);
        }
        rc = check_launch("lpips_vgg_tap");
        if (rc != EBFI_OK) return rc;
        if (a.pooled) {
            src = map[cur];
            cur ^= 1;
        }
    }
    {
        FinalArgs f;
        f.partial = partial, f.flags = flags;
        for (int l = 0; l <= LP_LAYERS; ++l) f.tile0[l] = wl.tile0[l];
        for (int l = 0; l < LP_LAYERS; ++l) f.hw[l] = wl.H[l] * wl.W[l];
        f.N = (int)N, f.nflags = C * wl.strips;
        f.lpips = out_lpips, f.layers = out_layers;
        ProfScope ps("lpips_vgg_finalize", st, 0.0, 8.0 * N * wl.tile0[LP_LAYERS]);
        hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)N), dim3(64), 0, st, f);
    }
    return check_launch("lpips_vgg_finalize");
}
