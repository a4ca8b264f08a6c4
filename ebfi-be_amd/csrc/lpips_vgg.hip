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
//
// The training form (ebfi_lpips_vgg_forward_train / ebfi_lpips_vgg_backward; the gradient's definition: include/ebfi_hip.h) runs
// the same kernels on the same values -- the pred images' convolutions write into 13 kept maps, the target images' run beside them
// between two maps and into 5 kept tap maps -- so its value is the evaluation form's bit for bit.  Its backward, pred images only:
//   tap adjoint x5   one thread per 2x2 window, two walks over the channels of both tap maps (the sums, then the gradient): the
//                    distance's gradient in fp64 plus the gradient of the pooled map, routed to the window's first maximum
//   data gradients   x13, the library's exact-fp32 3x3 data gradient with the ReLU mask read from the kept output
//   epilogue kernel  the prologue's adjoint, through grad_pred's strides; NaN for a pair the forward flagged
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
    const float *feat0, *feat1;   // [N][C][H][W] each: the pred images' maps and the target images'
    const float *head;            // [C]
    float *pooled0, *pooled1;     // [N][C][H / 2][W / 2] each, or null (f5)
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
        const float *f0 = a.feat0 + (int64_t)n * a.C * hw + (int64_t)y * a.W + x;
        const float *f1 = a.feat1 + (int64_t)n * a.C * hw + (int64_t)y * a.W + x;
        // the window's pixels: 0 (y, x), 1 (y, x + 1), 2 (y + 1, x), 3 (y + 1, x + 1); an absent one reads pixel 0 again
        const int o1 = vx ? 1 : 0, o2 = vy ? a.W : 0, o3 = o1 + o2;
        const bool pool = a.pooled0 != nullptr && wy < ph && wx < pw;    // (then all four pixels exist)
        const int64_t phw = (int64_t)ph * pw;
        float *g0 = a.pooled0 + (int64_t)n * a.C * phw + (int64_t)wy * pw + wx;
        float *g1 = a.pooled1 + (int64_t)n * a.C * phw + (int64_t)wy * pw + wx;
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


// ------------------------------------------------------------------ the training form: what the forward keeps, and the backward
namespace {

// training workspace: x' [2N][3][H][W] (the backward writes the gradient of the pred images' x' over it), two maps [N][64][H][W]
// (forward: the target images' layers that are no tap; backward: the gradient maps), the pred images' pooled map
// [N][64][H / 2][W / 2], the 13 ReLU outputs of the pred images, the 5 tap maps of the target images, tile partials, flags
struct TrainLayout {
    int64_t xin, map[2], ppool, saved[VG_CONVS], ttap[LP_LAYERS], partial, flags, total;   // byte offsets, 256-byte aligned
};

TrainLayout train_layout(int64_t N, int C, int H, int W, const WsLayout &g) {
    TrainLayout t;
    const int64_t f = (int64_t)sizeof(float);
    int64_t off = 0;
    t.xin = off;
    off = align256(off + 2 * N * 3 * H * W * f);
    for (int i = 0; i < 2; ++i) {
        t.map[i] = off;
        off = align256(off + N * 64 * H * W * f);
    }
    t.ppool = off;
    off = align256(off + N * 64 * (H / 2) * (W / 2) * f);
    int conv = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        for (; conv <= VG_LAST[l]; ++conv) {
            t.saved[conv] = off;
            off = align256(off + N * VG_COUT[conv] * g.H[l] * g.W[l] * f);
        }
        t.ttap[l] = off;
        off = align256(off + N * VG_TAPC[l] * g.H[l] * g.W[l] * f);
    }
    t.partial = off;
    off = align256(off + N * g.tile0[LP_LAYERS] * (int64_t)sizeof(double));
    t.flags = off;
    off = align256(off + 2 * N * C * g.strips * (int64_t)sizeof(int));
    t.total = off;
    return t;
}

// the buffers of one forward: the evaluation form runs all 2N images through two maps; the training form keeps the pred
// images' layers and runs the target images beside them
struct FwdBuffers {
    float *xin;
    float *map[2];               // evaluation: [2N][64][H][W]; training: [N][64][H][W], the target images'
    float *ppool;                // training: the pred images' pooled map
    float *saved[VG_CONVS];      // training
    float *ttap[LP_LAYERS];      // training
    double *partial;
    int *flags;
    bool train;
};

int check_forward_args(const char *what, const float *pred, const int64_t *pred_strides, const float *target,
                       const int64_t *target_strides, int64_t N, int C, int H, int W, const void *params, void *workspace,
                       float *out_lpips) {
    if (!pred || !target || !pred_strides || !target_strides || !params || !workspace || !out_lpips)
        return fail(EBFI_ERR_ARG, "%s: null argument", what);
    if (N < 0 || (C != 1 && C != 3) || H < VG_MIN || W < VG_MIN)
        return fail(EBFI_ERR_ARG, "%s: bad shape N=%lld C=%d H=%d W=%d (C in {1, 3}; H, W >= %d: four pools must leave a pixel)", what,
                    (long long)N, C, H, W, VG_MIN);
    if (pred_strides[3] != 1 || target_strides[3] != 1)
        return fail(EBFI_ERR_ARG, "%s: the column stride must be 1 (got %lld / %lld)", what, (long long)pred_strides[3],
                    (long long)target_strides[3]);
    if (!shape_ok(N, C, H, W))
        return fail(EBFI_ERR_ARG, "%s: N=%lld pairs of %d x %d in one call (at most 16384 pairs of %lld pixels)", what, (long long)N, H,
                    W, (long long)VG_MAX_PIXELS);
    return EBFI_OK;
}

void input_scale(int normalize, float mul[3], float add[3]) {
    static const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
    for (int c = 0; c < 3; ++c) {
        // normalize: x' = ((2x - 1) - shift) / scale; otherwise (x - shift) / scale
        mul[c] = (normalize ? 2.f : 1.f) / scale[c];
        add[c] = ((normalize ? -1.f : 0.f) - shift[c]) / scale[c];
    }
}

// Both forms launch the same kernels on the same values: a convolution's tiles are per image, so the training form's two calls of
// N images compute what the evaluation form's one call of 2N computes, bit for bit.
int run_forward(const float *pred, const int64_t *pred_strides, const float *target, const int64_t *target_strides, int64_t N, int C,
                int H, int W, int normalize, const float *prm, const WsLayout &wl, const FwdBuffers &b, float *out_lpips,
                float *out_layers, void *stream) {
    const ParamLayout pl = param_layout();
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int imgs = (int)(2 * N);
    {
        PrologueArgs a;
        a.pred = pred, a.target = target;
        for (int d = 0; d < 3; ++d) a.ps[d] = pred_strides[d], a.ts[d] = target_strides[d];
        a.N = (int)N, a.C = C, a.H = H, a.W = W, a.strips = wl.strips;
        input_scale(normalize, a.mul, a.add);
        a.xin = b.xin, a.flags = b.flags;
        ProfScope ps("lpips_vgg_prologue", st, 0.0, 4.0 * imgs * (C + 3.0) * H * (double)W);
        hipLaunchKernelGGL(lpips_vgg_prologue_kernel, dim3((unsigned)wl.strips, (unsigned)C, (unsigned)imgs), dim3(LP_THREADS), 0, st, a);
    }
    int rc = check_launch("lpips_vgg_prologue");
    if (rc != EBFI_OK) return rc;

    const float *src0 = b.xin, *src1 = b.xin + N * 3 * H * W;     // the pred images' input of the next layer and the target images'
    int cur = 0;                       // the map the next convolution writes
    int conv = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        const int h = wl.H[l], w = wl.W[l];
        for (; conv <= VG_LAST[l]; ++conv) {
            // bias + ReLU in the epilogue: activation 1 (LeakyReLU) at slope 0
            float *dst0, *dst1;
            if (b.train) {
                dst0 = b.saved[conv];
                dst1 = conv == VG_LAST[l] ? b.ttap[l] : b.map[cur];
                rc = ebfi_conv2d_forward(src0, prm + pl.w[conv], prm + pl.b[conv], dst0, (int)N, VG_CIN[conv], h, w, VG_COUT[conv], 3,
                                         1, 1, 1, 0.f, EBFI_F32, stream);
                if (rc != EBFI_OK) return rc;
                rc = ebfi_conv2d_forward(src1, prm + pl.w[conv], prm + pl.b[conv], dst1, (int)N, VG_CIN[conv], h, w, VG_COUT[conv], 3,
                                         1, 1, 1, 0.f, EBFI_F32, stream);
                if (conv != VG_LAST[l]) cur ^= 1;
            } else {
                dst0 = b.map[cur];
                dst1 = dst0 + N * VG_COUT[conv] * h * w;
                rc = ebfi_conv2d_forward(src0, prm + pl.w[conv], prm + pl.b[conv], dst0, imgs, VG_CIN[conv], h, w, VG_COUT[conv], 3, 1,
                                         1, 1, 0.f, EBFI_F32, stream);
                cur ^= 1;
            }
            if (rc != EBFI_OK) return rc;
            src0 = dst0, src1 = dst1;
        }
        TapArgs a;
        a.feat0 = src0, a.feat1 = src1, a.head = prm + pl.h[l];
        a.pooled0 = a.pooled1 = nullptr;
        if (l + 1 < LP_LAYERS) {
            a.pooled0 = b.train ? b.ppool : b.map[cur];
            a.pooled1 = b.train ? b.map[cur] : b.map[cur] + N * VG_TAPC[l] * (h / 2) * (w / 2);
        }
        a.N = (int)N, a.C = VG_TAPC[l], a.H = h, a.W = w;
        a.tile0 = wl.tile0[l], a.tiles = wl.tile0[LP_LAYERS], a.partial = b.partial;
        const double values = (double)imgs * VG_TAPC[l] * h * w;
        {
            ProfScope ps("lpips_vgg_tap", st, 0.0, 4.0 * values * (a.pooled0 ? 1.25 : 1.0));   // read once, a quarter written
            const dim3 grid((unsigned)(wl.tile0[l + 1] - wl.tile0[l]), (unsigned)N);
            if (w % 2 == 0) hipLaunchKernelGGL(lpips_vgg_tap_kernel<true>, grid, dim3(LP_THREADS), 0, st, a);
            else hipLaunchKernelGGL(lpips_vgg_tap_kernel<false>, grid, dim3(LP_THREADS), 0, st, a);
        }
        rc = check_launch("lpips_vgg_tap");
        if (rc != EBFI_OK) return rc;
        if (a.pooled0) {
            src0 = a.pooled0, src1 = a.pooled1;
            cur ^= 1;
        }
    }
    {
        FinalArgs f;
        f.partial = b.partial, f.flags = b.flags;
        for (int l = 0; l <= LP_LAYERS; ++l) f.tile0[l] = wl.tile0[l];
        for (int l = 0; l < LP_LAYERS; ++l) f.hw[l] = wl.H[l] * wl.W[l];
        f.N = (int)N, f.nflags = C * wl.strips;
        f.lpips = out_lpips, f.layers = out_layers;
        ProfScope ps("lpips_vgg_finalize", st, 0.0, 8.0 * N * wl.tile0[LP_LAYERS]);
        hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)N), dim3(64), 0, st, f);
    }
    return check_launch("lpips_vgg_finalize");
}

// ------------------------------------------------------------------ tap adjoint: the distances' gradient plus the pool's routed one
struct TapBwdArgs {
    const float *f0, *f1;     // [N][C][H][W]: the pred images' tap map and the target images'
    const float *head;        // [C]
    const float *gpool;       // [N][C][H / 2][W / 2]: the gradient of the pooled map, or null (f5)
    const float *grad_out;    // [N]
    float *gf;                // [N][C][H][W]: the gradient of the pred images' tap map
    int C, H, W;
};

// One thread per 2x2 window, as the forward.  The gradient of a pixel needs its channel sums first, so the channels are walked
// twice: the first walk forms sum x^2, sum y^2, sum w x^2, sum w x (y - x) in fp64, the second reads x and y again and writes
//   grad_out[n] / (H W) * (a_k r0 - x_k r0^2 S / n0) + (the pooled map's gradient where x_k is the window's first maximum)
// VEC as in the forward: aligned float2 loads and stores on even widths.
template <bool VEC>
__global__ __launch_bounds__(LP_THREADS) void lpips_vgg_tap_bwd_kernel(TapBwdArgs a) {
    const int n = blockIdx.y;
    const int wh = (a.H + 1) / 2, ww = (a.W + 1) / 2;
    const int ph = a.H / 2, pw = a.W / 2;
    const int p = blockIdx.x * LP_THREADS + threadIdx.x;
    if (p >= wh * ww) return;
    const int wy = p / ww, wx = p - wy * ww;
    const int y = 2 * wy, x = 2 * wx;
    const bool vx = x + 1 < a.W, vy = y + 1 < a.H;
    const int64_t hw = (int64_t)a.H * a.W;
    const int64_t at = (int64_t)n * a.C * hw + (int64_t)y * a.W + x;
    const float *f0 = a.f0 + at, *f1 = a.f1 + at;
    float *gf = a.gf + at;
    // the window's pixels: 0 (y, x), 1 (y, x + 1), 2 (y + 1, x), 3 (y + 1, x + 1); an absent one reads pixel 0 again and is not written
    const int o1 = vx ? 1 : 0, o2 = vy ? a.W : 0, o3 = o1 + o2;
    const bool pool = a.gpool != nullptr && wy < ph && wx < pw;      // (then all four pixels exist)
    const int64_t phw = (int64_t)ph * pw;
    const float *gp = a.gpool + (int64_t)n * a.C * phw + (int64_t)wy * pw + wx;

    auto load = [&](const float *q, float (&v)[4]) {
        if constexpr (VEC) {
            const float2 t = *reinterpret_cast<const float2 *>(q), b = *reinterpret_cast<const float2 *>(q + o2);
            v[0] = t.x, v[1] = t.y, v[2] = b.x, v[3] = b.y;
        } else {
            v[0] = q[0], v[1] = q[o1], v[2] = q[o2], v[3] = q[o3];
        }
    };

    // As in the forward, the target enters as e = y - x (exact in fp64): a_k = 2 w_k ((r0 - r1) x_k - r1 e_k) and
    // S = 2 ((r0 - r1) sum w x^2 - r1 sum w x e), so that a near-identical pair loses nothing to the cancellation of r0 x against
    // r1 y, and an identical pair (e = 0, r0 = r1) gets exactly 0 however the compiler contracts the products.
    double sxx[4] = {}, syy[4] = {}, wxx[4] = {}, wxe[4] = {};
#pragma unroll 4
    for (int c = 0; c < a.C; ++c) {
        float x0[4], x1[4];
        load(f0 + c * hw, x0);
        load(f1 + c * hw, x1);
        const double w = a.head[c];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double u = x0[k], v = x1[k], e = v - u, wu = w * u;
            sxx[k] = fma(u, u, sxx[k]);
            syy[k] = fma(v, v, syy[k]);
            wxx[k] = fma(wu, u, wxx[k]);
            wxe[k] = fma(wu, e, wxe[k]);
        }
    }
    const double sc = (double)a.grad_out[n] / (double)hw;
    double r0[4], r1[4], ra[4], q[4];      // ra = r0 - r1, q = r0^2 S / n0
    bool live[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double n0 = sqrt(sxx[k]);
        r0[k] = 1.0 / (n0 + 1e-10), r1[k] = 1.0 / (sqrt(syy[k]) + 1e-10), ra[k] = r0[k] - r1[k];
        const double S = 2.0 * (ra[k] * wxx[k] - r1[k] * wxe[k]);
        live[k] = !(n0 == 0.0);     // n0 == 0: every x_k is a ReLU zero, the gradient is exactly 0 (0 / 0 is never formed)
        q[k] = live[k] ? r0[k] * r0[k] * S / n0 : 0.0;
    }
#pragma unroll 2
    for (int c = 0; c < a.C; ++c) {
        float x0[4], x1[4];
        load(f0 + c * hw, x0);
        load(f1 + c * hw, x1);
        const double w = a.head[c];
        int first = -1;              // the window's first maximum in row-major order (torch's rule; a NaN wins, as in the pool)
        double routed = 0.0;
        if (pool) {
            first = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (x0[k] > x0[first] || (x0[k] != x0[k] && x0[first] == x0[first])) first = k;
            routed = gp[c * phw];
        }
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double u = x0[k], v = x1[k], e = v - u;
            const double ak = 2.0 * w * (ra[k] * u - r1[k] * e);
            const double tap = live[k] ? sc * (ak * r0[k] - u * q[k]) : 0.0;
            o[k] = (float)(tap + (k == first ? routed : 0.0));
        }
        float *g = gf + c * hw;
        if constexpr (VEC) {
            *reinterpret_cast<float2 *>(g) = make_float2(o[0], o[1]);
            if (vy) *reinterpret_cast<float2 *>(g + o2) = make_float2(o[2], o[3]);
        } else {
            g[0] = o[0];
            if (vx) g[o1] = o[1];
            if (vy) g[o2] = o[2];
            if (vx && vy) g[o3] = o[3];
        }
    }
}

// ------------------------------------------------------------------ input epilogue: the adjoint of the prologue
struct EpilogueArgs {
    const float *gx;          // [N][3][H][W]: the gradient of x'
    const int *flags;         // [2N][C][strips], the forward's
    float *grad_pred;
    int64_t gs[3];
    int N, C, H, W, strips;
    float mul[3];
};

__global__ __launch_bounds__(LP_THREADS) void lpips_vgg_epilogue_kernel(EpilogueArgs a) {
    const int strip = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
    const int nflags = a.C * a.strips;
    int bad = 0;
    for (int i = threadIdx.x; i < nflags; i += LP_THREADS)
        bad |= a.flags[(int64_t)n * nflags + i] | a.flags[(int64_t)(a.N + n) * nflags + i];
    bad = __syncthreads_or(bad);
    const int64_t hw = (int64_t)a.H * a.W;
    const float *src = a.gx + (int64_t)n * 3 * hw;
    float *dst = a.grad_pred + n * a.gs[0] + c * a.gs[1];
    const float qnan = __builtin_nanf("");
    const int r0 = strip * LP_FROWS, r1 = min(r0 + LP_FROWS, a.H);
    for (int r = r0; r < r1; ++r)
        for (int x = threadIdx.x; x < a.W; x += LP_THREADS) {
            const int64_t o = (int64_t)r * a.W + x;
            float v;
            if (a.C == 3) v = a.mul[c] * src[c * hw + o];
            else v = (a.mul[0] * src[o] + a.mul[1] * src[hw + o]) + a.mul[2] * src[2 * hw + o];   // one channel was read as three
            dst[r * a.gs[2] + x] = bad ? qnan : v;
        }
}

}  // namespace

extern "C" int64_t ebfi_lpips_vgg_workspace(int64_t N, int C, int H, int W) {
    if (!shape_ok(N, C, H, W)) return 0;
    return ws_layout(N, C, H, W).total;
}

extern "C" int ebfi_lpips_vgg(const float *pred, const int64_t pred_strides[4], const float *target, const int64_t target_strides[4],
                              int64_t N, int C, int H, int W, int normalize, const void *params, void *workspace,
                              int64_t workspace_bytes, float *out_lpips, float *out_layers, void *stream) {
    if (int rc = check_forward_args("lpips_vgg", pred, pred_strides, target, target_strides, N, C, H, W, params, workspace, out_lpips))
        return rc;
    const WsLayout wl = ws_layout(N, C, H, W);
    if (workspace_bytes < wl.total)
        return fail(EBFI_ERR_WORKSPACE, "lpips_vgg: workspace %lld bytes, %lld needed", (long long)workspace_bytes, (long long)wl.total);
    if (!aligned16(workspace) || !aligned16(params)) return fail(EBFI_ERR_ARG, "lpips_vgg: workspace / params must be 16-byte aligned");
    if (N == 0) return EBFI_OK;
    char *ws = static_cast<char *>(workspace);
    FwdBuffers b{};
    b.xin = reinterpret_cast<float *>(ws + wl.xin);
    for (int i = 0; i < 2; ++i) b.map[i] = reinterpret_cast<float *>(ws + wl.map[i]);
    b.partial = reinterpret_cast<double *>(ws + wl.partial);
    b.flags = reinterpret_cast<int *>(ws + wl.flags);
    b.train = false;
    return run_forward(pred, pred_strides, target, target_strides, N, C, H, W, normalize, static_cast<const float *>(params), wl, b,
                       out_lpips, out_layers, stream);
}

extern "C" int64_t ebfi_lpips_vgg_train_workspace(int64_t N, int C, int H, int W) {
    if (!shape_ok(N, C, H, W)) return 0;
    return train_layout(N, C, H, W, ws_layout(N, C, H, W)).total;
}

extern "C" int ebfi_lpips_vgg_forward_train(const float *pred, const int64_t pred_strides[4], const float *target,
                                            const int64_t target_strides[4], int64_t N, int C, int H, int W, int normalize,
                                            const void *params, void *workspace, int64_t workspace_bytes, float *out_lpips,
                                            float *out_layers, void *stream) {
    const char *what = "lpips_vgg_forward_train";
    if (int rc = check_forward_args(what, pred, pred_strides, target, target_strides, N, C, H, W, params, workspace, out_lpips)) return rc;
    const WsLayout wl = ws_layout(N, C, H, W);
    const TrainLayout tl = train_layout(N, C, H, W, wl);
    if (workspace_bytes < tl.total)
        return fail(EBFI_ERR_WORKSPACE, "%s: workspace %lld bytes, %lld needed", what, (long long)workspace_bytes, (long long)tl.total);
    if (!aligned16(workspace) || !aligned16(params)) return fail(EBFI_ERR_ARG, "%s: workspace / params must be 16-byte aligned", what);
    if (N == 0) return EBFI_OK;
    char *ws = static_cast<char *>(workspace);
    FwdBuffers b{};
    b.xin = reinterpret_cast<float *>(ws + tl.xin);
    for (int i = 0; i < 2; ++i) b.map[i] = reinterpret_cast<float *>(ws + tl.map[i]);
    b.ppool = reinterpret_cast<float *>(ws + tl.ppool);
    for (int i = 0; i < VG_CONVS; ++i) b.saved[i] = reinterpret_cast<float *>(ws + tl.saved[i]);
    for (int l = 0; l < LP_LAYERS; ++l) b.ttap[l] = reinterpret_cast<float *>(ws + tl.ttap[l]);
    b.partial = reinterpret_cast<double *>(ws + tl.partial);
    b.flags = reinterpret_cast<int *>(ws + tl.flags);
    b.train = true;
    return run_forward(pred, pred_strides, target, target_strides, N, C, H, W, normalize, static_cast<const float *>(params), wl, b,
                       out_lpips, out_layers, stream);
}

extern "C" int ebfi_lpips_vgg_backward(const float *grad_out, const void *params, void *workspace, int64_t workspace_bytes, int64_t N,
                                       int C, int H, int W, int normalize, float *grad_pred, const int64_t grad_pred_strides[4],
                                       void *stream) {
    if (!grad_out || !params || !workspace || !grad_pred || !grad_pred_strides)
        return fail(EBFI_ERR_ARG, "lpips_vgg_backward: null argument");
    if (N < 0 || (C != 1 && C != 3) || H < VG_MIN || W < VG_MIN)
        return fail(EBFI_ERR_ARG, "lpips_vgg_backward: bad shape N=%lld C=%d H=%d W=%d (C in {1, 3}; H, W >= %d)", (long long)N, C, H, W,
                    VG_MIN);
    if (grad_pred_strides[3] != 1)
        return fail(EBFI_ERR_ARG, "lpips_vgg_backward: the column stride must be 1 (got %lld)", (long long)grad_pred_strides[3]);
    if (!shape_ok(N, C, H, W))
        return fail(EBFI_ERR_ARG, "lpips_vgg_backward: N=%lld pairs of %d x %d in one call (at most 16384 pairs of %lld pixels)",
                    (long long)N, H, W, (long long)VG_MAX_PIXELS);
    const WsLayout wl = ws_layout(N, C, H, W);
    const TrainLayout tl = train_layout(N, C, H, W, wl);
    if (workspace_bytes < tl.total)
        return fail(EBFI_ERR_WORKSPACE, "lpips_vgg_backward: workspace %lld bytes, %lld needed", (long long)workspace_bytes,
                    (long long)tl.total);
    if (!aligned16(workspace) || !aligned16(params))
        return fail(EBFI_ERR_ARG, "lpips_vgg_backward: workspace / params must be 16-byte aligned");
    if (N == 0) return EBFI_OK;
    const ParamLayout pl = param_layout();
    const float *prm = static_cast<const float *>(params);
    char *ws = static_cast<char *>(workspace);
    float *g[2] = {reinterpret_cast<float *>(ws + tl.map[0]), reinterpret_cast<float *>(ws + tl.map[1])};
    float *gx = reinterpret_cast<float *>(ws + tl.xin);       // the pred images' x' is dead: its gradient takes the place
    hipStream_t st = static_cast<hipStream_t>(stream);

    int cur = 0;                        // the gradient map written next
    const float *gpool = nullptr;       // the gradient of the pooled map of layer l, from block l + 1
    int rc;
    for (int l = LP_LAYERS - 1; l >= 0; --l) {
        const int h = wl.H[l], w = wl.W[l];
        TapBwdArgs a;
        a.f0 = reinterpret_cast<const float *>(ws + tl.saved[VG_LAST[l]]);
        a.f1 = reinterpret_cast<const float *>(ws + tl.ttap[l]);
        a.head = prm + pl.h[l], a.gpool = gpool, a.grad_out = grad_out, a.gf = g[cur];
        a.C = VG_TAPC[l], a.H = h, a.W = w;
        {
            // both maps read twice, the gradient written once, a quarter of a map read from the pool
            const double values = (double)N * VG_TAPC[l] * h * w;
            ProfScope ps("lpips_vgg_tap_bwd", st, 0.0, 4.0 * values * (5.0 + (gpool ? 0.25 : 0.0)));
            const dim3 grid((unsigned)(wl.tile0[l + 1] - wl.tile0[l]), (unsigned)N);
            if (w % 2 == 0) hipLaunchKernelGGL(lpips_vgg_tap_bwd_kernel<true>, grid, dim3(LP_THREADS), 0, st, a);
            else hipLaunchKernelGGL(lpips_vgg_tap_bwd_kernel<false>, grid, dim3(LP_THREADS), 0, st, a);
        }
        rc = check_launch("lpips_vgg_tap_bwd");
        if (rc != EBFI_OK) return rc;
        const float *gsrc = g[cur];
        cur ^= 1;
        const int first = l ? VG_LAST[l - 1] + 1 : 0;
        for (int conv = VG_LAST[l]; conv >= first; --conv) {
            // the ReLU mask from the saved output: activation 1 (LeakyReLU) at slope 0
            float *dst = conv == 0 ? gx : g[cur];
            rc = ebfi_conv2d_backward_data(gsrc, ws + tl.saved[conv], prm + pl.w[conv], dst, (int)N, VG_CIN[conv], h, w, VG_COUT[conv],
                                           3, 1, 1, 1, 0.f, EBFI_F32, stream);
            if (rc != EBFI_OK) return rc;
            gsrc = dst;
            if (conv != 0) cur ^= 1;
        }
        gpool = gsrc;
    }
    {
        EpilogueArgs a;
        a.gx = gx, a.flags = reinterpret_cast<const int *>(ws + tl.flags), a.grad_pred = grad_pred;
        for (int d = 0; d < 3; ++d) a.gs[d] = grad_pred_strides[d];
        a.N = (int)N, a.C = C, a.H = H, a.W = W, a.strips = wl.strips;
        float add[3];
        input_scale(normalize, a.mul, add);
        ProfScope ps("lpips_vgg_epilogue", st, 0.0, 4.0 * N * (C + (C == 3 ? 3.0 : 9.0)) * H * (double)W);
        hipLaunchKernelGGL(lpips_vgg_epilogue_kernel, dim3((unsigned)wl.strips, (unsigned)C, (unsigned)N), dim3(LP_THREADS), 0, st, a);
    }
    return check_launch("lpips_vgg_epilogue");
}
