// The element-wise and gather kernels of the frame-upsampling step (generate_dataset/upsampling/upsample.py: the Vid2E adaptive
// upsampler around two Super-SloMo U-Nets).  The convolutions are csrc/conv2d.hip's; what is here is everything between them, at
// batch 1 and on planar [C, H, W] float32 tensors.  The law is written out in include/ebfi_hip.h (ebfi_slomo_*) and restated in
// float64 by tests/upsample_ref.py.
//
//   avgpool2 / bilinear_up2   the U-Net's 2x2 average pool and its bilinear x2 (align_corners = True) up-sampling
//   flow_max_magnitude        max over both flows of sqrt(u^2 + v^2): the one scalar the host reads per pair (N = ceil of it)
//   slomo_assemble            I0, I1, flowOut, t -> the 20-channel input of the interpolation network, both back-warps inside
//   slomo_blend               interpolation output + that tensor + t -> the float frame Ft_p + mean and its gray bytes
//   slomo_frame_u8            the tail of the blend alone: a normalised float frame -> gray bytes (I0, and the byte-law test)
//
// Memory-bound passes and gathers: one lane owns FOUR adjacent pixels of a row, so every contiguous side is a 16-byte load or
// store (4 bytes for the gray quad); the gathers of a back-warp read two source rows around where the lane's neighbours read.
// The vector forms need W % 4 == 0 and 16-byte aligned tensors; the pool, the up-sampling, the maximum and frame_u8 have a
// scalar form for everything else (the 1 x 1 and 2 x 3 maps at the bottom of the U-Net), assemble and blend require W % 4 == 0
// (the reader crops to multiples of 32).
//
// Rounding.  The byte law (+ mean, * 255, clip, truncate, gray) decides bytes, so the float32 order of the reference is kept and
// contraction is switched off for this file, as in esim.hip; sqrt and the division are hipcc's correctly rounded defaults.
//
// Gray.  GRAY15 below is OpenCV 4's 8-bit cvtColor(BGR2GRAY) fixed point as read from OpenCV's source (color_rgb: B 3735,
// G 19235, R 9798 over 2^15, round to nearest).  It has NOT been checked against a cv2 build: cv2 is installed nowhere this
// project is built or tested.  It is a different function from the 14-bit law esim.hip restates.  The reference hands cvtColor
// an RGB frame under the BGR code, so channel 0 (R) takes the blue coefficient; that is kept.
#include <cmath>

#include "common.hpp"

#pragma clang fp contract(off)

using namespace ebfi;

namespace {

constexpr int kThreads = 256;
__device__ constexpr int GRAY15[3] = {3735, 19235, 9798};   // coefficients of channel 0, 1, 2 as cvtColor(BGR2GRAY) sees them; shift 15
constexpr int GRAY15_SHIFT = 15;
__device__ constexpr float kMean[3] = {0.429f, 0.431f, 0.397f};   // const.py mean, RGB order

struct f4 {
    float v[4];
};

// four consecutive floats at p[i .. i + 3]; `vec`: one 16-byte load (i % 4 == 0, p aligned); else scalar loads below `n`
__device__ inline f4 load4(const float *__restrict__ p, int64_t i, int64_t n, bool vec) {
    f4 r;
    if (vec) {
        const float4 q = *reinterpret_cast<const float4 *>(p + i);
        r.v[0] = q.x, r.v[1] = q.y, r.v[2] = q.z, r.v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) r.v[k] = i + k < n ? p[i + k] : 0.f;
    }
    return r;
}

__device__ inline void store4(float *__restrict__ p, int64_t i, int64_t n, bool vec, const f4 &r) {
    if (vec) {
        *reinterpret_cast<float4 *>(p + i) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k < n) p[i + k] = r.v[k];
    }
}

// ---------------------------------------------------------------------------------------------- pool and up-sampling
// grid: ceil(C * Ho * ceil(Wo / 4) / kThreads); a lane owns outputs (c, yo, 4 q .. 4 q + 3)
__global__ __launch_bounds__(kThreads) void avgpool2_kernel(const float *__restrict__ x, float *__restrict__ out, int C, int Ho,
                                                            int Wo, int vec) {
    const int nq = (Wo + 3) / 4;
    const int64_t total = (int64_t)C * Ho * nq;
    const int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (id >= total) return;
    const int q = (int)(id % nq);
    const int64_t row = id / nq;               // c * Ho + yo
    const int W = 2 * Wo;
    const float *r0 = x + row * 2 * W, *r1 = r0 + W;
    f4 o;
    if (vec) {
        const f4 a0 = load4(r0, 8 * q, W, true), a1 = load4(r0, 8 * q + 4, W, true);
        const f4 b0 = load4(r1, 8 * q, W, true), b1 = load4(r1, 8 * q + 4, W, true);
        o.v[0] = (a0.v[0] + a0.v[1] + b0.v[0] + b0.v[1]) * 0.25f;
        o.v[1] = (a0.v[2] + a0.v[3] + b0.v[2] + b0.v[3]) * 0.25f;
        o.v[2] = (a1.v[0] + a1.v[1] + b1.v[0] + b1.v[1]) * 0.25f;
        o.v[3] = (a1.v[2] + a1.v[3] + b1.v[2] + b1.v[3]) * 0.25f;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xo = 4 * q + k;
            o.v[k] = xo < Wo ? (r0[2 * xo] + r0[2 * xo + 1] + r1[2 * xo] + r1[2 * xo + 1]) * 0.25f : 0.f;
        }
    }
    store4(out + row * Wo, 4 * q, Wo, vec != 0, o);
}

// x [C, H, W] -> out [C, 2H, 2W], align_corners = True: source coordinate = o * (n - 1) / (2n - 1) (0 for n = 1)
__global__ __launch_bounds__(kThreads) void bilinear_up2_kernel(const float *__restrict__ x, float *__restrict__ out, int C, int H,
                                                                int W, float sy, float sx, int vec) {
    const int Ho = 2 * H, Wo = 2 * W;
    const int nq = (Wo + 3) / 4;
    const int64_t total = (int64_t)C * Ho * nq;
    const int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (id >= total) return;
    const int q = (int)(id % nq);
    const int64_t row = id / nq;               // c * Ho + yo
    const int yo = (int)(row % Ho);
    const int64_t c = row / Ho;
    const float fy = sy * (float)yo;
    const int y0 = min((int)fy, H - 1);
    const int y1 = y0 < H - 1 ? y0 + 1 : y0;
    const float ly = fy - (float)y0, hy = 1.f - ly;
    const float *r0 = x + (c * H + y0) * W, *r1 = x + (c * H + y1) * W;
    // the source step is below 1/2, so the four outputs of a lane read at most four consecutive source columns of each row:
    // eight loads instead of sixteen, the per-output columns chosen from registers
    const int xb = min((int)(sx * (float)(4 * q)), W - 1);
    float a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int xc = min(xb + j, W - 1);
        a[j] = r0[xc];
        b[j] = r1[xc];
    }
    auto pick = [](const float (&r)[4], int d) { return d == 0 ? r[0] : (d == 1 ? r[1] : (d == 2 ? r[2] : r[3])); };
    f4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xo = 4 * q + k;
        float v = 0.f;
        if (xo < Wo) {
            const float fx = sx * (float)xo;
            const int x0 = min((int)fx, W - 1);
            const int d0 = min(max(x0 - xb, 0), 2), d1 = x0 < W - 1 ? d0 + 1 : d0;
            const float lx = fx - (float)x0, hx = 1.f - lx;
            v = hy * (hx * pick(a, d0) + lx * pick(a, d1)) + ly * (hx * pick(b, d0) + lx * pick(b, d1));
        }
        o.v[k] = v;
    }
    store4(out + row * Wo, 4 * q, Wo, vec != 0, o);
}

// ---------------------------------------------------------------------------------------------- maximum flow magnitude
// flow [4, HW] = (u01, v01, u10, v10); *out_bits holds the running maximum as the bit pattern of a non-negative float (such
// patterns order as unsigned integers), zeroed by the host before the launch: wave shuffle, LDS across the waves, then ONE
// integer atomic per workgroup.  A NaN magnitude has a pattern above +inf and wins: the host refuses a non-finite result.
__global__ __launch_bounds__(kThreads) void flow_max_kernel(const float *__restrict__ flow, int64_t HW, unsigned *out_bits,
                                                            int vec) {
    __shared__ unsigned part[kThreads / 64];
    const int64_t nq = (HW + 3) / 4;
    unsigned best = 0u;
    for (int64_t qd = (int64_t)blockIdx.x * kThreads + threadIdx.x; qd < nq; qd += (int64_t)gridDim.x * kThreads) {
        const int64_t i = 4 * qd;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const f4 u = load4(flow + (2 * f) * HW, i, HW, vec != 0), v = load4(flow + (2 * f + 1) * HW, i, HW, vec != 0);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float uu = u.v[k] * u.v[k], vv = v.v[k] * v.v[k];
                const unsigned b = __float_as_uint(sqrtf(uu + vv));   // (lanes past HW loaded zeros: magnitude +0)
                best = b > best ? b : best;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)best, off, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) best = part[w] > best ? part[w] : best;
        atomicMax(out_bits, best);
    }
}

// ---------------------------------------------------------------------------------------------- back-warp
// The reference's backWarp: x = 2 * ((gx + u) / W - 0.5), grid_sample(bilinear, zeros, align_corners = True), i.e. the pixel
// coordinate ((x + 1) / 2) * (W - 1) -- (gx + u) * (W - 1) / W up to rounding: zero flow is not the identity.
struct Taps {
    int o[4];       // offsets inside a plane of the four corners (nw, ne, sw, se); -1 = outside (zero padding)
    float w[4];
};

__device__ inline Taps warp_taps(int gx, int gy, float u, float v, int H, int W) {
    Taps t;
    float cx = (float)gx + u, cy = (float)gy + v;
    cx = 2.f * (cx / (float)W - 0.5f);
    cy = 2.f * (cy / (float)H - 0.5f);
    const float ix = ((cx + 1.f) / 2.f) * (float)(W - 1), iy = ((cy + 1.f) / 2.f) * (float)(H - 1);
    const float fx = floorf(ix), fy = floorf(iy);
#pragma unroll
    for (int k = 0; k < 4; ++k) t.o[k] = -1, t.w[k] = 0.f;
    // every corner outside (or a non-finite coordinate): nothing is read
    if (!(fx >= -1.f && fx <= (float)(W - 1) && fy >= -1.f && fy <= (float)(H - 1))) return t;
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    const float wx1 = ix - fx, wx0 = (fx + 1.f) - ix, wy1 = iy - fy, wy0 = (fy + 1.f) - iy;
    const bool xin0 = x0 >= 0, xin1 = x1 < W, yin0 = y0 >= 0, yin1 = y1 < H;   // (x0 <= W - 1 and x1 >= 0 hold already)
    if (xin0 && yin0) t.o[0] = y0 * W + x0;
    if (xin1 && yin0) t.o[1] = y0 * W + x1;
    if (xin0 && yin1) t.o[2] = y1 * W + x0;
    if (xin1 && yin1) t.o[3] = y1 * W + x1;
    t.w[0] = wx0 * wy0, t.w[1] = wx1 * wy0, t.w[2] = wx0 * wy1, t.w[3] = wx1 * wy1;
    return t;
}

__device__ inline float warp_sample(const float *__restrict__ plane, const Taps &t) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (t.o[k] >= 0) s = s + plane[t.o[k]] * t.w[k];
    return s;
}

struct TimeCoeff {   // float32 images of the reference's Python-double coefficients
    float c00, c01, c10, c11;   // F_t_0 = c00 F_0_1 + c01 F_1_0;  F_t_1 = c10 F_0_1 + c11 F_1_0
    float w0, w1;               // 1 - t, t
};

// grid: ceil(H * W / 4 / kThreads); a lane owns pixels (y, 4 q .. 4 q + 3).  out: [20, H, W]
//   0-2 I0 | 3-5 I1 | 6-7 F_0_1 | 8-9 F_1_0 | 10-11 F_t_1 | 12-13 F_t_0 | 14-16 warp(I1, F_t_1) | 17-19 warp(I0, F_t_0)
__global__ __launch_bounds__(kThreads) void slomo_assemble_kernel(const float *__restrict__ I0, const float *__restrict__ I1,
                                                                  const float *__restrict__ flow, TimeCoeff tc,
                                                                  float *__restrict__ out, int H, int W) {
    const int64_t HW = (int64_t)H * W;
    const int64_t i = 4 * ((int64_t)blockIdx.x * kThreads + threadIdx.x);
    if (i >= HW) return;
    const int y = (int)(i / W), x = (int)(i % W);
    f4 fl[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        fl[c] = load4(flow + c * HW, i, HW, true);
        store4(out + (6 + c) * HW, i, HW, true, fl[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        store4(out + c * HW, i, HW, true, load4(I0 + c * HW, i, HW, true));
        store4(out + (3 + c) * HW, i, HW, true, load4(I1 + c * HW, i, HW, true));
    }
    f4 ft0[2], ft1[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ft0[c].v[k] = tc.c00 * fl[c].v[k] + tc.c01 * fl[2 + c].v[k];
            ft1[c].v[k] = tc.c10 * fl[c].v[k] + tc.c11 * fl[2 + c].v[k];
        }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        store4(out + (10 + c) * HW, i, HW, true, ft1[c]);
        store4(out + (12 + c) * HW, i, HW, true, ft0[c]);
    }
    f4 g1[3], g0[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const Taps t1 = warp_taps(x + k, y, ft1[0].v[k], ft1[1].v[k], H, W);
        const Taps t0 = warp_taps(x + k, y, ft0[0].v[k], ft0[1].v[k], H, W);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            g1[c].v[k] = warp_sample(I1 + c * HW, t1);
            g0[c].v[k] = warp_sample(I0 + c * HW, t0);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        store4(out + (14 + c) * HW, i, HW, true, g1[c]);
        store4(out + (17 + c) * HW, i, HW, true, g0[c]);
    }
}

// ---------------------------------------------------------------------------------------------- the byte law
// frame value (normalised) -> + mean -> * 255 -> clip to [0, 255] -> truncate; a NaN gives 0
__device__ inline int to_level(float v, float mean, float *plus_mean) {
    const float m = v + mean;
    *plus_mean = m;
    const float s = 255.f * m;
    const float c = fminf(fmaxf(s, 0.f), 255.f);
    return (int)c;
}

__device__ inline unsigned char gray_of(int c0, int c1, int c2) {
    return (unsigned char)((GRAY15[0] * c0 + GRAY15[1] * c1 + GRAY15[2] * c2 + (1 << (GRAY15_SHIFT - 1))) >> GRAY15_SHIFT);
}

__device__ inline void store_gray4(unsigned char *__restrict__ g, int64_t i, int64_t n, bool vec, const unsigned char b[4]) {
    if (vec) {
        *reinterpret_cast<uchar4 *>(g + i) = make_uchar4(b[0], b[1], b[2], b[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k < n) g[i + k] = b[k];
    }
}

__global__ __launch_bounds__(kThreads) void slomo_frame_u8_kernel(const float *__restrict__ frame, unsigned char *__restrict__ gray,
                                                                  int64_t HW, int vec) {
    const int64_t i = 4 * ((int64_t)blockIdx.x * kThreads + threadIdx.x);
    if (i >= HW) return;
    int lv[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const f4 v = load4(frame + c * HW, i, HW, vec != 0);
        float unused;
#pragma unroll
        for (int k = 0; k < 4; ++k) lv[c][k] = to_level(v.v[k], kMean[c], &unused);
    }
    unsigned char b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = gray_of(lv[0][k], lv[1][k], lv[2][k]);
    store_gray4(gray, i, HW, vec != 0, b);
}

// intrp [5, H, W] (the interpolation network's output), x20 as slomo_assemble wrote it -> rgb [3, H, W] = Ft_p + mean (optional)
// and gray [H, W]
__global__ __launch_bounds__(kThreads) void slomo_blend_kernel(const float *__restrict__ intrp, const float *__restrict__ x20,
                                                               TimeCoeff tc, float *__restrict__ rgb,
                                                               unsigned char *__restrict__ gray, int H, int W) {
    const int64_t HW = (int64_t)H * W;
    const int64_t i = 4 * ((int64_t)blockIdx.x * kThreads + threadIdx.x);
    if (i >= HW) return;
    const int y = (int)(i / W), x = (int)(i % W);
    const float *I0 = x20, *I1 = x20 + 3 * HW;
    f4 io[5], ft1[2], ft0[2];
#pragma unroll
    for (int c = 0; c < 5; ++c) io[c] = load4(intrp + c * HW, i, HW, true);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        ft1[c] = load4(x20 + (10 + c) * HW, i, HW, true);
        ft0[c] = load4(x20 + (12 + c) * HW, i, HW, true);
    }
    f4 px[3];
    unsigned char b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float u0 = io[0].v[k] + ft0[0].v[k], v0 = io[1].v[k] + ft0[1].v[k];
        const float u1 = io[2].v[k] + ft1[0].v[k], v1 = io[3].v[k] + ft1[1].v[k];
        const float V0 = 1.f / (1.f + expf(-io[4].v[k]));
        const float V1 = 1.f - V0;
        const Taps t0 = warp_taps(x + k, y, u0, v0, H, W), t1 = warp_taps(x + k, y, u1, v1, H, W);
        const float a0 = tc.w0 * V0, a1 = tc.w1 * V1;
        const float den = a0 + a1;
        int lv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float g0 = warp_sample(I0 + c * HW, t0), g1 = warp_sample(I1 + c * HW, t1);
            const float p = (a0 * g0 + a1 * g1) / den;
            lv[c] = to_level(p, kMean[c], &px[c].v[k]);
        }
        b[k] = gray_of(lv[0], lv[1], lv[2]);
    }
    if (rgb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) store4(rgb + c * HW, i, HW, true, px[c]);
    }
    store_gray4(gray, i, HW, true, b);
}

int check_plane(const char *what, int C, int H, int W) {
    if (C < 1 || H < 1 || W < 1) return fail(EBFI_ERR_ARG, "%s: C = %d, H = %d, W = %d must be positive", what, C, H, W);
    if ((int64_t)C * H * W >= ((int64_t)1 << 31)) return fail(EBFI_ERR_ARG, "%s: %d x %d x %d elements exceed 2^31", what, C, H, W);
    return EBFI_OK;
}

int check_frame(const char *what, int H, int W, bool quads) {
    if (int rc = check_plane(what, 20, H, W)) return rc;
    if (H < 2 || W < 2) return fail(EBFI_ERR_ARG, "%s: H = %d, W = %d: a frame has at least 2 x 2 pixels", what, H, W);
    if (quads && W % 4 != 0) return fail(EBFI_ERR_ARG, "%s: W = %d is no multiple of 4 (the reader crops to multiples of 32)", what, W);
    return EBFI_OK;
}

TimeCoeff time_coeff(double t) {   // the reference forms these as Python doubles; the tensors then take their float32 images
    const double temp = -t * (1 - t);
    return TimeCoeff{(float)temp, (float)(t * t), (float)((1 - t) * (1 - t)), (float)temp, (float)(1 - t), (float)t};
}

}  // namespace

extern "C" int ebfi_avgpool2_forward(const float *x, float *out, int C, int H, int W, void *stream) {
    if (!x || !out) return fail(EBFI_ERR_ARG, "avgpool2_forward: null pointer");
    if (int rc = check_plane("avgpool2_forward", C, H, W)) return rc;
    if ((H | W) & 1) return fail(EBFI_ERR_ARG, "avgpool2_forward: H = %d, W = %d must be even", H, W);
    const int Ho = H / 2, Wo = W / 2;
    const int vec = Wo % 4 == 0 && aligned16(x) && aligned16(out);
    const int64_t total = (int64_t)C * Ho * ((Wo + 3) / 4);
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("avgpool2", st, 0.0, 5.0 * C * (double)Ho * Wo * 4.0);
        hipLaunchKernelGGL(avgpool2_kernel, dim3((unsigned)ceil_div(total, kThreads)), dim3(kThreads), 0, st, x, out, C, Ho, Wo, vec);
    }
    return check_launch("avgpool2_forward");
}

extern "C" int ebfi_bilinear_up2_forward(const float *x, float *out, int C, int H, int W, void *stream) {
    if (!x || !out) return fail(EBFI_ERR_ARG, "bilinear_up2_forward: null pointer");
    if (int rc = check_plane("bilinear_up2_forward", 4 * C, H, W)) return rc;
    const int vec = (2 * W) % 4 == 0 && aligned16(out);
    const float sy = (float)(H - 1) / (float)(2 * H - 1), sx = (float)(W - 1) / (float)(2 * W - 1);
    const int64_t total = (int64_t)C * 2 * H * ((2 * W + 3) / 4);
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("bilinear_up2", st, 0.0, 5.0 * C * (double)H * W * 4.0);
        hipLaunchKernelGGL(bilinear_up2_kernel, dim3((unsigned)ceil_div(total, kThreads)), dim3(kThreads), 0, st, x, out, C, H, W, sy,
                           sx, vec);
    }
    return check_launch("bilinear_up2_forward");
}

extern "C" int ebfi_flow_max_magnitude(const float *flow, int H, int W, float *out, void *stream) {
    if (!flow || !out) return fail(EBFI_ERR_ARG, "flow_max_magnitude: null pointer");
    if (int rc = check_plane("flow_max_magnitude", 4, H, W)) return rc;
    const int64_t HW = (int64_t)H * W;
    const int vec = HW % 4 == 0 && aligned16(flow);
    int64_t blocks = ceil_div(ceil_div(HW, 4), kThreads);
    if (blocks > 1024) blocks = 1024;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(out, 0, sizeof(float), st) != hipSuccess) return fail(EBFI_ERR_LAUNCH, "flow_max_magnitude: hipMemsetAsync failed");
    {
        ProfScope ps_("flow_max", st, 0.0, 16.0 * (double)HW);
        hipLaunchKernelGGL(flow_max_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, flow, HW, reinterpret_cast<unsigned *>(out), vec);
    }
    return check_launch("flow_max_magnitude");
}

extern "C" int ebfi_slomo_assemble(const float *I0, const float *I1, const float *flow, double t, float *out20, int H, int W,
                                   void *stream) {
    if (!I0 || !I1 || !flow || !out20) return fail(EBFI_ERR_ARG, "slomo_assemble: null pointer");
    if (int rc = check_frame("slomo_assemble", H, W, true)) return rc;
    if (!(t > 0.0 && t < 1.0)) return fail(EBFI_ERR_ARG, "slomo_assemble: t = %g outside (0, 1)", t);
    if (!aligned16(I0) || !aligned16(I1) || !aligned16(flow) || !aligned16(out20))
        return fail(EBFI_ERR_ARG, "slomo_assemble: tensors must be 16-byte aligned");
    const int64_t HW = (int64_t)H * W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("slomo_assemble", st, 0.0, (10.0 + 20.0) * 4.0 * (double)HW);
        hipLaunchKernelGGL(slomo_assemble_kernel, dim3((unsigned)ceil_div(HW / 4, kThreads)), dim3(kThreads), 0, st, I0, I1, flow,
                           time_coeff(t), out20, H, W);
    }
    return check_launch("slomo_assemble");
}

extern "C" int ebfi_slomo_blend(const float *intrp, const float *x20, double t, float *rgb, uint8_t *gray, int H, int W, void *stream) {
    if (!intrp || !x20 || !gray) return fail(EBFI_ERR_ARG, "slomo_blend: null pointer");
    if (int rc = check_frame("slomo_blend", H, W, true)) return rc;
    if (!(t > 0.0 && t < 1.0)) return fail(EBFI_ERR_ARG, "slomo_blend: t = %g outside (0, 1)", t);
    if (!aligned16(intrp) || !aligned16(x20) || (rgb && !aligned16(rgb)) || (reinterpret_cast<uintptr_t>(gray) & 3u))
        return fail(EBFI_ERR_ARG, "slomo_blend: float tensors must be 16-byte aligned, the gray frame 4-byte aligned");
    const int64_t HW = (int64_t)H * W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("slomo_blend", st, 0.0, ((5.0 + 10.0 + (rgb ? 3.0 : 0.0)) * 4.0 + 1.0) * (double)HW);
        hipLaunchKernelGGL(slomo_blend_kernel, dim3((unsigned)ceil_div(HW / 4, kThreads)), dim3(kThreads), 0, st, intrp, x20,
                           time_coeff(t), rgb, gray, H, W);
    }
    return check_launch("slomo_blend");
}

extern "C" int ebfi_slomo_frame_u8(const float *frame, uint8_t *gray, int H, int W, void *stream) {
    if (!frame || !gray) return fail(EBFI_ERR_ARG, "slomo_frame_u8: null pointer");
    if (int rc = check_plane("slomo_frame_u8", 3, H, W)) return rc;
    const int64_t HW = (int64_t)H * W;
    const int vec = HW % 4 == 0 && aligned16(frame) && (reinterpret_cast<uintptr_t>(gray) & 3u) == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("slomo_frame_u8", st, 0.0, 13.0 * (double)HW);
        hipLaunchKernelGGL(slomo_frame_u8_kernel, dim3((unsigned)ceil_div(ceil_div(HW, 4), kThreads)), dim3(kThreads), 0, st, frame, gray,
                           HW, vec);
    }
    return check_launch("slomo_frame_u8");
}
