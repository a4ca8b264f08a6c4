// The two ends of an inference run on recorded clips: stored uint8 frames -> the planar fp32 tensor the network reads
// (dataloader/h5dataset_realdata.py:178-189: `torch.from_numpy(frames).permute(0, 3, 1, 2).float() / 255`, with the crop
// and the flips of AugmentData folded into the read), and restored planar fp32 frames -> the interleaved uint8 image the
// reference saves (infer_ours.py:135: `(x.clamp(0, 1) * 255).astype('uint8')`, a truncating cast).
//
// The training reader's form of the first (period_frames_u8) also writes the blurry input the synthetic-blur dataset feeds,
// `torch.from_numpy(frames[:e].mean(0)).permute(2, 0, 1).float() / 255` (dataloader/h5dataset.py:311), in the same pass.
//
// All are pure streaming kernels: one thread owns FOUR consecutive pixels of one row in all three channels, so the planar
// side moves as three 16-byte accesses per thread (64 lanes x 16 B = 1 KiB per wave instruction) and the interleaved side as
// 12 consecutive bytes.  The 16-byte form needs the planar base 16-byte aligned and every planar row start a multiple of four
// floats; the 4-byte form of the interleaved side needs its base and strides multiples of four bytes.  Both are decided on the
// HOST from the actual pointers and strides; anything else (a ragged width, a view that starts mid-row, a byte-offset source)
// takes the scalar path, which makes no alignment assumption at all.  Offsets are 64-bit element offsets throughout.
//
// Numerics.  byte / 255.0f is one correctly rounded fp32 division (hipcc's default; the library is built without fast-math
// flags), which is what the CPU expression computes: bit-identical for all 256 byte values.  The way back is
// min(max(x, 0), 1) * 255.0f -- one fp32 multiply -- truncated towards zero; NaN maps to 0 (the comparisons below are false
// for it), which numpy leaves undefined.  The blurry mean rounds three times and the kernel rounds in the same places: the byte
// sum is an exact integer, sum / e is a float64 division (numpy's mean), the quotient is rounded to fp32, and that is divided
// by 255.0f.  The fused sum / (255 * e) is NOT the same function (e = 3: 167 of the 766 possible sums differ).
#include "common.hpp"

using namespace ebfi;

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 4;   // pixels per thread

struct alignas(4) Bytes12 {
    uint32_t w[3];
};

// p: first source pixel of this thread's four (ascending source order); returns the 12 interleaved bytes
template <bool SRC4>
__device__ inline void load12(const uint8_t *__restrict__ p, int64_t sp, uint8_t (&b)[12]) {
    if constexpr (SRC4) {   // pixel stride 3 and p 4-byte aligned (host-checked)
        const Bytes12 v = *reinterpret_cast<const Bytes12 *>(p);
#pragma unroll
        for (int k = 0; k < 12; ++k) b[k] = (uint8_t)(v.w[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) b[3 * k + c] = p[(int64_t)k * sp + c];
    }
}

// out [n][3][h][w] contiguous; src pixel (f, Y, X) at src + f * sn + Y * sh + X * sp, channels adjacent.
// VEC: w % 4 == 0 and `out` 16-byte aligned -> every thread owns four in-range pixels and stores float4.
template <bool VEC, bool SRC4>
__global__ __launch_bounds__(kThreads) void frames_u8_to_planar(const uint8_t *__restrict__ src, int64_t sn, int64_t sh,
                                                                int64_t sp, int64_t n, int i0, int j0, int h, int w, int rev,
                                                                int fliph, int flipv, float *__restrict__ out) {
    const int quads = (w + kPix - 1) / kPix;
    const int64_t total = n * (int64_t)h * quads;
    const int64_t plane = (int64_t)h * w;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
        const int xq = (int)(t % quads);
        const int64_t r = t / quads;
        const int y = (int)(r % h);
        const int64_t f = r / h;
        const int x = xq * kPix;
        const int Y = i0 + (flipv ? h - 1 - y : y);
        const uint8_t *row = src + f * sn + (int64_t)Y * sh;
        float *o = out + f * 3 * plane + (int64_t)y * w + x;
        if constexpr (VEC) {
            // output pixels x .. x+3 come from source pixels X0 .. X0+3, reversed under a horizontal flip
            const int X0 = fliph ? j0 + w - kPix - x : j0 + x;
            uint8_t b[12];
            load12<SRC4>(row + (int64_t)X0 * sp, sp, b);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int cs = rev ? 2 - c : c;
                float4 v;
                v.x = (float)b[3 * (fliph ? 3 : 0) + cs] / 255.0f;
                v.y = (float)b[3 * (fliph ? 2 : 1) + cs] / 255.0f;
                v.z = (float)b[3 * (fliph ? 1 : 2) + cs] / 255.0f;
                v.w = (float)b[3 * (fliph ? 0 : 3) + cs] / 255.0f;
                *reinterpret_cast<float4 *>(o + c * plane) = v;
            }
        } else {
            for (int k = 0; k < kPix && x + k < w; ++k) {
                const int X = j0 + (fliph ? w - 1 - (x + k) : x + k);
                const uint8_t *p = row + (int64_t)X * sp;
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c * plane + k] = (float)p[rev ? 2 - c : c] / 255.0f;
            }
        }
    }
}

// `torch.from_numpy(a[:e].mean(0)).float() / 255` of one sample: the exact integer sum divided by e in float64 (numpy's mean of
// a uint8 array), rounded to fp32, divided by 255 in fp32 -- three roundings, in this order.
__device__ inline float blur_mean(uint32_t sum, double n_blur) { return (float)((double)sum / n_blur) / 255.0f; }

// One period of a training item in one pass: sharp [n][3][h][w] as frames_u8_to_planar writes it, and blur [3][h][w], the mean
// of the first n_blur frames.  A thread owns four pixels of a row (window indexing as above) and walks the n frames, summing
// the bytes of the first n_blur in integers; every source byte is read once.
// VEC: w % 4 == 0 and `sharp`, `blur` 16-byte aligned.
template <bool VEC, bool SRC4>
__global__ __launch_bounds__(kThreads) void period_frames_u8(const uint8_t *__restrict__ src, int64_t sn, int64_t sh, int64_t sp,
                                                             int64_t n, int64_t n_blur, int i0, int j0, int h, int w, int rev,
                                                             int fliph, int flipv, float *__restrict__ sharp,
                                                             float *__restrict__ blur) {
    const int quads = (w + kPix - 1) / kPix;
    const int64_t total = (int64_t)h * quads;
    const int64_t plane = (int64_t)h * w;
    const double nb = (double)n_blur;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
        const int xq = (int)(t % quads);
        const int y = (int)(t / quads);
        const int x = xq * kPix;
        const int Y = i0 + (flipv ? h - 1 - y : y);
        const uint8_t *row = src + (int64_t)Y * sh;
        const int64_t at = (int64_t)y * w + x;
        uint32_t sum[12];   // [output pixel k][output channel c] at 3 * k + c
#pragma unroll
        for (int k = 0; k < 12; ++k) sum[k] = 0;
        if constexpr (VEC) {
            const int X0 = fliph ? j0 + w - kPix - x : j0 + x;
            const uint8_t *p = row + (int64_t)X0 * sp;
            for (int64_t f = 0; f < n; ++f) {
                uint8_t b[12];
                load12<SRC4>(p + f * sn, sp, b);
                float *o = sharp + f * 3 * plane + at;
                const uint32_t acc = f < n_blur ? 1u : 0u;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int cs = rev ? 2 - c : c;
                    const uint8_t b0 = b[3 * (fliph ? 3 : 0) + cs], b1 = b[3 * (fliph ? 2 : 1) + cs];
                    const uint8_t b2 = b[3 * (fliph ? 1 : 2) + cs], b3 = b[3 * (fliph ? 0 : 3) + cs];
                    sum[c] += acc * b0;
                    sum[3 + c] += acc * b1;
                    sum[6 + c] += acc * b2;
                    sum[9 + c] += acc * b3;
                    float4 v;
                    v.x = (float)b0 / 255.0f;
                    v.y = (float)b1 / 255.0f;
                    v.z = (float)b2 / 255.0f;
                    v.w = (float)b3 / 255.0f;
                    *reinterpret_cast<float4 *>(o + c * plane) = v;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float4 v;
                v.x = blur_mean(sum[c], nb);
                v.y = blur_mean(sum[3 + c], nb);
                v.z = blur_mean(sum[6 + c], nb);
                v.w = blur_mean(sum[9 + c], nb);
                *reinterpret_cast<float4 *>(blur + c * plane + at) = v;
            }
        } else {
            for (int64_t f = 0; f < n; ++f) {
                float *o = sharp + f * 3 * plane + at;
                const uint32_t acc = f < n_blur ? 1u : 0u;
#pragma unroll
                for (int k = 0; k < kPix; ++k) {
                    if (x + k < w) {
                        const int X = j0 + (fliph ? w - 1 - (x + k) : x + k);
                        const uint8_t *p = row + f * sn + (int64_t)X * sp;
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const uint8_t v = p[rev ? 2 - c : c];
                            sum[3 * k + c] += acc * v;
                            o[c * plane + k] = (float)v / 255.0f;
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kPix; ++k)
                if (x + k < w) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) blur[c * plane + at + k] = blur_mean(sum[3 * k + c], nb);
                }
        }
    }
}

__device__ inline uint32_t quantise(float x) {
    float v = x > 0.0f ? x : 0.0f;   // NaN -> 0
    v = v < 1.0f ? v : 1.0f;
    return (uint32_t)(v * 255.0f);   // truncation, like astype('uint8') of a value in [0, 255]
}

// in pixel (f, c, y, x) at in + f * sn + c * sc + y * sh + x; out [n][H][W][3] contiguous.
// VEC: W % 4 == 0, `in` 16-byte aligned, sn / sc / sh multiples of 4 -> float4 loads; OUT4: `out` 4-byte aligned -> the
// thread's 12 bytes (offset a multiple of 12) go out as three dwords.
template <bool VEC, bool OUT4>
__global__ __launch_bounds__(kThreads) void planar_to_u8(const float *__restrict__ in, int64_t sn, int64_t sc, int64_t sh,
                                                         int64_t n, int H, int W, uint8_t *__restrict__ out) {
    const int quads = (W + kPix - 1) / kPix;
    const int64_t total = n * (int64_t)H * quads;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
        const int xq = (int)(t % quads);
        const int64_t r = t / quads;
        const int y = (int)(r % H);
        const int64_t f = r / H;
        const int x = xq * kPix;
        const float *p = in + f * sn + (int64_t)y * sh + x;
        uint8_t *o = out + ((f * H + y) * (int64_t)W + x) * 3;
        if constexpr (VEC) {
            uint32_t q[12];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 v = *reinterpret_cast<const float4 *>(p + c * sc);
                q[c] = quantise(v.x);
                q[3 + c] = quantise(v.y);
                q[6 + c] = quantise(v.z);
                q[9 + c] = quantise(v.w);
            }
            if constexpr (OUT4) {
                Bytes12 v;
#pragma unroll
                for (int d = 0; d < 3; ++d)
                    v.w[d] = q[4 * d] | (q[4 * d + 1] << 8) | (q[4 * d + 2] << 16) | (q[4 * d + 3] << 24);
                *reinterpret_cast<Bytes12 *>(o) = v;
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) o[k] = (uint8_t)q[k];
            }
        } else {
            for (int k = 0; k < kPix && x + k < W; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) o[3 * k + c] = (uint8_t)quantise(p[c * sc + k]);
        }
    }
}

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

inline unsigned grid_for(int64_t threads) {
    const int64_t blocks = ceil_div(threads, kThreads);
    return (unsigned)(blocks < (1 << 20) ? blocks : (1 << 20));   // (grid-stride loops cover the rest)
}

}  // namespace

extern "C" int ebfi_frames_u8_to_planar(const uint8_t *src, const int64_t src_strides[3], int64_t n, int H0, int W0, int i,
                                        int j, int h, int w, int reverse_channels, int flip_h, int flip_v, float *out,
                                        void *stream) {
    if (!src || !out || !src_strides) return fail(EBFI_ERR_ARG, "frames_u8_to_planar: null pointer");
    if (n < 0 || H0 < 1 || W0 < 1) return fail(EBFI_ERR_ARG, "frames_u8_to_planar: bad sizes n=%lld H0=%d W0=%d", (long long)n, H0, W0);
    if (i < 0 || j < 0 || h < 1 || w < 1 || (int64_t)i + h > H0 || (int64_t)j + w > W0)
        return fail(EBFI_ERR_ARG, "frames_u8_to_planar: window (%d, %d, %d, %d) outside the %d x %d frame", i, j, h, w, H0, W0);
    const int64_t sn = src_strides[0], sh = src_strides[1], sp = src_strides[2];
    if (sn < 0 || sh < 0 || sp < 3) return fail(EBFI_ERR_ARG, "frames_u8_to_planar: strides must be >= 0 (pixel stride >= 3)");
    if (n == 0) return EBFI_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = (w % kPix == 0) && aligned16(out);
    const bool src4 = vec && aligned4(src) && sn % 4 == 0 && sh % 4 == 0 && sp == 3 && j % 4 == 0;
    const int64_t threads = n * (int64_t)h * ceil_div(w, kPix);
    const dim3 grid(grid_for(threads)), block(kThreads);
    {
        ProfScope ps_("frames_u8_to_planar", st, 0.0, (double)n * h * w * 15.0);
        if (vec && src4)
            hipLaunchKernelGGL((frames_u8_to_planar<true, true>), grid, block, 0, st, src, sn, sh, sp, n, i, j, h, w,
                               reverse_channels, flip_h, flip_v, out);
        else if (vec)
            hipLaunchKernelGGL((frames_u8_to_planar<true, false>), grid, block, 0, st, src, sn, sh, sp, n, i, j, h, w,
                               reverse_channels, flip_h, flip_v, out);
        else
            hipLaunchKernelGGL((frames_u8_to_planar<false, false>), grid, block, 0, st, src, sn, sh, sp, n, i, j, h, w,
                               reverse_channels, flip_h, flip_v, out);
    }
    return check_launch("frames_u8_to_planar");
}

extern "C" int ebfi_period_frames_u8(const uint8_t *src, const int64_t src_strides[3], int64_t n, int64_t n_blur, int H0,
                                     int W0, int i, int j, int h, int w, int reverse_channels, int flip_h, int flip_v,
                                     float *sharp, float *blur, void *stream) {
    if (!src || !sharp || !blur || !src_strides) return fail(EBFI_ERR_ARG, "period_frames_u8: null pointer");
    if (n < 1 || n_blur < 1 || n_blur > n || n_blur > (1 << 24) || H0 < 1 || W0 < 1)   // (255 * n_blur fits the 32-bit sums)
        return fail(EBFI_ERR_ARG, "period_frames_u8: bad sizes n=%lld n_blur=%lld H0=%d W0=%d (1 <= n_blur <= n)", (long long)n,
                    (long long)n_blur, H0, W0);
    if (i < 0 || j < 0 || h < 1 || w < 1 || (int64_t)i + h > H0 || (int64_t)j + w > W0)
        return fail(EBFI_ERR_ARG, "period_frames_u8: window (%d, %d, %d, %d) outside the %d x %d frame", i, j, h, w, H0, W0);
    const int64_t sn = src_strides[0], sh = src_strides[1], sp = src_strides[2];
    if (sn < 0 || sh < 0 || sp < 3) return fail(EBFI_ERR_ARG, "period_frames_u8: strides must be >= 0 (pixel stride >= 3)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = (w % kPix == 0) && aligned16(sharp) && aligned16(blur);
    const bool src4 = vec && aligned4(src) && sn % 4 == 0 && sh % 4 == 0 && sp == 3 && j % 4 == 0;
    const int64_t threads = (int64_t)h * ceil_div(w, kPix);
    const dim3 grid(grid_for(threads)), block(kThreads);
    {
        ProfScope ps_("period_frames_u8", st, 0.0, ((double)n * 15.0 + 12.0) * h * w);
        if (vec && src4)
            hipLaunchKernelGGL((period_frames_u8<true, true>), grid, block, 0, st, src, sn, sh, sp, n, n_blur, i, j, h, w,
                               reverse_channels, flip_h, flip_v, sharp, blur);
        else if (vec)
            hipLaunchKernelGGL((period_frames_u8<true, false>), grid, block, 0, st, src, sn, sh, sp, n, n_blur, i, j, h, w,
                               reverse_channels, flip_h, flip_v, sharp, blur);
        else
            hipLaunchKernelGGL((period_frames_u8<false, false>), grid, block, 0, st, src, sn, sh, sp, n, n_blur, i, j, h, w,
                               reverse_channels, flip_h, flip_v, sharp, blur);
    }
    return check_launch("period_frames_u8");
}

extern "C" int ebfi_planar_to_u8(const float *in, const int64_t in_strides[3], int64_t n, int H, int W, uint8_t *out,
                                 void *stream) {
    if (!in || !out || !in_strides) return fail(EBFI_ERR_ARG, "planar_to_u8: null pointer");
    if (n < 0 || H < 1 || W < 1) return fail(EBFI_ERR_ARG, "planar_to_u8: bad sizes n=%lld H=%d W=%d", (long long)n, H, W);
    const int64_t sn = in_strides[0], sc = in_strides[1], sh = in_strides[2];
    if (sn < 0 || sc < 0 || sh < 0) return fail(EBFI_ERR_ARG, "planar_to_u8: strides must be >= 0");
    if (n == 0) return EBFI_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = (W % kPix == 0) && aligned16(in) && sn % 4 == 0 && sc % 4 == 0 && sh % 4 == 0;
    const bool out4 = vec && aligned4(out);
    const int64_t threads = n * (int64_t)H * ceil_div(W, kPix);
    const dim3 grid(grid_for(threads)), block(kThreads);
    {
        ProfScope ps_("planar_to_u8", st, 0.0, (double)n * H * W * 15.0);
        if (vec && out4)
            hipLaunchKernelGGL((planar_to_u8<true, true>), grid, block, 0, st, in, sn, sc, sh, n, H, W, out);
        else if (vec)
            hipLaunchKernelGGL((planar_to_u8<true, false>), grid, block, 0, st, in, sn, sc, sh, n, H, W, out);
        else
            hipLaunchKernelGGL((planar_to_u8<false, false>), grid, block, 0, st, in, sn, sc, sh, n, H, W, out);
    }
    return check_launch("planar_to_u8");
}
