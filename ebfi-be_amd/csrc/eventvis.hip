// The event-count images of the evaluation loop (infer_ours.py:139-142): event_visualisation.plot_event_cnt of
// myutils/vis_events/matplotlib_plot_events.py:127-251 for the 'blue_red' and 'green_red' schemes, on the device, from the event
// stack where events_to_stack left it to the finished interleaved uint8 picture.  Bit-identical to the numpy function for every
// finite fp32 input.
//
// Stage A -- order statistics.  plot_event_cnt normalises a polarity pair by np.percentile(plane, 1) and np.percentile(plane, 99)
// of both planes.  numpy's linear method reads two ADJACENT order statistics per percentile and interpolates; which two, and
// the weight, depend only on the pixel count and are host arithmetic (percentile_rank below).  That leaves four exact order
// statistics per plane ("targets").  They are found by a radix select over an order-preserving 32-bit key of the fp32 value
// (sign flipped for non-negative values, all bits flipped for negative ones; -0 is keyed as +0), 11 + 11 + 10 bits:
//   hist<P>    every workgroup histograms the pass's digit of its slice of one plane in LDS (integer LDS adds) and merges its
//              non-zero bins into the plane's global histogram with integer atomic adds.  Pass 0 counts every value; passes 1
//              and 2 count, per target, the values whose higher digits equal the target's prefix.  Targets that share a prefix
//              (the usual case: neighbours almost always do) share one histogram, decided on the device from the prefixes.
//   select<P>  one workgroup per plane scans the merged histogram, finds each target's bin, and writes the longer prefix and the
//              rank inside that bin.  After pass 2 the prefix IS the key; one thread turns the four keys back into floats and
//              interpolates the two percentiles in numpy's operation order.
// Integer counts make every result independent of arrival order: there is no float atomic anywhere.  The general path is the
// only path: count-valued stacks (a few distinct small integers) take the same three passes, where nearly every value lands in
// one bin and the LDS adds of a wave serialise on it (not timed yet).
//
// Stage B -- colour map.  One thread owns four consecutive pixels of a row, reads both polarities (two 16-byte loads on the
// vector path) and writes 12 bytes (three dwords when the output is 4-byte aligned): the store side of planar_to_u8.
//
// Rounding.  Everything the reference does in float32 is one fp32 operation here and nothing is fused: contraction is switched
// off for this file (a + d * t must round twice, as numpy's _lerp does), the division is hipcc's correctly rounded default
// (the library is built without fast-math).  The reference's canvas is float64: `1 - x` is formed in fp32, widened, multiplied
// by 255 in double and truncated -- the same here.
#include "common.hpp"

#pragma clang fp contract(off)

using namespace ebfi;

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 4;            // pixels per thread and step
constexpr int kTargets = 4;        // order statistics per plane: the two neighbours of the 1st and of the 99th percentile
constexpr int kSliceQuads = 4096;  // quads (of four pixels) one workgroup histograms: 16 per thread

__host__ __device__ constexpr int pass_bits(int pass) { return pass == 2 ? 10 : 11; }
__host__ __device__ constexpr int pass_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__host__ __device__ constexpr int pass_bins(int pass) { return 1 << pass_bits(pass); }

// workspace, in uint32 words: per plane the three passes' histograms (all planes' first, zeroed by one memset per call), then
// per plane the two prefix / rank tables and the two percentiles
constexpr int64_t kHist0 = 0;
constexpr int64_t kHist1 = kHist0 + pass_bins(0);
constexpr int64_t kHist2 = kHist1 + (int64_t)kTargets * pass_bins(1);
constexpr int64_t kHistWords = kHist2 + (int64_t)kTargets * pass_bins(2);
constexpr int64_t kStateWords = 2 * kTargets;   // {prefix, rank} per target
constexpr int64_t kTableWords = 2 * kStateWords + 2;
constexpr int64_t kPlaneWords = kHistWords + kTableWords;

__device__ inline uint32_t key_of(float x) {
    uint32_t u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0;   // -0 == +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ inline float value_of(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// first target with the same prefix as target t (t itself when none): targets with equal prefixes share that one's histogram
__device__ inline int alias_of(const uint32_t (&prefix)[kTargets], int t) {
    for (int s = 0; s < t; ++s)
        if (prefix[s] == prefix[t]) return s;
    return t;
}

// ev value (plane pl = 2 * image + polarity, y, x) at ev + (pl / 2) * sn + (pl % 2) * sp + y * sh + x.
// grid: planes * chunks workgroups; workgroup (pl, c) owns quads [c * kSliceQuads, (c + 1) * kSliceQuads) of plane pl.
// VEC: W % 4 == 0, ev 16-byte aligned, all strides multiples of 4 (host-checked).
template <int PASS, bool VEC>
__global__ __launch_bounds__(kThreads) void eventvis_hist(const float *__restrict__ ev, int64_t sn, int64_t sp, int64_t sh, int H,
                                                          int W, int chunks, uint32_t *__restrict__ ws) {
    constexpr int B = pass_bins(PASS);
    constexpr int SHIFT = pass_shift(PASS);
    constexpr int NT = PASS == 0 ? 1 : kTargets;
    __shared__ uint32_t h[NT * B];
    const int64_t pl = blockIdx.x / chunks;
    const int chunk = (int)(blockIdx.x % chunks);
    const int64_t planes = gridDim.x / chunks;

    uint32_t prefix[kTargets] = {0, 0, 0, 0};
    bool own[kTargets] = {true, false, false, false};
    if constexpr (PASS > 0) {
        const uint32_t *st = ws + planes * kHistWords + pl * kTableWords + (PASS - 1) * kStateWords;
#pragma unroll
        for (int t = 0; t < kTargets; ++t) prefix[t] = st[2 * t];
#pragma unroll
        for (int t = 0; t < kTargets; ++t) own[t] = alias_of(prefix, t) == t;
    }
    for (int i = threadIdx.x; i < NT * B; i += kThreads) h[i] = 0;
    __syncthreads();

    const int quads = (W + kPix - 1) / kPix;
    const int64_t total = (int64_t)H * quads;
    const int64_t q0 = (int64_t)chunk * kSliceQuads;
    const int64_t q1 = q0 + kSliceQuads < total ? q0 + kSliceQuads : total;
    const float *base = ev + (pl >> 1) * sn + (pl & 1) * sp;
    for (int64_t q = q0 + threadIdx.x; q < q1; q += kThreads) {
        const int y = (int)(q / quads);
        const int x = (int)(q % quads) * kPix;
        const float *p = base + (int64_t)y * sh + x;
        uint32_t key[kPix];
        int cnt = kPix;
        if constexpr (VEC) {
            const float4 v = *reinterpret_cast<const float4 *>(p);
            key[0] = key_of(v.x), key[1] = key_of(v.y), key[2] = key_of(v.z), key[3] = key_of(v.w);
        } else {
            cnt = W - x < kPix ? W - x : kPix;
#pragma unroll
            for (int k = 0; k < kPix; ++k) key[k] = k < cnt ? key_of(p[k]) : 0u;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (!own[t]) continue;
            // equal neighbouring bins of the thread's four values go out as one add
            int cur = -1;
            uint32_t run = 0;
#pragma unroll
            for (int k = 0; k < kPix; ++k) {
                bool take = k < cnt;
                if constexpr (PASS > 0) take = take && (key[k] >> (SHIFT + pass_bits(PASS))) == prefix[t];
                const int bin = take ? (int)((key[k] >> SHIFT) & (B - 1)) : -1;
                if (bin == cur) {
                    ++run;
                } else {
                    if (cur >= 0) atomicAdd(&h[t * B + cur], run);
                    cur = bin;
                    run = 1;
                }
            }
            if (cur >= 0) atomicAdd(&h[t * B + cur], run);
        }
    }
    __syncthreads();

    uint32_t *g = ws + pl * kHistWords + (PASS == 0 ? kHist0 : PASS == 1 ? kHist1 : kHist2);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (!own[t]) continue;
        for (int i = threadIdx.x; i < B; i += kThreads) {
            const uint32_t c = h[t * B + i];
            if (c) atomicAdd(&g[t * B + i], c);
        }
    }
}

struct Ranks {
    uint32_t r[kTargets];   // 0-based ranks of the four targets in a plane: lo(1 %), hi(1 %), lo(99 %), hi(99 %)
    float g[2];             // numpy's interpolation weights of the two percentiles
};

// numpy's _lerp in float32: a + (b - a) * t, replaced by b - (b - a) * (1 - t) where t >= 0.5; every operation rounds once
__device__ inline float lerp_np(float a, float b, float t) {
    const float d = b - a;
    if (t >= 0.5f) {
        const float u = 1.0f - t;
        const float m = d * u;
        return b - m;
    }
    const float m = d * t;
    return a + m;
}

// grid: planes; one workgroup scans the plane's merged histograms of pass PASS
template <int PASS>
__global__ __launch_bounds__(kThreads) void eventvis_select(uint32_t *__restrict__ ws, Ranks ranks) {
    constexpr int B = pass_bins(PASS);
    constexpr int PER = B / kThreads;
    __shared__ uint32_t s[kThreads];
    __shared__ uint32_t keys[kTargets];
    const uint32_t *hist = ws + (int64_t)blockIdx.x * kHistWords + (PASS == 0 ? kHist0 : PASS == 1 ? kHist1 : kHist2);
    uint32_t *table = ws + (int64_t)gridDim.x * kHistWords + (int64_t)blockIdx.x * kTableWords;
    uint32_t *st_out = table + PASS * kStateWords;
    const int tid = threadIdx.x;

    uint32_t prefix[kTargets] = {0, 0, 0, 0}, rank[kTargets];
    if constexpr (PASS == 0) {
#pragma unroll
        for (int t = 0; t < kTargets; ++t) rank[t] = ranks.r[t];
    } else {
        const uint32_t *st_in = table + (PASS - 1) * kStateWords;
#pragma unroll
        for (int t = 0; t < kTargets; ++t) prefix[t] = st_in[2 * t], rank[t] = st_in[2 * t + 1];
    }
    if (tid < kTargets) keys[tid] = 0;

    for (int t = 0; t < kTargets; ++t) {
        const uint32_t *ht = hist + (PASS == 0 ? 0 : alias_of(prefix, t) * B);
        uint32_t c[PER], sum = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) sum += c[k] = ht[tid * PER + k];
        __syncthreads();   // (the previous round's readers of s are done)
        s[tid] = sum;
        __syncthreads();
        for (int off = 1; off < kThreads; off <<= 1) {
            const uint32_t v = tid >= off ? s[tid - off] : 0;
            __syncthreads();
            s[tid] += v;
            __syncthreads();
        }
        uint32_t below = s[tid] - sum;   // values in bins before this thread's
        const uint32_t r = rank[t];
        if (below <= r && r < below + sum) {   // exactly one thread: the bins' total exceeds the rank
            int k = 0;
            while (k < PER - 1 && r >= below + c[k]) below += c[k], ++k;
            const uint32_t longer = (prefix[t] << pass_bits(PASS)) | (uint32_t)(tid * PER + k);
            if constexpr (PASS < 2) {
                st_out[2 * t] = longer;
                st_out[2 * t + 1] = r - below;
            } else {
                keys[t] = longer;
            }
        }
    }
    if constexpr (PASS == 2) {
        __syncthreads();
        if (tid == 0) {
            float *pct = reinterpret_cast<float *>(table + 2 * kStateWords);
            pct[0] = lerp_np(value_of(keys[0]), value_of(keys[1]), ranks.g[0]);
            pct[1] = lerp_np(value_of(keys[2]), value_of(keys[3]), ranks.g[1]);
        }
    }
}

struct alignas(4) Bytes12 {
    uint32_t w[3];
};

__device__ inline float clip01(float x) {   // np.clip(x, 0, 1); NaN stays NaN
    x = x < 0.0f ? 0.0f : x;
    return x > 1.0f ? 1.0f : x;
}

// the reference's float64 canvas value -> byte: (canvas * 255).astype(uint8), canvas in [0, 1] (NaN never reaches the canvas)
__device__ inline uint32_t canvas_byte(float c) { return (uint32_t)(int)((double)c * 255.0); }

struct Norm {   // per image
    float pos_min, neg_min, pos_den, neg_den;
    bool pos_on, neg_on;
};

// one pixel: p, n raw counts -> three canvas bytes in the reference's canvas order (before its BGR -> RGB reversal)
template <bool GREEN, bool BLACK, bool NORM>
__device__ inline void colour(float p, float n, const Norm &nm, uint32_t (&b)[3]) {
    if constexpr (NORM) {
        if (nm.pos_on) p = (p - nm.pos_min) / nm.pos_den;
        if (nm.neg_on) n = (n - nm.neg_min) / nm.neg_den;
    } else {
        if (p >= n && p != 0.0f) {
            p = 1.0f, n = 0.0f;
        } else if (p < n && n != 0.0f) {
            n = 1.0f, p = 0.0f;
        }
    }
    p = clip01(p);
    n = clip01(n);
    const bool mp = p > 0.0f, mn = n > 0.0f;
    constexpr int POS = GREEN ? 1 : 0;   // the canvas channel of the positive polarity; the negative one is channel 2
    if constexpr (BLACK) {
        b[0] = b[1] = b[2] = 0;
        if (mp) b[POS] = canvas_byte(p);
        if (mn) b[2] = canvas_byte(n);
    } else {
        b[0] = b[1] = b[2] = 255;
        int which = -1;   // 0: drawn as positive, 1: as negative
        if (mp && n == 0.0f) which = 0;
        else if (mn && p == 0.0f) which = 1;
        else if (mp && mn) which = p >= n ? 0 : 1;
        if (which == 0) {
            const uint32_t v = canvas_byte(1.0f - p);
            b[0] = b[1] = b[2] = v;
            b[POS] = 255;
        } else if (which == 1) {
            const uint32_t v = canvas_byte(1.0f - n);
            b[0] = b[1] = v;
        }
    }
}

// out [n][H][W][3] contiguous.  VEC as in eventvis_hist; OUT4: out 4-byte aligned -> three dword stores per thread.
template <bool GREEN, bool BLACK, bool NORM, bool VEC, bool OUT4>
__global__ __launch_bounds__(kThreads) void eventvis_colour(const float *__restrict__ ev, int64_t sn, int64_t sp, int64_t sh,
                                                            int64_t n, int H, int W, int reverse,
                                                            const uint32_t *__restrict__ ws, uint8_t *__restrict__ out) {
    const int quads = (W + kPix - 1) / kPix;
    const int64_t total = n * (int64_t)H * quads;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
        const int xq = (int)(t % quads);
        const int64_t r = t / quads;
        const int y = (int)(r % H);
        const int64_t f = r / H;
        const int x = xq * kPix;
        Norm nm = {};
        if constexpr (NORM) {
            const uint32_t *tables = ws + 2 * n * kHistWords;
            const float *pp = reinterpret_cast<const float *>(tables + (2 * f) * kTableWords + 2 * kStateWords);
            const float *pn = reinterpret_cast<const float *>(tables + (2 * f + 1) * kTableWords + 2 * kStateWords);
            const float pos_min = pp[0], pos_max = pp[1], neg_min = pn[0], neg_max = pn[1];
            const float mx = pos_max > neg_max ? pos_max : neg_max;
            nm.pos_min = pos_min, nm.neg_min = neg_min;
            nm.pos_on = pos_min != mx, nm.neg_on = neg_min != mx;
            nm.pos_den = mx - pos_min, nm.neg_den = mx - neg_min;
        }
        const float *p = ev + f * sn + (int64_t)y * sh + x;
        uint8_t *o = out + ((f * H + y) * (int64_t)W + x) * 3;
        if constexpr (VEC) {
            const float4 vp = *reinterpret_cast<const float4 *>(p);
            const float4 vn = *reinterpret_cast<const float4 *>(p + sp);
            const float ps[kPix] = {vp.x, vp.y, vp.z, vp.w}, ns[kPix] = {vn.x, vn.y, vn.z, vn.w};
            uint32_t q[12];
#pragma unroll
            for (int k = 0; k < kPix; ++k) {
                uint32_t b[3];
                colour<GREEN, BLACK, NORM>(ps[k], ns[k], nm, b);
                q[3 * k] = reverse ? b[2] : b[0];
                q[3 * k + 1] = b[1];
                q[3 * k + 2] = reverse ? b[0] : b[2];
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
            for (int k = 0; k < kPix && x + k < W; ++k) {
                uint32_t b[3];
                colour<GREEN, BLACK, NORM>(p[k], p[sp + k], nm, b);
                o[3 * k] = (uint8_t)(reverse ? b[2] : b[0]);
                o[3 * k + 1] = (uint8_t)b[1];
                o[3 * k + 2] = (uint8_t)(reverse ? b[0] : b[2]);
            }
        }
    }
}

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// np.percentile(a, q) of a float32 array of n values, method 'linear': the two order statistics it reads and the weight.
// numpy forms q / 100 and the virtual index (n - 1) * q in the array's dtype, floors it, and keeps the fraction in that dtype;
// an index at or past the last element reads the last element twice.
void percentile_rank(int64_t n, float q, uint32_t *lo, uint32_t *hi, float *gamma) {
    const float frac = q / 100.0f;
    const float last = (float)(n - 1);
    const float vi = last * frac;
    if (vi >= last) {
        *lo = *hi = (uint32_t)(n - 1);
        *gamma = 0.0f;   // (the two values are the same one: the weight does not matter)
        return;
    }
    const float fl = floorf(vi);
    *lo = (uint32_t)fl;
    *hi = *lo + 1;
    *gamma = vi - fl;
}

template <bool GREEN, bool BLACK, bool NORM>
void launch_colour(bool vec, bool out4, dim3 grid, hipStream_t st, const float *ev, int64_t sn, int64_t sp, int64_t sh, int64_t n,
                   int H, int W, int reverse, const uint32_t *ws, uint8_t *out) {
    const dim3 block(kThreads);
    if (vec && out4)
        hipLaunchKernelGGL((eventvis_colour<GREEN, BLACK, NORM, true, true>), grid, block, 0, st, ev, sn, sp, sh, n, H, W, reverse,
                           ws, out);
    else if (vec)
        hipLaunchKernelGGL((eventvis_colour<GREEN, BLACK, NORM, true, false>), grid, block, 0, st, ev, sn, sp, sh, n, H, W, reverse,
                           ws, out);
    else
        hipLaunchKernelGGL((eventvis_colour<GREEN, BLACK, NORM, false, false>), grid, block, 0, st, ev, sn, sp, sh, n, H, W, reverse,
                           ws, out);
}

template <int PASS>
void launch_pass(bool vec, int64_t planes, int chunks, hipStream_t st, const float *ev, int64_t sn, int64_t sp, int64_t sh, int H,
                 int W, uint32_t *ws, const Ranks &ranks) {
    const dim3 grid((unsigned)(planes * chunks)), block(kThreads);
    {
        ProfScope ps_("eventvis_hist", st, 0.0, (double)planes * H * W * 4.0);
        if (vec)
            hipLaunchKernelGGL((eventvis_hist<PASS, true>), grid, block, 0, st, ev, sn, sp, sh, H, W, chunks, ws);
        else
            hipLaunchKernelGGL((eventvis_hist<PASS, false>), grid, block, 0, st, ev, sn, sp, sh, H, W, chunks, ws);
    }
    {
        ProfScope ps_("eventvis_select", st, 0.0, 0.0);
        hipLaunchKernelGGL((eventvis_select<PASS>), dim3((unsigned)planes), block, 0, st, ws, ranks);
    }
}

}  // namespace

extern "C" int64_t ebfi_event_cnt_image_workspace(int64_t n, int H, int W, int is_norm) {
    if (n < 0 || H < 1 || W < 1) return 0;
    if (!is_norm || n == 0) return 0;
    return 2 * n * kPlaneWords * (int64_t)sizeof(uint32_t);
}

extern "C" int ebfi_event_cnt_image(const float *ev, const int64_t ev_strides[3], int64_t n, int H, int W, int color_scheme,
                                    int is_black_background, int is_norm, int use_opencv, uint8_t *out, void *workspace,
                                    int64_t workspace_bytes, void *stream) {
    if (!ev || !out || !ev_strides) return fail(EBFI_ERR_ARG, "event_cnt_image: null pointer");
    if (n < 0 || H < 1 || W < 1) return fail(EBFI_ERR_ARG, "event_cnt_image: bad sizes n=%lld H=%d W=%d", (long long)n, H, W);
    const int64_t sn = ev_strides[0], sp = ev_strides[1], sh = ev_strides[2];
    if (sn < 0 || sp < 0 || sh < 0) return fail(EBFI_ERR_ARG, "event_cnt_image: strides must be >= 0");
    if (color_scheme == EBFI_EVENT_GRAY)
        return fail(EBFI_ERR_UNSUPPORTED, "event_cnt_image: the 'gray' scheme is not built (in the reference it only runs with "
                                          "use_opencv=True and nothing calls it)");
    if (color_scheme != EBFI_EVENT_BLUE_RED && color_scheme != EBFI_EVENT_GREEN_RED)
        return fail(EBFI_ERR_ARG, "event_cnt_image: unknown color_scheme %d", color_scheme);
    const int64_t n_pix = (int64_t)H * W;
    const int64_t planes = 2 * n;
    const int chunks = (int)ceil_div(ceil_div(W, kPix) * (int64_t)H, kSliceQuads);
    if (n_pix > INT32_MAX || planes * chunks > INT32_MAX)
        return fail(EBFI_ERR_UNSUPPORTED, "event_cnt_image: %lld images of %d x %d exceed the 32-bit counts and grid", (long long)n,
                    H, W);
    const int64_t need = ebfi_event_cnt_image_workspace(n, H, W, is_norm);
    if (need > 0) {
        if (!workspace) return fail(EBFI_ERR_WORKSPACE, "event_cnt_image: workspace missing (%lld bytes needed)", (long long)need);
        if (!aligned16(workspace)) return fail(EBFI_ERR_ARG, "event_cnt_image: workspace must be 16-byte aligned");
        if (workspace_bytes < need)
            return fail(EBFI_ERR_WORKSPACE, "event_cnt_image: workspace %lld < %lld bytes", (long long)workspace_bytes,
                        (long long)need);
    }
    if (n == 0) return EBFI_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = (W % kPix == 0) && aligned16(ev) && sn % 4 == 0 && sp % 4 == 0 && sh % 4 == 0;
    const bool out4 = vec && aligned4(out);
    uint32_t *ws = static_cast<uint32_t *>(workspace);

    if (is_norm) {
        Ranks ranks;
        percentile_rank(n_pix, 1.0f, &ranks.r[0], &ranks.r[1], &ranks.g[0]);
        percentile_rank(n_pix, 99.0f, &ranks.r[2], &ranks.r[3], &ranks.g[1]);
        // the histograms of all three passes start from zero; the tables behind them are written before they are read
        if (hipMemsetAsync(ws, 0, (size_t)(planes * kHistWords) * sizeof(uint32_t), st) != hipSuccess)
            return check_launch("event_cnt_image (memset)");
        launch_pass<0>(vec, planes, chunks, st, ev, sn, sp, sh, H, W, ws, ranks);
        launch_pass<1>(vec, planes, chunks, st, ev, sn, sp, sh, H, W, ws, ranks);
        launch_pass<2>(vec, planes, chunks, st, ev, sn, sp, sh, H, W, ws, ranks);
        const int rc = check_launch("event_cnt_image (select)");
        if (rc != EBFI_OK) return rc;
    }
    const int64_t threads = n * (int64_t)H * ceil_div(W, kPix);
    const int64_t blocks = ceil_div(threads, kThreads);
    const dim3 grid((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)));   // (grid-stride loop covers the rest)
    const int reverse = use_opencv ? 0 : 1;
    const bool green = color_scheme == EBFI_EVENT_GREEN_RED;
    {
        ProfScope ps_("eventvis_colour", st, 0.0, (double)n * n_pix * 11.0);
#define EBFI_EV_COLOUR(G, B, N) launch_colour<G, B, N>(vec, out4, grid, st, ev, sn, sp, sh, n, H, W, reverse, ws, out)
        if (green) {
            if (is_black_background) { if (is_norm) EBFI_EV_COLOUR(true, true, true); else EBFI_EV_COLOUR(true, true, false); }
            else { if (is_norm) EBFI_EV_COLOUR(true, false, true); else EBFI_EV_COLOUR(true, false, false); }
        } else {
            if (is_black_background) { if (is_norm) EBFI_EV_COLOUR(false, true, true); else EBFI_EV_COLOUR(false, true, false); }
            else { if (is_norm) EBFI_EV_COLOUR(false, false, true); else EBFI_EV_COLOUR(false, false, false); }
        }
#undef EBFI_EV_COLOUR
    }
    return check_launch("event_cnt_image");
}
